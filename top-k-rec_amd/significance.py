"""How far a rank metric moves when the test lines are drawn again, and whether two models differ by more than that (K18).

The metric values of every test line form a table X [n_lines, C] on the device (``line_table``, tkr_hip.line_metrics, from K8's ranks);
a bootstrap replicate is the column sums of n_lines rows of X drawn with replacement (``bootstrap_sums``, tkr_hip.bootstrap_sums), and a
metric is a ratio of two such sums (``values``): the same ratio rankmetrics.finish forms from the sums over all lines.  Two models' tables
side by side are resampled together -- every replicate draws the same lines for both -- which makes the comparison a paired one.

  columns(interval)             the names of X's columns
  values(sums, interval, m)     any row(s) of column sums -> {metric: values}
  interval_of(v, level)         the percentile interval of sorted replicate values
  p_value(d)                    two-sided bootstrap p of replicate differences d against 0
"""
from __future__ import annotations

import math

import numpy as np

METRICS = ('acc', 'auc', 'mrr', 'ndcg', 'map')


def n_columns(interval):
    return 3 * interval + 5


def columns(interval):
    """the names of the table's columns: hits@b, likes, auc, auc.n, rr, rr.n, ndcg@b, ap@b (b = bucket index, K_b = step * (b + 1))"""
    return (['hits@%d' % b for b in range(interval)] + ['likes', 'auc', 'auc.n', 'rr', 'rr.n'] + ['ndcg@%d' % b for b in range(interval)]
            + ['ap@%d' % b for b in range(interval)])


def gain_tables(total):
    """(gain float64 [total], ideal float64 [total + 1]): gain[r] = 1 / log2(r + 2), ideal[d] = gain[0] + ... + gain[d - 1]"""
    gain = 1.0 / np.log2(np.arange(total, dtype=np.float64) + 2.0)
    return gain, np.concatenate(([0.0], np.cumsum(gain)))


def line_table(ranks, like_ptr, rated_ptr, n_cols, step, total):
    """X float64 [n_lines, 3 * (total // step) + 5] on the device of `ranks` (int32 [n_likes], K8's output; like_ptr / rated_ptr int64
    [n_lines + 1] on the same device)"""
    import torch
    import tkr_hip
    gain, ideal = gain_tables(int(total))
    return tkr_hip.line_metrics(ranks, like_ptr, rated_ptr, n_cols, step, total, torch.from_numpy(gain).to(ranks.device),
                                torch.from_numpy(ideal).to(ranks.device))


def bootstrap_sums(X, R, seed):
    """float64 [R, C] on the device: R resamples of len(X) lines with replacement, every column summed over the same lines"""
    import tkr_hip
    return tkr_hip.bootstrap_sums(X, R, seed)


def values(sums, interval, metrics=METRICS):
    """sums float64 [C] or [R, C] (column sums of the table, of all lines or of replicates) -> {metric: float64 [interval] resp.
    [R, interval]} (auc, mrr: one value instead of `interval`).  acc = hits / likes; auc, mrr, ndcg, map = sum / their flag sum.
    ZeroDivisionError, naming the metric, where a denominator is 0 in any row"""
    s = np.asarray(sums, dtype=np.float64)
    if s.shape[-1] != n_columns(interval):
        raise ValueError('%d columns, interval = %d needs %d' % (s.shape[-1], interval, n_columns(interval)))
    i = interval
    parts = {'acc': (slice(0, i), i), 'auc': (slice(i + 1, i + 2), i + 2), 'mrr': (slice(i + 3, i + 4), i + 4),
             'ndcg': (slice(i + 5, 2 * i + 5), i + 4), 'map': (slice(2 * i + 5, 3 * i + 5), i + 4)}
    out = {}
    for m in metrics:
        num, den = parts[m]
        d = s[..., den]
        if np.any(d == 0):
            raise ZeroDivisionError('%s: no test line to average over%s' % (m, ' in a bootstrap replicate' if s.ndim > 1 else ''))
        out[m] = s[..., num] / d[..., None]
    return out


def interval_of(v, level):
    """v: R replicate values sorted ascending -> (v[j], v[R - 1 - j]), j = floor((1 - level) / 2 * R).  (1e-9 is added before the
    floor: 1 - 0.9 is 0.0999...98 in binary, and a product that is a whole number on paper must not lose its last unit to that)"""
    if not 0.0 < level < 1.0:
        raise ValueError('the level must lie inside (0, 1)')
    R = len(v)
    j = int(math.floor((1.0 - level) / 2.0 * R + 1e-9))
    return float(v[j]), float(v[R - 1 - j])


def p_value(d):
    """d: R replicate differences -> min(1, 2 min((1 + #{d <= 0}) / (R + 1), (1 + #{d >= 0}) / (R + 1)))"""
    d = np.asarray(d)
    R = len(d)
    return min(1.0, 2.0 * min((1 + int(np.count_nonzero(d <= 0))) / (R + 1), (1 + int(np.count_nonzero(d >= 0))) / (R + 1)))


def report(point, reps, interval, metrics, level, n_models=1):
    """the figures evaluate.py prints: point float64 [n_models * C] (column sums over all lines), reps [R, n_models * C] (replicates)
    -> {metric: {'lo', 'hi'[, 'vs', 'diff', 'diff.lo', 'diff.hi', 'diff.p']: list of values}} -- model 0's interval and, with two
    models, model 1's values, the difference model 0 - model 1, its interval and its p"""
    C = n_columns(interval)
    point, reps = np.asarray(point, dtype=np.float64), np.asarray(reps, dtype=np.float64)
    pa, ra = values(point[:C], interval, metrics), values(reps[:, :C], interval, metrics)
    if n_models == 2:
        pb, rb = values(point[C:2 * C], interval, metrics), values(reps[:, C:2 * C], interval, metrics)
    out = {}
    for m in metrics:
        width = pa[m].shape[-1]
        ends = [interval_of(np.sort(ra[m][:, b]), level) for b in range(width)]
        out[m] = {'lo': [e[0] for e in ends], 'hi': [e[1] for e in ends]}
        if n_models == 2:
            d = ra[m] - rb[m]
            ends = [interval_of(np.sort(d[:, b]), level) for b in range(width)]
            out[m].update({'vs': [float(x) for x in pb[m]], 'diff': [float(x) for x in pa[m] - pb[m]], 'diff.lo': [e[0] for e in ends],
                           'diff.hi': [e[1] for e in ends], 'diff.p': [p_value(d[:, b]) for b in range(width)]})
    return out
