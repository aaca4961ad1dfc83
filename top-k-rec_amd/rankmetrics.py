"""Rank metrics from the filtered ranks of the liked test columns (K8, tkr_hip.like_ranks).  Pure NumPy, no GPU.

For a test line r with likes at filtered ranks rho_0 < ... < rho_{P-1} (rated likes, rank -1, left out), C_r = n_cols - |rated_r|
unrated candidates and N_r = C_r - P of them not liked:

  acc      the reference's accuracy@k (evaluate.py:99-112): a like with rho < interval * step adds 1 to buckets rho // step ..
           interval - 1; sum of hits / sum of |likes| over ALL lines, rated likes counted in the denominator (micro average)
  auc      1 - sum_q (rho_q - q) / (P * N_r): the fraction of (like, non-like) pairs in the right order; mean over lines with
           P >= 1 and N_r >= 1
  mrr      1 / (rho_0 + 1); mean over lines with P >= 1
  ndcg@K   sum_{rho_q < K} 1 / log2(rho_q + 2)  /  sum_{q < min(P, K)} 1 / log2(q + 2),  K = step, 2 step, ..., interval * step;
           mean over lines with P >= 1
  map@K    1 / min(P, K) * sum_{rho_q < K} (q + 1) / (rho_q + 1), same K grid; mean over lines with P >= 1

``rank_sums`` returns fp64 sums and integer counts, so the sums of the shards of a scenario can be added (``add_sums``, or an
all-reduce of ``to_vector``) before ``finish`` divides.
"""
from __future__ import annotations

import numpy as np

METRICS = ('acc', 'auc', 'mrr', 'ndcg', 'map')
PER_BUCKET = ('acc', 'ndcg', 'map')          # one value per K = step, 2 step, ...; the others are one number


def rank_sums(ranks, like_ptr, rated_ptr, n_cols, step, total):
    """ranks int [n_likes] in the order of the like CSR (-1 = rated like), like_ptr / rated_ptr int64 [n_lines + 1]
    -> {metric: (sum, count)}: sums are fp64 (acc: int64 hits), arrays of `interval` = total // step entries for acc / ndcg / map"""
    ranks = np.asarray(ranks, dtype=np.int64)
    like_ptr, rated_ptr = np.asarray(like_ptr, dtype=np.int64), np.asarray(rated_ptr, dtype=np.int64)
    n = len(like_ptr) - 1
    interval = total // step
    grid = step * np.arange(1, interval + 1, dtype=np.int64)                      # K of every bucket
    line = np.repeat(np.arange(n, dtype=np.int64), np.diff(like_ptr))
    keep = ranks >= 0
    order = np.lexsort((ranks[keep], line[keep]))                                  # by line, ranks ascending inside a line
    rho, ln = ranks[keep][order], line[keep][order]
    P = np.bincount(ln, minlength=n).astype(np.int64)
    first = np.cumsum(P) - P
    q = np.arange(len(rho), dtype=np.int64) - first[ln]                           # index of the like among its line's ranked likes
    hits = np.array([np.count_nonzero(rho < K) for K in grid], dtype=np.int64)
    N = (n_cols - np.diff(rated_ptr)) - P
    ranked = P >= 1

    def per_line(weights):
        return np.bincount(ln, weights=weights, minlength=n) if len(rho) else np.zeros(n)

    pairs = ranked & (N >= 1)
    wrong = per_line((rho - q).astype(np.float64))                                 # non-likes in front of a like, summed over the likes
    auc = 1.0 - wrong[pairs] / (P[pairs] * N[pairs]).astype(np.float64)
    rr = 1.0 / (rho[q == 0] + 1.0)                                                 # one per ranked line, in line order
    gain = 1.0 / np.log2(rho + 2.0)
    ideal = np.concatenate(([0.0], np.cumsum(1.0 / np.log2(np.arange(int(P.max()) if n else 0, dtype=np.float64) + 2.0))))
    prec = (q + 1.0) / (rho + 1.0)
    ndcg, ap = np.zeros(interval), np.zeros(interval)
    for b, K in enumerate(grid):
        depth = np.minimum(P[ranked], K)
        inside = rho < K
        ndcg[b] = np.sum(per_line(np.where(inside, gain, 0.0))[ranked] / ideal[depth])
        ap[b] = np.sum(per_line(np.where(inside, prec, 0.0))[ranked] / depth)
    lines = int(np.count_nonzero(ranked))
    return {'acc': (hits, int(like_ptr[-1] - like_ptr[0])), 'auc': (float(np.sum(auc)), int(np.count_nonzero(pairs))),
            'mrr': (float(np.sum(rr)), lines), 'ndcg': (ndcg, lines), 'map': (ap, lines)}


def add_sums(a, b):
    """the sums of two shards of one scenario -> the sums of both"""
    return {m: (a[m][0] + b[m][0], a[m][1] + b[m][1]) for m in a}


def to_vector(sums):
    """-> fp64 vector for an all-reduce (counts and hits are integers below 2^53: exact)"""
    return np.concatenate([np.r_[np.asarray(sums[m][0], dtype=np.float64).reshape(-1), float(sums[m][1])] for m in METRICS])


def from_vector(vec, interval):
    out, at = {}, 0
    for m in METRICS:
        width = interval if m in PER_BUCKET else 1
        s, count = np.asarray(vec[at:at + width], dtype=np.float64), int(round(float(vec[at + width])))
        out[m] = (np.rint(s).astype(np.int64) if m == 'acc' else s.copy() if m in PER_BUCKET else float(s[0]), count)
        at += width + 1
    return out


def finish(sums, metrics=METRICS):
    """{metric: list of values}: `interval` values for acc / ndcg / map, one for auc / mrr.  ZeroDivisionError where no line counts
    (as evaluate.py:112 for acc)"""
    out = {}
    for m in metrics:
        s, c = sums[m]
        vals = [float(v) for v in np.asarray(s, dtype=np.float64).reshape(-1)]
        if c == 0:
            raise ZeroDivisionError('%s: no test line to average over' % m)
        out[m] = [v / c for v in vals]
    return out
