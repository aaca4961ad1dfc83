"""NumPy / plain-Python oracle of K18 (tkr_line_metrics, tkr_bootstrap_sums) and of the figures evaluate.py --bootstrap prints: the table
by per-line loops over the definitions, the draw through oracle/plan_np.py, resample sums in long double.  Not a test module."""
import math

import numpy as np

from oracle import plan_np as P


class Refused(ValueError):
    """what the kernel reports through its status word"""


def tables(total):
    gain = 1.0 / np.log2(np.arange(total, dtype=np.float64) + 2.0)
    return gain, np.concatenate(([0.0], np.cumsum(gain)))


def line_table(ranks, like_ptr, rated_ptr, n_cols, step, total):
    """float64 [n_lines, 3 * interval + 5], every entry one IEEE operation after the other in the stated order"""
    ranks = [int(x) for x in np.asarray(ranks)]
    like_ptr, rated_ptr = [int(x) for x in like_ptr], [int(x) for x in rated_ptr]
    n = len(like_ptr) - 1
    if like_ptr[0] != 0 or rated_ptr[0] != 0 or like_ptr[-1] > len(ranks):
        raise Refused('pointers')
    interval = total // step
    gain, ideal = tables(total)
    X = np.zeros((n, 3 * interval + 5), dtype=np.float64)
    for r in range(n):
        if like_ptr[r + 1] < like_ptr[r] or rated_ptr[r + 1] < rated_ptr[r] or rated_ptr[r + 1] - rated_ptr[r] > n_cols:
            raise Refused('pointers')
        line = ranks[like_ptr[r]:like_ptr[r + 1]]
        cap = n_cols - (rated_ptr[r + 1] - rated_ptr[r])
        if any(x < -1 for x in line):
            raise Refused('low')
        if any(x >= cap for x in line):
            raise Refused('high')
        rho = sorted(x for x in line if x >= 0)
        if len(set(rho)) != len(rho):
            raise Refused('twice')
        Pn = len(rho)
        N = cap - Pn
        X[r, interval] = float(len(line))
        if Pn >= 1 and N >= 1:
            X[r, interval + 1] = np.float64(1.0) - np.float64(sum(rho) - Pn * (Pn - 1) // 2) / np.float64(Pn * N)
            X[r, interval + 2] = 1.0
        if Pn >= 1:
            X[r, interval + 3] = np.float64(1.0) / np.float64(rho[0] + 1)
            X[r, interval + 4] = 1.0
        for b in range(interval):
            K = step * (b + 1)
            dcg, ap, hits = np.float64(0.0), np.float64(0.0), 0
            for q, x in enumerate(rho):
                if x < K:
                    hits += 1
                    dcg = dcg + gain[x]
                    ap = ap + np.float64(q + 1) / np.float64(x + 1)
            X[r, b] = float(hits)
            if Pn >= 1:
                X[r, interval + 5 + b] = dcg / ideal[min(Pn, K)]
                X[r, 2 * interval + 5 + b] = ap / np.float64(min(Pn, K))
    return X


def draw(n, r, seed):
    """idx(r, t) for t < n -> int64 [n]"""
    p = np.arange((n + 1) // 2, dtype=np.uint64)
    x, y, z, w = P.philox4x32_10(p & np.uint64(0xFFFFFFFF), p >> np.uint64(32), np.full(len(p), r, dtype=np.uint64),
                                 np.full(len(p), 3, dtype=np.uint64), seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF)
    idx = np.empty(2 * len(p), dtype=np.int64)
    idx[0::2] = P.mulhi64(x, y, n)
    idx[1::2] = P.mulhi64(z, w, n)
    return idx[:n]


def bootstrap_sums(X, R, seed, want_abs=False):
    """long double [R, C] (and, with want_abs, the sums of |x| over the same draws)"""
    X = np.asarray(X, dtype=np.float64)
    out = np.zeros((R, X.shape[1]), dtype=np.longdouble)
    mag = np.zeros((R, X.shape[1]), dtype=np.longdouble)
    for r in range(R):
        g = X[draw(len(X), r, seed)].astype(np.longdouble)
        out[r] = g.sum(0)
        mag[r] = np.abs(g).sum(0)
    return (out, mag) if want_abs else out


def values(sums, interval, metrics):
    s = np.asarray(sums, dtype=np.float64)
    i = interval
    out = {}
    for m in metrics:
        if m == 'acc':
            out[m] = [s[b] / s[i] for b in range(i)]
        elif m == 'auc':
            out[m] = [s[i + 1] / s[i + 2]]
        elif m == 'mrr':
            out[m] = [s[i + 3] / s[i + 4]]
        elif m == 'ndcg':
            out[m] = [s[i + 5 + b] / s[i + 4] for b in range(i)]
        else:
            out[m] = [s[2 * i + 5 + b] / s[i + 4] for b in range(i)]
    return out


def ends(v, level):
    v = sorted(v)
    j = int(math.floor((1.0 - level) / 2.0 * len(v) + 1e-9))          # (whole products survive the rounding of 1 - level)
    return v[j], v[len(v) - 1 - j]


def p_value(d):
    R = len(d)
    return min(1.0, 2.0 * min((1 + sum(x <= 0 for x in d)) / (R + 1), (1 + sum(x >= 0 for x in d)) / (R + 1)))


def cli_lines(scenario, XA, XB, interval, metrics, R, seed, level):
    """the lines evaluate.py --bootstrap [--compare] adds for one scenario, as (name, [values]) -- from oracle tables"""
    X = XA if XB is None else np.concatenate([XA, XB], axis=1)
    C = XA.shape[1]
    reps = bootstrap_sums(X, R, seed).astype(np.float64)
    point = X.astype(np.longdouble).sum(0).astype(np.float64)
    out = []
    ra = [values(row[:C], interval, metrics) for row in reps]
    if XB is not None:
        pa, pb = values(point[:C], interval, metrics), values(point[C:], interval, metrics)
        rb = [values(row[C:], interval, metrics) for row in reps]
    for m in metrics:
        width = len(ra[0][m])
        e = [ends([x[m][b] for x in ra], level) for b in range(width)]
        out.append(('%s.%s.lo' % (scenario, m), [x[0] for x in e]))
        out.append(('%s.%s.hi' % (scenario, m), [x[1] for x in e]))
        if XB is not None:
            d = [[x[m][b] - y[m][b] for x, y in zip(ra, rb)] for b in range(width)]
            e = [ends(col, level) for col in d]
            out.append(('%s.vs.%s' % (scenario, m), pb[m]))
            out.append(('%s.diff.%s' % (scenario, m), [x - y for x, y in zip(pa[m], pb[m])]))
            out.append(('%s.diff.%s.lo' % (scenario, m), [x[0] for x in e]))
            out.append(('%s.diff.%s.hi' % (scenario, m), [x[1] for x in e]))
            out.append(('%s.diff.%s.p' % (scenario, m), [p_value(col) for col in d]))
    return out
