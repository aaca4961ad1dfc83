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


# ---- evaluation against sampled negatives (evaluate.py --negatives; ranks from K12, tkr_hip.rank_candidates) -------------------------
# Every ranked like gets a row of its own: the like plus N columns drawn without replacement from those the user neither rated in
# training nor has anywhere on the test line.  With r the like's rank inside its row:
#   hr@K = mean [r < K],  ndcg@K = mean [r < K] / log2(r + 2)   (one relevant entry per row: the ideal DCG is 1),  mrr = mean 1 / (r + 1)
NEG_METRICS = ('hr', 'ndcg', 'mrr')


def _distinct_below(rng, M, n_draw):
    """for every row i, min(n_draw, M[i]) distinct integers of [0, M[i]), every subset equally likely -> (ptr int64, flat int64 values,
    ascending inside a row).  Rows with M >= 2 n_draw: n_draw draws, duplicates drawn again until none is left (symmetric in the values,
    at most every second draw is lost); the others: the first entries of a random order of [0, M)."""
    M = np.asarray(M, dtype=np.int64)
    R = len(M)
    take = np.minimum(M, n_draw)
    ptr = np.zeros(R + 1, dtype=np.int64)
    np.cumsum(take, out=ptr[1:])
    out = np.zeros(int(ptr[-1]), dtype=np.int64)
    if n_draw <= 0 or R == 0:
        return ptr, out
    sparse = np.flatnonzero(M >= 2 * n_draw)
    if len(sparse):
        high = M[sparse][:, None]
        draws = np.sort(rng.integers(0, high, size=(len(sparse), n_draw)), axis=1)
        while True:
            dup = np.zeros(draws.shape, dtype=bool)
            dup[:, 1:] = draws[:, 1:] == draws[:, :-1]
            if not dup.any():
                break
            rows = np.nonzero(dup)[0]
            draws[dup] = rng.integers(0, M[sparse][rows])
            draws.sort(axis=1)
        at = (ptr[sparse][:, None] + np.arange(n_draw, dtype=np.int64)[None, :]).reshape(-1)
        out[at] = draws.reshape(-1)
    dense = np.flatnonzero((M < 2 * n_draw) & (M > 0))
    if len(dense):
        W = int(M[dense].max())
        keys = rng.random((len(dense), W))
        keys[np.arange(W)[None, :] >= M[dense][:, None]] = np.inf
        order = np.argsort(keys, axis=1, kind='stable')[:, :min(n_draw, W)]
        valid = np.arange(order.shape[1])[None, :] < take[dense][:, None]
        picked = np.where(valid, order, np.iinfo(np.int64).max)
        picked.sort(axis=1)
        out[(ptr[dense][:, None] + np.arange(order.shape[1], dtype=np.int64)[None, :])[valid]] = picked[valid]
    return ptr, out


def sample_negatives(like_ptr, like_cols, excluded_ptr, excluded_cols, n_cols, N, seed):
    """The candidate rows of the sampled-negatives protocol, drawn on numpy.random.Generator(PCG64(seed)): the same seed gives the same rows.

    like_ptr [n_lines + 1] / like_cols: the likes of every test line that get a row (the caller leaves train-rated likes out);
    excluded_ptr / excluded_cols: per line, ascending and unique, every column that must not be drawn -- the user's train-rated columns
    and every column on the test line, the likes included.  Row q (like q of the CSR, line by line) holds its like and min(N, eligible)
    distinct columns drawn uniformly without replacement from the n_cols - |excluded| eligible ones of its line.
    -> (cand_ptr int64 [n_likes + 1], cand_cols int32 ascending inside a row, like_at int64 [n_likes]: where the like sits in cand_cols)"""
    like_ptr, excluded_ptr = np.asarray(like_ptr, dtype=np.int64), np.asarray(excluded_ptr, dtype=np.int64)
    like_cols, excluded_cols = np.asarray(like_cols, dtype=np.int64), np.asarray(excluded_cols, dtype=np.int64)
    n_lines, Q = len(like_ptr) - 1, len(like_cols)
    rng = np.random.Generator(np.random.PCG64(seed))
    line = np.repeat(np.arange(n_lines, dtype=np.int64), np.diff(like_ptr))
    M = (n_cols - np.diff(excluded_ptr))[line]
    dptr, idx = _distinct_below(rng, M, int(N))
    # the idx-th eligible column of a line: idx + #{j : x_j - j <= idx} over the line's excluded columns x_0 < x_1 < ...
    ex_line = np.repeat(np.arange(n_lines, dtype=np.int64), np.diff(excluded_ptr))
    gap = excluded_cols - (np.arange(len(excluded_cols), dtype=np.int64) - excluded_ptr[ex_line])
    stride = np.int64(n_cols + 1)
    row = np.repeat(np.arange(Q, dtype=np.int64), np.diff(dptr))
    skipped = np.searchsorted(ex_line * stride + gap, line[row] * stride + idx, side='right') - excluded_ptr[line[row]]
    neg = idx + skipped
    rows = np.concatenate([row, np.arange(Q, dtype=np.int64)])
    cols = np.concatenate([neg, like_cols])
    order = np.lexsort((cols, rows))
    cand_ptr = np.zeros(Q + 1, dtype=np.int64)
    np.cumsum(np.bincount(rows, minlength=Q), out=cand_ptr[1:])
    like_at = np.empty(Q, dtype=np.int64)
    is_like = order >= len(neg)
    like_at[rows[order][is_like]] = np.flatnonzero(is_like)
    return cand_ptr, cols[order].astype(np.int32), like_at


def negative_sums(like_ranks, step, total):
    """like_ranks int [n_rows]: the rank of every row's like among its candidates -> {metric: (fp64 sum(s), n_rows)} like rank_sums"""
    r = np.asarray(like_ranks, dtype=np.int64)
    interval = total // step
    grid = step * np.arange(1, interval + 1, dtype=np.int64)
    gain = 1.0 / np.log2(r + 2.0)
    hr = np.array([np.count_nonzero(r < K) for K in grid], dtype=np.float64)
    ndcg = np.array([np.sum(gain[r < K]) for K in grid], dtype=np.float64)
    return {'hr': (hr, len(r)), 'ndcg': (ndcg, len(r)), 'mrr': (float(np.sum(1.0 / (r + 1.0))), len(r))}


def neg_to_vector(sums):
    return np.concatenate([np.r_[np.asarray(sums[m][0], dtype=np.float64).reshape(-1), float(sums[m][1])] for m in NEG_METRICS])


def neg_from_vector(vec, interval):
    out, at = {}, 0
    for m in NEG_METRICS:
        width = 1 if m == 'mrr' else interval
        s, count = np.asarray(vec[at:at + width], dtype=np.float64), int(round(float(vec[at + width])))
        out[m] = (float(s[0]) if m == 'mrr' else s.copy(), count)
        at += width + 1
    return out
