"""NumPy oracle of K17 (tkr_mmr_select, tkr_list_pair_sums; csrc/diversity.hip) and of diversity.metrics_from_pair_sums.  Not a test module.

sim(a, b) comes through oracle.ref_np.mfma_chain_scores(S[c], S[c]): the library's one fp32 order.  The greedy loop works on float32
values; the fused multiply-add  obj = fma(-mu, pen, a)  is float32(float64(a) - float64(mu) * float64(pen)) -- the product is exact in
float64, the difference is rounded to 53 and then to 24 bits, which differs from one rounding only on a float32 tie of the float64
value (the one-ulp double rounding mfma_chain_scores' docstring describes).  At every pick the gap between the best and the second-best
objective is recorded: a row is AMBIGUOUS when any gap is <= 2^-20 (16 ulp at 1.0, far above that one ulp) -- the comparing tests skip
such rows where inputs are generic floats, and skip nothing where the arithmetic is exact."""
import numpy as np

from oracle import ref_np as R

F32 = np.float32
GAP = 2.0 ** -20


def valid_len(ids_row, n_items):
    """the valid prefix: up to the first id that is negative or >= n_items"""
    bad = np.flatnonzero((np.asarray(ids_row) < 0) | (np.asarray(ids_row) >= n_items))
    return int(bad[0]) if len(bad) else len(ids_row)


def sims(S, cols, full=None):
    """float32 [n, n]: the chain of every pair of the rows `cols` of S; full: sims(S, every row), computed once by the caller"""
    if full is not None:
        return full[np.ix_(cols, cols)]
    return R.mfma_chain_scores(S[cols], S[cols])


def mmr_row(S, ids_row, rel_row, lam, t, n_items, full=None):
    """-> (sel_pos int32 [t], -1 padded; the smallest gap between the best and the second-best objective over the picks)"""
    n = valid_len(ids_row, n_items)
    sel = np.full(t, -1, dtype=np.int32)
    if n == 0:
        return sel, np.inf
    sim = sims(S, np.asarray(ids_row[:n], dtype=np.int64), full)
    lam32 = F32(lam)
    mu32 = F32(F32(1.0) - lam32)
    a = (lam32 * np.asarray(rel_row[:n], dtype=F32)).astype(F32)
    pen = np.full(n, -np.inf, dtype=F32)
    free = np.ones(n, dtype=bool)
    gap = np.inf
    for r in range(min(t, n)):
        if r == 0:
            obj = a.copy()
        else:
            obj = (a.astype(np.float64) - np.float64(mu32) * pen.astype(np.float64)).astype(F32)
        obj = np.where(free, obj, -np.inf)
        p = int(np.argmax(obj))                                       # the first maximum: ties go to the lower pool position
        if free.sum() > 1:
            rest = obj.copy()
            rest[p] = -np.inf
            gap = min(gap, float(np.float64(obj[p]) - np.float64(rest[free & (np.arange(n) != p)].max())))
        sel[r] = p
        free[p] = False
        pen = np.maximum(pen, sim[:, p])
    return sel, gap


def mmr(S, ids, rel, lam, t, n_items, full=None):
    """every row -> (sel_pos int32 [n_rows, t], ambiguous bool [n_rows])"""
    out = np.full((len(ids), t), -1, dtype=np.int32)
    amb = np.zeros(len(ids), dtype=bool)
    for r in range(len(ids)):
        out[r], gap = mmr_row(S, ids[r], rel[r], lam, t, n_items, full)
        amb[r] = gap <= GAP
    return out, amb


def pair_sums(S, ids, n_items, full=None):
    """float64 [n_rows, t]: sum over a < b of 1 - sim(a, b) inside the valid prefix, 0 behind it"""
    out = np.zeros(ids.shape, dtype=np.float64)
    for r in range(len(ids)):
        n = valid_len(ids[r], n_items)
        if n:
            d = 1.0 - sims(S, ids[r, :n].astype(np.int64), full).astype(np.float64)
            for b in range(n):
                out[r, b] = d[:b, b].sum()
    return out


def gini_loop(counts):
    x = sorted(float(c) for c in counts)
    n, total = len(x), sum(x)
    if n == 0 or total == 0:
        return 0.0
    return sum((2 * (i + 1) - n - 1) * v for i, v in enumerate(x)) / (n * total)


def metrics_loop(pair_sum, ids, n_cols, grid):
    """diversity.metrics_from_pair_sums as loops over rows and entries"""
    out = {'ild': [], 'cov': [], 'gini': []}
    for K in grid:
        K = min(K, ids.shape[1])
        per_row, counts = [], [0] * n_cols
        for r in range(len(ids)):
            n = valid_len(ids[r], 1 << 62)
            m = min(K, n)
            for c in ids[r, :m]:
                counts[int(c)] += 1
            if m >= 2:
                per_row.append(sum(float(pair_sum[r, b]) for b in range(m)) / (m * (m - 1) / 2))
        out['ild'].append(sum(per_row) / len(per_row) if per_row else 0.0)
        out['cov'].append(sum(1 for c in counts if c) / n_cols)
        out['gini'].append(gini_loop(counts))
    return out
