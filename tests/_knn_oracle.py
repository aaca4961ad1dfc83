"""NumPy restatement of K28 and K29 (include/tkr.h tkr_knn_build / tkr_knn_score), bit for bit: the oracle of tests/test_gpu_knn.py and
tests/test_gpu_knn_wide.py.

  C = X^T X in int64; sim = fp32(C / (fl64(norm_i norm_j) + shrink)), every operation rounded on its own; the canonical order is a
  stable argsort read backwards (score descending, ties -> the higher column first); a score is the ascending fp32 chain over the
  history; ranks by counting.
"""
import numpy as np


def csr(rows, n_rows):
    """a list of index sequences -> (ptr int64, cols int32), every row ascending and unique"""
    rows = [sorted(set(int(c) for c in r)) for r in rows]
    assert len(rows) == n_rows
    ptr = np.zeros(n_rows + 1, np.int64)
    np.cumsum([len(r) for r in rows], out=ptr[1:])
    return ptr, np.asarray([c for r in rows for c in r], np.int32)


def transpose(ptr, cols, n_cols):
    """the CSR of the transpose, rows ascending"""
    n_rows = len(ptr) - 1
    row = np.repeat(np.arange(n_rows, dtype=np.int64), np.diff(ptr))
    order = np.argsort(cols.astype(np.int64) * n_rows + row, kind='stable')
    tptr = np.zeros(n_cols + 1, np.int64)
    np.cumsum(np.bincount(cols, minlength=n_cols), out=tptr[1:])
    return tptr, row[order].astype(np.int32)


def dense(ptr, cols, n_cols):
    X = np.zeros((len(ptr) - 1, n_cols), np.int64)
    X[np.repeat(np.arange(len(ptr) - 1), np.diff(ptr)), cols] = 1
    return X


def norms(n_likers, similarity):
    n = np.asarray(n_likers, np.float64)
    return np.sqrt(np.maximum(n, 1.0)) if similarity == 'cosine' else np.ones_like(n)


def similarities(C, norm, shrink):
    """fp32 [n_items, n_items]: the formula on every pair (the caller looks at the candidates only)"""
    with np.errstate(divide='ignore'):
        den = norm[:, None] * norm[None, :]            # rounded
        den = den + np.float64(shrink)                 # rounded
        return (C.astype(np.float64) / den).astype(np.float32)


def canonical(scores):
    """the columns by score descending, ties -> the higher column first: a stable argsort read backwards"""
    return np.argsort(scores, kind='stable')[::-1]


def build(u_ptr, u_cols, n_items, norm, shrink, N):
    """-> (nbr_ids int32 [n_items, N], nbr_w fp32 [n_items, N], C int64, sim fp32)"""
    X = dense(u_ptr, u_cols, n_items)
    C = X.T @ X
    sim = similarities(C, np.asarray(norm, np.float64), shrink)
    ids = np.full((n_items, N), -1, np.int32)
    w = np.zeros((n_items, N), np.float32)
    for i in range(n_items):
        order = canonical(sim[i])
        order = order[(order != i) & (C[i, order] > 0)][:N]
        ids[i, :len(order)] = order
        w[i, :len(order)] = sim[i, order]
    return ids, w, C, sim


def build_compact(u_ptr, u_cols, n_items, norm, shrink, N):
    """build() without the n_items x n_items matrix -> (nbr_ids, nbr_w): the liked columns are mapped to 0 .. m - 1 in ascending order (a
    monotone map keeps the canonical tie order), build() runs on the compacted CSR with norm[liked], the ids are mapped back, and the row
    of an item nobody likes is -1 / +0.0"""
    liked = np.flatnonzero(np.bincount(u_cols, minlength=n_items))
    to_compact = np.full(n_items, -1, np.int32)
    to_compact[liked] = np.arange(len(liked), dtype=np.int32)
    ids = np.full((n_items, N), -1, np.int32)
    w = np.zeros((n_items, N), np.float32)
    if len(liked):
        cids, cw = build(u_ptr, to_compact[u_cols], len(liked), np.asarray(norm, np.float64)[liked], shrink, N)[:2]
        ids[liked] = np.where(cids >= 0, liked[np.maximum(cids, 0)], -1)
        w[liked] = cw
    return ids, w


def scores(hist_ptr, hist_cols, nbr_ids, nbr_w, col_of_item, n_cols):
    """fp32 [n_rows, n_cols]: acc = fl(acc + w) from +0.0 over the history items in ascending order"""
    n_rows = len(hist_ptr) - 1
    s = np.zeros((n_rows, n_cols), np.float32)
    for r in range(n_rows):
        for i in hist_cols[hist_ptr[r]:hist_ptr[r + 1]]:
            for j, wt in zip(nbr_ids[i], nbr_w[i]):
                if j < 0:
                    continue
                c = j if col_of_item is None else col_of_item[j]
                if c >= 0:
                    s[r, c] = np.float32(s[r, c] + wt)
    return s


def scores_by_item(hist_ptr, hist_cols, nbr_ids, nbr_w, col_of_item, n_cols):
    """scores() with one NumPy statement per history item: the ids of a neighbour list are distinct and so are the columns they map to, so
    s[r, cols] = fl(s[r, cols] + w) is the same chain on every column (tests/test_knn_cpu.py holds it to scores() bit for bit)"""
    n_rows = len(hist_ptr) - 1
    s = np.zeros((n_rows, n_cols), np.float32)
    for r in range(n_rows):
        for i in hist_cols[hist_ptr[r]:hist_ptr[r + 1]]:
            ids, wt = nbr_ids[i], nbr_w[i]
            ok = ids >= 0
            cols = ids[ok] if col_of_item is None else col_of_item[ids[ok]]
            wt = wt[ok]
            s[r, cols[cols >= 0]] += wt[cols >= 0]                 # fp32 + fp32, rounded once; no column twice
    return s


def masked_columns(rated_ptr, rated_cols, n_rows, n_cols):
    m = np.zeros((n_rows, n_cols), bool)
    if rated_ptr is not None:
        m[np.repeat(np.arange(n_rows), np.diff(rated_ptr)), rated_cols] = True
    return m


def topk(s, masked, K):
    """-> (ids int32 [n_rows, K] padded -1, scores fp32 padded -inf)"""
    n_rows = s.shape[0]
    ids = np.full((n_rows, K), -1, np.int32)
    out = np.full((n_rows, K), -np.inf, np.float32)
    for r in range(n_rows):
        order = canonical(s[r])
        order = order[~masked[r, order]][:K]
        ids[r, :len(order)] = order
        out[r, :len(order)] = s[r, order]
    return ids, out


def ranks(s, masked, like_ptr, like_cols):
    """int32 [n_likes]: -1 for a masked or out-of-range like, else the number of kept columns in front of it"""
    n_cols = s.shape[1]
    out = np.full(len(like_cols), -1, np.int32)
    for r in range(len(like_ptr) - 1):
        kept = ~masked[r]
        cols = np.arange(n_cols)
        for e in range(like_ptr[r], like_ptr[r + 1]):
            l = like_cols[e]
            if not 0 <= l < n_cols or masked[r, l]:
                continue
            out[e] = int(np.sum(kept & ((s[r] > s[r, l]) | ((s[r] == s[r, l]) & (cols > l)))))
    return out
