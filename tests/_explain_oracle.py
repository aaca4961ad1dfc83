"""NumPy / plain-Python oracle of K19 (tkr_nearest_anchors; csrc/explain.hip), of explain.unexpectedness and of the lines
recommend.py --explain writes.  Not a test module.

sim(a, b) comes through oracle.ref_np.mfma_chain_scores: the library's one fp32 order (a `full` table of every pair, computed once by
the caller, is indexed instead where given).  Per entry the eligible anchor POSITIONS are sorted by (-sim, position) with a stable
sort.  The double rounding mfma_chain_scores' docstring describes can move a similarity by one ulp, so next to the result the smallest
gap between neighbouring similarities among an entry's best e + 1 is kept: an entry is AMBIGUOUS when that gap is <= 2^-20 (K17's
GAP) -- the comparing tests skip such entries where inputs are generic floats, and skip nothing where the arithmetic is exact.
Similarities are finite numbers here (the oracle marks an ineligible pair with -inf)."""
import numpy as np

from oracle import ref_np as R

F32 = np.float32
GAP = 2.0 ** -20


def valid_len(ids_row, n_items):
    """the valid prefix: up to the first id that is negative or >= n_items"""
    bad = np.flatnonzero((np.asarray(ids_row) < 0) | (np.asarray(ids_row) >= n_items))
    return int(bad[0]) if len(bad) else len(ids_row)


def ptr_ok(anchor_ptr, r, n_anchors):
    lo, hi = int(anchor_ptr[r]), int(anchor_ptr[r + 1])
    return 0 <= lo <= hi <= n_anchors and (r != 0 or lo == 0)


def status_word(ids, anchor_ptr, anchor_cols, n_items):
    """-1, or the smallest 4 * row + kind: 0 -- an id >= n_items ends the row; 1 -- an anchor outside [0, n_items); 3 -- a bad anchor_ptr
    (the anchors of such a row are not looked at)"""
    found = []
    for r in range(len(ids)):
        n = valid_len(ids[r], n_items)
        if n < len(ids[r]) and ids[r][n] >= n_items:
            found.append(4 * r)
        if not ptr_ok(anchor_ptr, r, len(anchor_cols)):
            found.append(4 * r + 3)
        else:
            a = np.asarray(anchor_cols[int(anchor_ptr[r]):int(anchor_ptr[r + 1])])
            if np.any((a < 0) | (a >= n_items)):
                found.append(4 * r + 1)
    return min(found) if found else -1


def nearest_row(S, ids_row, anchors, e, n_items, full=None):
    """one row -> (pos int32 [t, e], sim float32 [t, e], gap float64 [t]); anchors: the row's columns, positions from 0"""
    t = len(ids_row)
    pos = np.full((t, e), -1, dtype=np.int32)
    sim = np.full((t, e), -np.inf, dtype=F32)
    gap = np.full(t, np.inf)
    n = valid_len(ids_row, n_items)
    anchors = np.asarray(anchors, dtype=np.int64)
    in_table = np.flatnonzero((anchors >= 0) & (anchors < n_items))
    if n == 0 or len(in_table) == 0:
        return pos, sim, gap
    entries = np.asarray(ids_row[:n], dtype=np.int64)
    cols = anchors[in_table]
    s = full[np.ix_(entries, cols)] if full is not None else R.mfma_chain_scores(S[entries], S[cols])
    s = np.where(cols[None, :] == entries[:, None], -np.inf, s.astype(np.float64))         # an item does not explain itself
    order = np.argsort(-s, axis=1, kind='stable')[:, :e + 1]          # in_table is ascending: ties go to the lower position
    best = np.take_along_axis(s, order, 1)
    have = best > -np.inf
    m = min(e, order.shape[1])
    pos[:n, :m] = np.where(have[:, :m], in_table[order[:, :m]], -1)
    sim[:n, :m] = np.where(have[:, :m], best[:, :m], -np.inf).astype(F32)
    if order.shape[1] >= 2:
        d = np.where(have[:, 1:], best[:, :-1] - np.where(have[:, 1:], best[:, 1:], 0.0), np.inf)
        gap[:n] = d.min(axis=1)
    return pos, sim, gap


def nearest(S, ids, anchor_ptr, anchor_cols, e, n_items, full=None):
    """every row -> (pos int32 [n, t, e], sim float32 [n, t, e], ambiguous bool [n, t]); a row whose anchor_ptr is refused gets padding"""
    n, t = ids.shape
    pos = np.full((n, t, e), -1, dtype=np.int32)
    sim = np.full((n, t, e), -np.inf, dtype=F32)
    amb = np.zeros((n, t), dtype=bool)
    for r in range(n):
        if ptr_ok(anchor_ptr, r, len(anchor_cols)):
            pos[r], sim[r], gap = nearest_row(S, ids[r], anchor_cols[int(anchor_ptr[r]):int(anchor_ptr[r + 1])], e, n_items, full)
            amb[r] = gap <= GAP
    return pos, sim, amb


def columns(pos, anchor_ptr, anchor_cols):
    """positions -> anchor columns, -1 padded (what explain.explain's gather does)"""
    out = np.full(pos.shape, -1, dtype=np.int32)
    for r in range(len(pos)):
        at = pos[r] >= 0
        out[r][at] = np.asarray(anchor_cols)[int(anchor_ptr[r]) + pos[r][at]]
    return out


def unexpectedness_loop(sims0, ids, grid):
    """explain.unexpectedness as loops over lines and entries, float64"""
    out = []
    for K in grid:
        K = min(K, ids.shape[1])
        per_line = []
        for r in range(len(ids)):
            n = min(K, valid_len(ids[r], 1 << 62))
            vals = [1.0 - float(sims0[r, p]) for p in range(n) if np.isfinite(sims0[r, p])]
            if vals:
                per_line.append(sum(vals) / len(vals))
        out.append(sum(per_line) / len(per_line) if per_line else 0.0)
    return out


def explain_lines(users, ids, cols, sims, tokens):
    """the lines of recommend.py --explain-output: 'uid,iid:aid:%f:aid:%f,iid,...' -> (lines, per line the fields as
    (item token, [(anchor token, '%f' text), ...]))"""
    lines, fields = [], []
    for u, row_i, row_c, row_s in zip(users, ids, cols, sims):
        row = []
        for c, anchors, values in zip(row_i, row_c, row_s):
            if c >= 0:
                row.append((tokens[int(c)], [(tokens[int(a)], '%f' % float(s)) for a, s in zip(anchors, values) if a >= 0]))
        fields.append(row)
        lines.append(','.join([u] + [i + ''.join(':%s:%s' % pair for pair in why) for i, why in row]))
    return lines, fields
