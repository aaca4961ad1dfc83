"""What K15 (tkr_hip.group_segments and its two helpers) must produce, restated in plain Python: sorted(set(...)) per row.  Independent
of evaluate._group (numpy keys) and of the kernels (bitmaps)."""
import numpy as np


def csr(rows):
    """list of ascending lists -> (ptr int64 [n + 1], cols int32)"""
    ptr = np.zeros(len(rows) + 1, dtype=np.int64)
    for r, row in enumerate(rows):
        ptr[r + 1] = ptr[r] + len(row)
    return ptr, np.array([c for row in rows for c in row], dtype=np.int32)


def segment_items(seg_ptr, item, like, g, like_only):
    return {int(item[e]) for e in range(int(seg_ptr[g]), int(seg_ptr[g + 1])) if item[e] >= 0 and (not like_only or like[e] == 1)}


def group_segments(sources, n_rows, like_only=False):
    """sources: tuples (seg_ptr, item, like | None, seg_of_row | None) of host arrays -> (ptr, cols)"""
    rows = []
    for r in range(n_rows):
        found = set()
        for seg_ptr, item, like, seg_of_row in sources:
            g = r if seg_of_row is None else int(seg_of_row[r])
            if g >= 0:
                found |= segment_items(seg_ptr, item, like, g, like_only)
        rows.append(sorted(found))
    return csr(rows)


def last_line_of_user(line_user, n_users):
    last = [-1] * n_users
    for line, u in enumerate(line_user):
        if 0 <= u < n_users:
            last[int(u)] = line
    return np.array(last, dtype=np.int64).reshape(n_users)


def scenario_lines(ptr):
    rows = [r for r in range(len(ptr) - 1) if ptr[r + 1] > ptr[r]]
    out = np.array([ptr[r] for r in rows] + [ptr[-1]], dtype=np.int64)
    return np.array(rows, dtype=np.int64), out


def scenario(T, H):
    """the seven arrays of evaluate.load_scenario from the parsed test file T and train file H (textio.Ratings), the reference's way:
    a dict of the last train line per user, a set per line -> (users, like_ptr, like_cols, rated_ptr, rated_cols, seen_ptr, seen_cols)"""
    users, likes, seen = [], [], []
    for line in range(len(T.line_user)):
        mine = segment_items(T.line_ptr, T.item, T.like, line, True)
        if mine:
            users.append(int(T.line_user[line]))
            likes.append(sorted(mine))
            seen.append(sorted(segment_items(T.line_ptr, T.item, T.like, line, False)))
    last = {}
    for line, u in enumerate(H.line_user):
        if u >= 0:
            last[int(u)] = line
    rated = [sorted(segment_items(H.line_ptr, H.item, H.like, last[u], False)) for u in users]
    return (np.array(users, dtype=np.int64).reshape(len(users)),) + csr(likes) + csr(rated) + csr(seen)


def random_source(rng, n_seg, n_cols, lengths=None, unknown=0.1):
    """a source of n_seg segments: items in [-1, n_cols) with repeats, likes in {-1, 0, 1, 2}"""
    if lengths is None:
        lengths = rng.integers(0, 40, n_seg)
    seg_ptr = np.zeros(n_seg + 1, dtype=np.int64)
    np.cumsum(lengths, out=seg_ptr[1:])
    n = int(seg_ptr[-1])
    item = rng.integers(0, n_cols, n).astype(np.int32)
    item[rng.random(n) < unknown] = -1
    like = rng.integers(-1, 3, n).astype(np.int32)
    return seg_ptr, item, like
