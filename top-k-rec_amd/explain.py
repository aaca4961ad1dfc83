"""explain.py -- say why an item is on a list, and how far a list strays from what its user already has: for every entry of a top-k
list the user's own liked items whose factors are closest to it (K19, tkr_hip.nearest_anchors), and unexpectedness, 1 - the
similarity of an entry to the nearest item of the user's history, averaged over a list and then over the lists.

torch and numpy are plumbing here (grouping the likes into rows, a gather, two cumulative sums, the text of the lines); the
similarities and the ranking of the anchors run in csrc/explain.hip.

    S = diversity.similarity_table(V_dev, 'cosine')
    aptr, acols = anchors_csr([R], user_rows, n_items, device)            # the like == 1 items of every row's user
    cols, sims = explain(S, ids, aptr, acols, e=3)                          # int32 / fp32 [n, t, e], -1 / -inf padded
    u = unexpectedness(sims[:, :, 0], ids, [5, 10, 30])
"""
from __future__ import annotations

import numpy as np
import torch

import diversity
import textio
import tkr_hip

METRICS = ('unexp',)


def add_arguments(parser):
    """--explain / --explain-output of recommend.py (--similarity is diversity.add_arguments')"""
    parser.add_argument('--explain', type=int, default=None, metavar='E',
                        help="Explain every recommended item by the E (1 ... %d) liked items of its user that are most similar to it; "
                             "needs --explain-output" % tkr_hip.ANCHOR_MAX_E)
    parser.add_argument('--explain-output', default=None, metavar='FILE',
                        help="With --explain: the file that gets one line 'uid,iid:aid:%%f:aid:%%f,iid:...' per output line")


def check_arguments(parser, args):
    """the arguments of add_arguments -> the keyword arguments of recommend.rank they stand for ({} without --explain); parser.error
    on what cannot be served"""
    if (args.explain is None) != (args.explain_output is None):
        parser.error('--explain and --explain-output go together')
    if args.explain is None:
        return {}
    if not 1 <= args.explain <= tkr_hip.ANCHOR_MAX_E:
        parser.error('--explain takes a number of anchors in 1 ... %d' % tkr_hip.ANCHOR_MAX_E)
    return dict(explain=args.explain, similarity=args.similarity or 'cosine')


def _liked_pairs(R, user_rows, n_users):
    """(row, item) of every known like == 1 entry on the LAST line of each row's user in the parsed ratings file R (numpy)"""
    known = np.flatnonzero((R.line_user >= 0) & (R.line_user < n_users))
    last = np.full(max(n_users, 1), -1, dtype=np.int64)
    np.maximum.at(last, R.line_user[known], known)
    hl = last[user_rows] if len(user_rows) else np.zeros(0, dtype=np.int64)
    rows = np.flatnonzero(hl >= 0)
    seg = R.line_ptr[hl[rows] + 1] - R.line_ptr[hl[rows]]
    row = np.repeat(rows, seg)
    at = np.arange(int(seg.sum()), dtype=np.int64) - np.repeat(np.cumsum(seg) - seg, seg) + np.repeat(R.line_ptr[hl[rows]], seg)
    keep = (R.item[at] >= 0) & (R.like[at] == 1)
    return row[keep], R.item[at][keep].astype(np.int64)


def anchors_csr(sources, user_rows, n_items, device, where=None):
    """the anchors of every ranked row: the like == 1 items on the last line of its user in each of the parsed ratings files `sources`
    (one or two, in one user and item numbering), ascending and without repeats -> (ptr int64 [n + 1], cols int32) on `device`.
    where / TKR_GROUP: K15 (tkr_hip.group_segments, like_only) or numpy, the same arrays (textio.group_on_device)"""
    where = textio._group_where(where)
    user_rows = np.asarray(user_rows, dtype=np.int64)
    n, n_cols = len(user_rows), max(int(n_items), 1)
    n_users = int(user_rows.max()) + 1 if n else 0
    if n and textio.group_on_device(where, sum(textio.n_entries_of(R) for R in sources), n_cols):
        try:
            rows = torch.from_numpy(user_rows).to(device)
            segs = []
            for R in sources:
                Rd = textio.ratings_to_device(R, device)
                last = tkr_hip.last_line_of_user(Rd.line_user, n_users)
                segs.append((Rd.line_ptr, Rd.item, Rd.like, last[rows].contiguous()))
            textio.group_fits(4 * sum(int(s[1].numel()) for s in segs) + 8 * n + 64, device, 'the anchors')
            return tkr_hip.group_segments(segs, n, n_cols, like_only=True)
        except textio.DeviceGroupTooLarge:
            if where == 'device':
                raise
    pairs = [_liked_pairs(textio.ratings_to_host(R), user_rows, n_users) for R in sources]
    key = np.unique(np.concatenate([p[0] for p in pairs]) * n_cols + np.concatenate([p[1] for p in pairs]))
    ptr = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(np.bincount(key // n_cols, minlength=n), out=ptr[1:])
    return torch.from_numpy(ptr).to(device), torch.from_numpy((key % n_cols).astype(np.int32)).to(device)


def explain(S, ids, anchor_ptr, anchor_cols, e):
    """-> (cols int32 [n, t, e], sims fp32 [n, t, e]) on the device: for every entry of the lists `ids` the e anchors of its row that
    are most similar to it in S and are not the entry itself, as COLUMNS (K19 ranks positions; a gather turns them into columns), best
    first, with their similarities; -1 / -inf where a row has fewer, and behind a list's end"""
    ids = ids.contiguous()
    pos, sims = tkr_hip.nearest_anchors(S, ids, anchor_ptr, anchor_cols, e)
    n_anchors = int(anchor_cols.numel())
    if int(ids.shape[0]) == 0 or n_anchors == 0:
        return torch.full_like(pos, -1), sims
    at = (anchor_ptr[:-1].reshape(-1, 1, 1) + pos.clamp(min=0).long()).clamp(max=n_anchors - 1)
    return torch.where(pos < 0, torch.full_like(pos, -1), anchor_cols[at]), sims


def unexpectedness(sims0, ids, grid):
    """unexpectedness at every cut-off K of `grid` from the similarity of every entry to its nearest anchor (sims0 fp32 [n, t]: explain's
    sims[:, :, 0]) and the lists (int [n, t], -1 padded); any device, float64 -> [float per K].  An entry is EXPLAINED when it lies in
    the valid prefix and its similarity is finite (-inf: no eligible anchor); its value is 1 - sim.  A line's value at K is the mean over
    its explained entries among the first K; the figure is the mean over the lines that have one, 0.0 when there is no such line"""
    explained = diversity.valid_prefix(ids) & torch.isfinite(sims0)
    value = torch.where(explained, 1.0 - sims0.to(torch.float64), torch.zeros_like(sims0, dtype=torch.float64))
    total, count = torch.cumsum(value, dim=1), torch.cumsum(explained.to(torch.int64), dim=1)
    out = []
    for K in grid:
        K = min(int(K), int(ids.shape[1]))
        lines = count[:, K - 1] > 0 if K >= 1 else None
        if K >= 1 and bool(lines.any()):
            out.append(float((total[:, K - 1][lines] / count[:, K - 1][lines].to(torch.float64)).mean()))
        else:
            out.append(0.0)
    return out


def list_unexpectedness(S, ids, anchor_ptr, anchor_cols, grid):
    """unexpectedness of the lists `ids` (int32 [n, t] on the device, -1 padded) against the anchors -> [float per cut-off of grid]"""
    if int(ids.shape[0]) == 0:
        return [0.0] * len(grid)
    _, sims = explain(S, ids, anchor_ptr, anchor_cols, 1)
    return unexpectedness(sims[:, :, 0], ids, grid)


def format_lines(users, ids, cols, sims, items):
    """users: n tokens; ids int [n, t] catalogue indices, -1 = no item; cols int [n, t, e], -1 = no anchor; sims float [n, t, e]; items:
    index -> token -> n lines 'uid,iid:aid:%f:aid:%f,iid,...': a field per item in list order, its anchors best first"""
    out = []
    for u, row_i, row_c, row_s in zip(users, np.asarray(ids), np.asarray(cols), np.asarray(sims)):
        fields = [u]
        for c, anchors, values in zip(row_i, row_c, row_s):
            if c >= 0:
                fields.append(items[int(c)] + ''.join(':%s:%f' % (items[int(a)], float(s)) for a, s in zip(anchors, values) if a >= 0))
        out.append(','.join(fields))
    return out


def write_lines(path, users: textio.IdMap, ids, cols, sims, row_user, items: textio.IdMap, append=False):
    """write (or append) the lines of format_lines for the rows of ids / cols / sims; row r is the list of user index row_user[r]"""
    host = lambda x, dtype: np.ascontiguousarray(x.detach().cpu().numpy() if isinstance(x, torch.Tensor) else x, dtype=dtype)
    utok, itok = users.tokens_by_index(), items.tokens_by_index()
    lines = format_lines([utok[int(u)] for u in host(row_user, np.int64).reshape(-1)], host(ids, np.int64), host(cols, np.int64),
                         host(sims, np.float32), itok)
    with open(path, 'ab' if append else 'wb') as fh:
        fh.write(('\n'.join(lines) + '\n').encode() if lines else b'')
