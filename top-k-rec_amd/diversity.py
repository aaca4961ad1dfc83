"""diversity.py -- look at a top-k list as a whole: re-rank a pool by greedy Maximal Marginal Relevance (K17, tkr_hip.mmr_select) and
measure intra-list diversity, catalogue coverage and the Gini index of item exposure (tkr_hip.list_pair_sums + torch).

torch is plumbing here (normalising, gathering, counting); the similarities and the greedy selection run in csrc/diversity.hip.

    S, rel = prepare(V_dev, pool_ids, pool_scores, 'cosine')
    ids, scores = rerank(S, rel, pool_ids, pool_scores, lam=0.7, t=30)
    m = list_metrics(S, ids, n_cols, [5, 10, 30])          # {'ild': [...], 'cov': [...], 'gini': [...]}
"""
from __future__ import annotations

import torch

import tkr_hip

SIMILARITIES = ('cosine', 'dot')
LIST_METRICS = ('ild', 'cov', 'gini')
DEFAULT_POOL = 100


def default_pool(total):
    return max(DEFAULT_POOL, total)


def valid_prefix(ids):
    """bool [n, N]: the entries of every row in front of its first negative id (the padding rule of K4's lists)"""
    return torch.cumprod((ids >= 0).to(torch.int32), dim=1).bool()


def add_arguments(parser):
    """--diversify / --pool / --similarity, the same on recommend.py and evaluate.py"""
    parser.add_argument('--diversify', type=float, default=None, metavar='LAMBDA',
                        help="Re-rank every list by greedy MMR: LAMBDA in [0, 1] weighs relevance against similarity to the items already "
                             "picked (1: no change).  The scores written are the model's own and no longer monotone along a line")
    parser.add_argument('--pool', type=int, default=None, help="With --diversify: the best items of a list that are re-ranked (default max(100, -t); at most 1024)")
    parser.add_argument('--similarity', default=None, choices=SIMILARITIES, help="With --diversify (and recommend.py --explain): similarity of two items' factors (default cosine)")


def check_arguments(parser, args):
    """the arguments of add_arguments -> the keyword arguments of recommend.rank they stand for ({} without --diversify); parser.error
    on what cannot be served"""
    if args.diversify is None:
        if args.pool is not None or (args.similarity is not None and getattr(args, 'explain', None) is None):     # (--explain: recommend.py's)
            parser.error('--pool and --similarity need --diversify')
        return {}
    if not 0.0 <= args.diversify <= 1.0:                             # (a NaN fails both comparisons)
        parser.error('--diversify takes a lambda in [0, 1]')
    pool = default_pool(args.total) if args.pool is None else args.pool
    if pool < args.total:
        parser.error('--pool must be at least -t')
    if pool > tkr_hip.MMR_MAX_POOL:
        parser.error('--pool can be at most %d' % tkr_hip.MMR_MAX_POOL)
    return dict(diversify=args.diversify, pool=pool, similarity=args.similarity or 'cosine')


def similarity_table(V_dev, similarity='cosine'):
    """-> S fp32 [n_items, k], the table similarity is measured in: 'cosine' -- V scaled by its inverse row norm, a zero row stays zero;
    'dot' -- V itself"""
    if similarity not in SIMILARITIES:
        raise ValueError('similarity must be one of %s, not %r' % (', '.join(SIMILARITIES), similarity))
    V = V_dev.to(torch.float32).contiguous()
    if similarity == 'dot':
        return V
    norm = torch.linalg.vector_norm(V, dim=1, keepdim=True)
    return (V * torch.where(norm > 0, 1.0 / norm, torch.zeros_like(norm))).contiguous()


def relevance(ids, scores):
    """-> rel fp32 [n, N]: the per-row min-max of the valid scores onto [0, 1]: all 0 where they are all equal or there is a single
    entry, 0 in the padding"""
    valid = valid_prefix(ids)
    s = scores.to(torch.float32)
    lo = torch.where(valid, s, torch.full_like(s, float('inf'))).amin(dim=1, keepdim=True)
    hi = torch.where(valid, s, torch.full_like(s, float('-inf'))).amax(dim=1, keepdim=True)
    span = hi - lo
    ok = valid & (span > 0)
    rel = torch.where(ok, (s - lo) / torch.where(span > 0, span, torch.ones_like(span)), torch.zeros_like(s))
    return rel.contiguous()


def prepare(V_dev, ids, scores, similarity='cosine'):
    """-> (S, rel) = (similarity_table, relevance): exactly what `rerank` consumes"""
    return similarity_table(V_dev, similarity), relevance(ids, scores)


def rerank(S, rel, ids, scores, lam, t):
    """-> (ids int32 [n, t], scores fp32 [n, t]): the pool entries K17 picks, in pick order, with the model's own scores; -1 / -inf
    where a row has fewer than t valid entries.  lam = 1 is the identity on a pool sorted by score: the first t entries."""
    ids = ids.contiguous()
    n = int(ids.shape[0])
    if n == 0:
        return ids[:, :t].contiguous(), scores[:, :t].contiguous()
    sel = tkr_hip.mmr_select(S, ids, rel, lam, t)
    at = sel.clamp(min=0).long()
    pad = sel < 0
    out_ids = torch.where(pad, torch.full_like(sel, -1), torch.gather(ids, 1, at))
    out_scores = torch.gather(scores, 1, at).masked_fill(pad, float('-inf'))
    return out_ids.contiguous(), out_scores.contiguous()


def gini(counts):
    """the Gini index of a vector of non-negative counts, float64: sum_i (2 i - n - 1) x_(i) / (n sum x), x ascending, i from 1; 0 for
    an all-zero vector"""
    x, _ = torch.sort(counts.to(torch.float64).reshape(-1))
    n = int(x.numel())
    total = float(x.sum())
    if n == 0 or total == 0.0:
        return 0.0
    i = torch.arange(1, n + 1, dtype=torch.float64, device=x.device)
    return float(((2.0 * i - n - 1.0) * x).sum()) / (n * total)


def metrics_from_pair_sums(pair_sum, ids, n_cols, grid):
    """the list metrics at every cut-off K of `grid` from K17's pair sums (float64 [n, t]) and the lists (int [n, t], -1 padded); any
    device.  -> {'ild': [...], 'cov': [...], 'gini': [...]}, one float per K:
      ild   the mean over the rows with m = min(K, valid) >= 2 of  sum_{b < K} pair_sum[b] / (m (m - 1) / 2)  (0 when there is no such row)
      cov   the number of distinct ids in the rows' top-K prefixes / n_cols
      gini  the Gini index of how often each of the n_cols columns appears in those prefixes"""
    valid = valid_prefix(ids)
    n_valid = valid.sum(dim=1)
    cum = torch.cumsum(torch.where(valid, pair_sum.to(torch.float64), torch.zeros_like(pair_sum, dtype=torch.float64)), dim=1)
    out = {m: [] for m in LIST_METRICS}
    for K in grid:
        K = min(int(K), int(ids.shape[1]))
        m = torch.clamp(n_valid, max=K).to(torch.float64)
        rows = m >= 2
        if K >= 1 and bool(rows.any()):
            out['ild'].append(float((cum[:, K - 1][rows] / (m[rows] * (m[rows] - 1.0) / 2.0)).mean()))
        else:
            out['ild'].append(0.0)
        shown = ids[:, :K][valid[:, :K]].long()
        counts = torch.bincount(shown, minlength=n_cols)
        out['cov'].append(float((counts > 0).sum()) / n_cols)
        out['gini'].append(gini(counts))
    return out


def list_metrics(S, ids, n_cols, grid):
    """intra-list diversity (1 - similarity in S, averaged over the pairs of a list), coverage and exposure Gini of the lists `ids`
    (int32 [n, t] on the device, -1 padded) at every cut-off of `grid` -> the dict of metrics_from_pair_sums"""
    ids = ids.contiguous()
    if int(ids.shape[0]) == 0:
        return {m: [0.0] * len(grid) for m in LIST_METRICS}
    return metrics_from_pair_sums(tkr_hip.list_pair_sums(S, ids), ids, n_cols, grid)
