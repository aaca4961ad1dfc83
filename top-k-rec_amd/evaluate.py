"""evaluate.py -- accuracy@k of matrix-factorisation models, scored on MI355X.

Same command line and output as the reference's evaluate.py (flags :48-55, one stdout line per
scenario ``S,%.6f,...`` :113-117):

    python evaluate.py -d data -m embed/bpr -f 0 -s 5 -t 30 -sl im om

Same inputs: ``DATA/uid``, ``DATA/vid``, ``DATA/f{fold}tr.txt``, ``MODEL/final-U.dat``,
``final-V.dat``, optional ``final-B.dat``, ``DATA/f{fold}te.{S}.idl`` and ``.txt``.

What runs where: the text files are parsed by the native host parsers of libtkr_hip.so
(textio.py; one pass per file, flat arrays instead of dicts of sets -- SURVEY.md §8f n2; the
'%f ' matrices keep a binary ``.npy`` copy beside them, n1); the flat arrays are grouped into the like / rated / seen CSRs on the host or, from
TKR_GROUP_DEVICE_FROM parsed entries upward, on the GPU (K15, ``TKR_GROUP=host|device|auto``: the same arrays); the scores, the rated-item filter,
the top-``total`` selection (K4) and the hit counting (K5) run on the GPU -- the
[n_users, n_items] score matrix and its argsort (evaluate.py:78-81) are never materialised.

Stated differences from the reference:
  * ``final-B.dat`` is honoured for every scenario by gathering the bias per test id; the
    reference adds the whole vid-ordered bias row (:79-80), which raises unless the scenario's
    id list equals ``vid`` -- where it is defined, results are identical.
  * tie order among exactly equal scores is defined (higher test column first); the reference
    inherits numpy's unspecified unstable order.
  * only users that appear in the scenario's test file with at least one like are ranked
    (the reference scores every user and then reads only those rows).
  * under a torch.distributed launcher (one process per GPU) the test lines of every scenario are block-sharded over the
    ranks and the hit counters / like counts all-reduced; rank 0 prints.  The reference is single-process.
  * ids are resolved to indices while parsing, so the rated set of a user is keyed by the uid's
    index and a test column by its index in the id list; the reference keys both by token.  The
    two differ only if an id file repeats a token (the re-pointing quirk of evaluate.py:5-10).
  * ``-M/--metrics acc auc mrr ndcg map`` (not in the reference) prints, after the reference lines, one line
    ``S.metric,%.6f[,...]`` per scenario and metric from ONE full-rank pass: the filtered rank of every liked column (K8,
    tkr_hip.like_ranks) and rankmetrics.py.  Without the flag stdout is the reference's, byte for byte.
  * ``-M ... --negatives N [--neg-seed S]`` (not in the reference) adds, after those, ``S.negN.hr,...``, ``S.negN.ndcg,...`` and
    ``S.negN.mrr,...`` for the metrics of ``hr ndcg mrr`` that ``-M`` names: the sampled-negatives protocol of the BPR / NCF
    literature.  Every liked test column the user did not rate in training is ranked among N columns drawn without replacement from
    those the user neither rated in training nor has on that test line (rankmetrics.sample_negatives, seeded by S; all of them when
    fewer than N are eligible), by K12 (tkr_hip.rank_candidates).  ``hr`` exists only with ``--negatives``.
  * ``-M ... ild cov gini`` (not in the reference) prints, after all of those, ``S.ild,...``, ``S.cov,...`` and ``S.gini,...``: the
    intra-list diversity (1 - similarity of two items' factors, averaged over the pairs of a list and then over the lists), the share
    of the scenario's id list the lists reach and the Gini index of item exposure, of the scenario's ordinary top-``total`` lists at
    every cut-off step, 2 step, ... (K17, diversity.list_metrics).  ``-M ... unexp`` prints, after those, ``S.unexp,...``: the
    unexpectedness of the same lists -- 1 - the similarity of an item to the nearest item its user liked in the fold's training file,
    averaged over a list and then over the lists (K19, explain.py; the similarity table is the whole ``final-V.dat``'s, so scenarios
    whose items are outside the training matrix work); not with ``--bootstrap`` / ``--compare``.
    ``--diversify LAMBDA [--pool N] [--similarity cosine|dot]`` adds, after those, ``S.mmr.acc,...`` -- the accuracy lines' hit counting on the lists re-ranked by greedy MMR from the ``--pool`` best
    (diversity.rerank) -- and ``S.mmr.ild`` / ``.cov`` / ``.gini`` / ``.unexp`` for those of the four that ``-M`` names.  Single process only.
  * ``-M ... --bootstrap R [--boot-seed S] [--level L]`` (not in the reference) prints, after all of those, ``S.m.lo,...`` and
    ``S.m.hi,...`` for every m of ``acc auc mrr ndcg map`` that ``-M`` names: the percentile interval at level L (0.95) of the metric
    over R resamples of the scenario's test lines with replacement.  The ranks stay on the device from K8 to the resample sums (K18,
    significance.py); only the [R, columns] sums come down.  ``--compare MODEL_B`` ranks a second model directory on the same lines,
    resamples both together (a paired bootstrap) and adds ``S.vs.m`` (B's values), ``S.diff.m`` (this model - B), ``S.diff.m.lo`` /
    ``.hi`` and ``S.diff.m.p`` (two-sided).  Single process only.
"""
from __future__ import annotations

import argparse
import os

os.environ.setdefault('HSA_ENABLE_IPC_MODE_LEGACY', '0')     # multi-process GPU work on this driver needs dmabuf IPC; must be set before
                                                             # the HIP runtime starts, i.e. before the first torch.cuda call
import numpy as np
import torch

import diversity
import explain
import rankmetrics
import significance
import textio
import tkr_hip


def read_ids(path):
    """id token -> index in file order (evaluate.py:5-10)"""
    table = {}
    with open(path) as fh:
        for line in fh:
            table[line.strip()] = len(table)
    return table


def read_matrix(path, ids):
    """'%f ' text matrix rows addressed through ``ids`` (evaluate.py:19-28) -> fp32 [len(ids), k]"""
    every = textio.read_matrix(path)
    rows = np.unique(np.fromiter(ids.values(), dtype=np.int64, count=len(ids)))
    out = np.zeros((len(ids), every.shape[1]), dtype=np.float32)
    out[rows] = every[rows]
    return out


class Scenario:
    """One test scenario as flat arrays.  ``users`` [n] = uid index of every test line with >= 1 like (file order),
    ``like_ptr``/``like_cols``: its liked test columns, ascending (evaluate.py:84-95); ``rated_ptr``/``rated_cols``:
    the test columns on the user's train line, like 0 or 1 (evaluate.py:30-45,98); ``tcount`` = sum of |likes|."""

    def __init__(self, teids, users, like_ptr, like_cols, rated_ptr, rated_cols, seen_ptr=None, seen_cols=None):
        self.teids, self.users = teids, users
        self.like_ptr, self.like_cols, self.rated_ptr, self.rated_cols = like_ptr, like_cols, rated_ptr, rated_cols
        self.seen_ptr, self.seen_cols = seen_ptr, seen_cols          # every known column on the test line, whatever its like value
        self.tcount = int(like_ptr[-1])


def _group(rows, cols, n_rows, n_cols):
    """unique (row, col) pairs -> CSR over rows with ascending cols"""
    key = np.unique(rows.astype(np.int64) * n_cols + cols)
    ptr = np.zeros(n_rows + 1, dtype=np.int64)
    np.cumsum(np.bincount(key // n_cols, minlength=n_rows), out=ptr[1:])
    return ptr, (key % n_cols).astype(np.int32)


def load_scenario(data_dir, fold, scenario, uids, umap=None, where=None):
    """the Scenario of one test file.  where / TKR_GROUP: 'host' -- the arrays are grouped by numpy; 'device' -- by K15
    (tkr_hip.group_segments), and the Scenario also carries them as device tensors (``dev``) for K4 / K5 / K8; 'auto' (the default) -- the
    device when a GPU is visible, the two files hold at least TKR_GROUP_DEVICE_FROM entries, the arrays fit and the id list has at most
    tkr_hip.GROUP_MAX_COLS ids, else the host.  Same arrays, same KeyErrors either way"""
    where = textio._group_where(where)
    umap = umap or textio.IdMap(uids)
    teids = read_ids(os.path.join(data_dir, 'f%dte.%s.idl' % (fold, scenario)))
    temap = textio.IdMap(teids)
    n_te = max(len(teids), 1)
    te_path = os.path.join(data_dir, 'f%dte.%s.txt' % (fold, scenario))
    hist_path = os.path.join(data_dir, 'f%dtr.txt' % fold)
    T = H = None
    if textio.group_on_device(where, textio._group_device_from() if where == 'auto' else 0, n_te):      # 'auto': a GPU and an id list that fits
        T = textio.parse_ratings_for_group(te_path, umap, temap, where)
        n = textio.n_entries_of(T)
        if where == 'auto' and n < textio._group_device_from():
            try:                                                     # 'auto' decides by both files; what is wrong with the train file is
                H = textio.parse_ratings_for_group(hist_path, umap, temap, where)       # raised where the host path raises it
                n += textio.n_entries_of(H)
            except (OSError, ValueError):
                H = None
        if textio.group_on_device(where, n, n_te):
            try:
                sc = _load_scenario_device(T, H, te_path, hist_path, teids, temap, n_te, uids, umap, where)
                textio.group_counts['device'] += 1
                return sc
            except textio.DeviceGroupTooLarge:
                if where == 'device':
                    raise
        T, H = textio.ratings_to_host(T), None if H is None else textio.ratings_to_host(H)
    textio.group_counts['host'] += 1
    T = textio.parse_ratings(te_path, umap, temap) if T is None else T
    liked = T.like == 1
    if np.any(liked & (T.item < 0)):
        raise KeyError('%s likes an id that is not in the scenario id list' % te_path)        # teids[vid], :93
    lptr_all, lcols = _group(T.entry_line[liked], T.item[liked], len(T.line_user), n_te)
    lines = np.flatnonzero(np.diff(lptr_all) > 0)                                           # len(likes) != 0, :95
    users = T.line_user[lines].astype(np.int64)
    if np.any(users < 0):
        raise KeyError('%s: test user missing from the uid list' % te_path)                   # uids[uid], :98
    like_ptr = np.zeros(len(lines) + 1, dtype=np.int64)
    np.cumsum(np.diff(lptr_all)[lines], out=like_ptr[1:])
    # history: the LAST train line of a user is its rated set (rated[uid] = set() per line, :34)
    H = textio.parse_ratings(hist_path, umap, temap) if H is None else H
    n_users = max(int(max(uids.values())) + 1 if uids else 0, 1)
    last = np.full(n_users, -1, dtype=np.int64)
    known = np.flatnonzero(H.line_user >= 0)
    np.maximum.at(last, H.line_user[known], known)
    hl = last[users]
    if np.any(hl < 0):
        raise KeyError('%s: test user without a line in %s' % (te_path, hist_path))           # rated[uid], :98
    seg = H.line_ptr[hl + 1] - H.line_ptr[hl]
    row = np.repeat(np.arange(len(lines), dtype=np.int64), seg)
    pos = np.arange(int(seg.sum()), dtype=np.int64) - np.repeat(np.cumsum(seg) - seg, seg) + np.repeat(H.line_ptr[hl], seg)
    item = H.item[pos]
    keep = item >= 0                                                                         # only test columns matter
    rated_ptr, rated_cols = _group(row[keep], item[keep], len(lines), n_te)
    known = T.item >= 0
    sptr_all, scols_all = _group(T.entry_line[known], T.item[known], len(T.line_user), n_te)
    seen_ptr, seen_cols = _take_rows(sptr_all, scols_all, lines)
    return Scenario(teids, users, like_ptr, lcols, rated_ptr, rated_cols, seen_ptr, seen_cols)


def _load_scenario_device(T, H, te_path, hist_path, teids, temap, n_te, uids, umap, where, timing=None):
    """load_scenario with the grouping on the GPU (K15): T (and H, when 'auto' has parsed it already) are Ratings or RatingsDevice.  The
    checks are the host path's, in its order, each computed on the device and read back as one word.  timing: a dict that receives the
    seconds of 'download', the seven arrays to numpy at the end (scripts/time_group.py)"""
    dev = T.item.device if isinstance(T, textio.RatingsDevice) else torch.device('cuda', torch.cuda.current_device())
    T = textio.ratings_to_device(T, dev)
    n_lines, n_entries = int(T.line_user.numel()), int(T.item.numel())
    textio.group_fits(8 * n_entries + 40 * n_lines + 64, dev, 'the CSRs of %s' % te_path)
    lptr_all, lcols = tkr_hip.group_segments([(T.line_ptr, T.item, T.like, None)], n_lines, n_te, like_only=True)
    lines, like_ptr = tkr_hip.scenario_lines(lptr_all)               # len(likes) != 0, :95
    users = T.line_user[lines].to(torch.int64)
    bad = torch.stack([((T.like == 1) & (T.item < 0)).any(), (users < 0).any()]).tolist()
    if bad[0]:
        raise KeyError('%s likes an id that is not in the scenario id list' % te_path)        # teids[vid], :93
    if bad[1]:
        raise KeyError('%s: test user missing from the uid list' % te_path)                   # uids[uid], :98
    H = textio.ratings_to_device(textio.parse_ratings_for_group(hist_path, umap, temap, where) if H is None else H, dev)
    n_users = max(int(max(uids.values())) + 1 if uids else 0, 1)
    last = tkr_hip.last_line_of_user(H.line_user, n_users)           # the LAST train line of a user is its rated set, :34
    hl = last[users]
    if bool((hl < 0).any().item()):
        raise KeyError('%s: test user without a line in %s' % (te_path, hist_path))           # rated[uid], :98
    n = int(lines.numel())
    textio.group_fits(4 * int(H.item.numel()) + 4 * n_entries + 16 * n + 64, dev, 'the CSRs of %s' % te_path)
    rated_ptr, rated_cols = tkr_hip.group_segments([(H.line_ptr, H.item, None, hl.contiguous())], n, n_te)
    seen_ptr, seen_cols = tkr_hip.group_segments([(T.line_ptr, T.item, None, lines)], n, n_te)
    if timing is not None:
        import time
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
    host = [t.cpu().numpy() for t in (users, like_ptr, lcols, rated_ptr, rated_cols, seen_ptr, seen_cols)]
    if timing is not None:
        timing['download'] = time.perf_counter() - t0
    sc = Scenario(teids, *host)
    sc.dev = dict(users=users, like_ptr=like_ptr, like_cols=lcols, rated_ptr=rated_ptr, rated_cols=rated_cols, seen_ptr=seen_ptr,
                  seen_cols=seen_cols)
    return sc


def _on_device(sc, device, *names):
    """the arrays `names` of a Scenario on `device`: the tensors K15 left there, else uploaded"""
    kept = getattr(sc, 'dev', None)
    if kept is not None and kept[names[0]].device == torch.device(device):
        return tuple(kept[n] for n in names)
    return tuple(torch.from_numpy(getattr(sc, n)).to(device) for n in names)


def _take_rows(ptr, cols, rows):
    """the rows `rows` of a CSR, in that order -> (ptr, cols)"""
    seg = ptr[rows + 1] - ptr[rows]
    out = np.zeros(len(rows) + 1, dtype=np.int64)
    np.cumsum(seg, out=out[1:])
    pos = np.arange(int(out[-1]), dtype=np.int64) - np.repeat(out[:-1], seg) + np.repeat(ptr[rows], seg)
    return out, cols[pos]


def _scenario_operands(vmat, bmat, vids, sc, device):
    """the scenario's test-item rows, bias, user rows and rated mask on the device: the operands of K4 and K8"""
    te_rows = np.zeros(len(sc.teids), dtype=np.int64)
    for vid, col in sc.teids.items():
        te_rows[col] = vids[vid]                                     # evaluate.py:75-77
    Vt = torch.from_numpy(np.ascontiguousarray(vmat[te_rows])).to(device)
    bias = None
    if bmat is not None:
        bias = torch.from_numpy(np.ascontiguousarray(bmat.reshape(-1)[te_rows])).to(device)
    users, rptr, rcols = _on_device(sc, device, 'users', 'rated_ptr', 'rated_cols')
    user_idx = users.to(torch.int32)
    mask, pitch = tkr_hip.build_rated_mask(rptr, rcols, len(sc.users), len(sc.teids))
    return Vt, bias, user_idx, mask, pitch


def rank_scenario(umat_dev, vmat, bmat, vids, sc, total, device, want_scores=False):
    """filtered top-`total` test columns of every test line -> int32 [n_lines, total] (device)"""
    Vt, bias, user_idx, mask, pitch = _scenario_operands(vmat, bmat, vids, sc, device)
    return tkr_hip.score_topk(umat_dev, Vt, total, bias=bias, user_idx=user_idx, mask=mask, mask_pitch=pitch,
                              want_scores=want_scores)


def shard_scenario(sc, rank, world):
    """the contiguous block of test lines rank `rank` of `world` ranks scores (users are independent: SURVEY.md §8e)"""
    n = len(sc.users)
    lo, hi = rank * n // world, (rank + 1) * n // world
    lp, rp = sc.like_ptr, sc.rated_ptr
    sp = sc.seen_ptr
    seen = (None, None) if sp is None else (sp[lo:hi + 1] - sp[lo], sc.seen_cols[sp[lo]:sp[hi]])
    return Scenario(sc.teids, sc.users[lo:hi], lp[lo:hi + 1] - lp[lo], sc.like_cols[lp[lo]:lp[hi]],
                    rp[lo:hi + 1] - rp[lo], sc.rated_cols[rp[lo]:rp[hi]], *seen)


def _world():
    import torch.distributed as dist
    if dist.is_available() and dist.is_initialized():
        return dist.get_rank(), dist.get_world_size()
    return 0, 1


def evaluate_scenario(umat_dev, vmat, bmat, uids, vids, data_dir, fold, scenario, step, total, device, umap=None):
    """accuracy@(step, 2*step, ...) of one scenario (evaluate.py:72-112).  Under torch.distributed every rank ranks its
    block of the scenario's test lines; what the reference accumulates over users -- tresults[k] and tcount, :106-112 --
    is summed over the ranks by one all-reduce of interval + 1 integers (no other exchange: the factors are replicated)."""
    full = load_scenario(data_dir, fold, scenario, uids, umap)
    return evaluate_loaded(umat_dev, vmat, bmat, vids, full, step, total, device)


def evaluate_loaded(umat_dev, vmat, bmat, vids, full, step, total, device):
    """the ranking + counting half of evaluate_scenario on an already parsed Scenario (the same on every rank)"""
    rank, world = _world()
    sc = shard_scenario(full, rank, world) if world > 1 else full
    interval = total // step
    hits = np.zeros(interval, dtype=np.int64)
    if len(sc.users):
        ids = rank_scenario(umat_dev, vmat, bmat, vids, sc, total, device)
        lptr, lcols = _on_device(sc, device, 'like_ptr', 'like_cols')
        hits = tkr_hip.count_hits(ids, lptr, lcols, step, interval).cpu().numpy()
    tcount = sc.tcount
    if world > 1:
        import torch.distributed as dist
        on_dev = dist.get_backend() == 'nccl'                        # RCCL reduces device tensors, gloo host tensors
        acc = torch.from_numpy(np.r_[hits, tcount].astype(np.int64))
        acc = acc.to(device) if on_dev else acc
        dist.all_reduce(acc, op=dist.ReduceOp.SUM)
        acc = acc.cpu().numpy()
        hits, tcount = acc[:interval], int(acc[interval])
    return [float(h) / tcount for h in hits]                          # ZeroDivisionError like evaluate.py:112


def like_ranks_loaded(umat_dev, vmat, bmat, vids, sc, device):
    """K8 on an already parsed Scenario with at least one line -> the filtered rank of every liked column, int32 [n_likes] (device)"""
    Vt, bias, user_idx, mask, pitch = _scenario_operands(vmat, bmat, vids, sc, device)
    lptr, lcols = _on_device(sc, device, 'like_ptr', 'like_cols')
    return tkr_hip.like_ranks(umat_dev, Vt, lptr, lcols, bias=bias, user_idx=user_idx, mask=mask, mask_pitch=pitch)


def rank_metrics_loaded(umat_dev, vmat, bmat, vids, full, step, total, metrics, device, keep=None):
    """{metric: list of values} (rankmetrics.py) of an already parsed Scenario from one full-rank pass: K8 gives the filtered rank of
    every liked column of this rank's block of test lines, the metric sums and counts are all-reduced like the hits of
    evaluate_loaded (one fp64 vector; the same on every rank afterwards).  keep: a dict that receives K8's output, still on the device,
    as 'ranks' (None without a test line)."""
    rank, world = _world()
    sc = shard_scenario(full, rank, world) if world > 1 else full
    ranks, ranks_dev = np.zeros(0, dtype=np.int32), None
    if len(sc.users):
        ranks_dev = like_ranks_loaded(umat_dev, vmat, bmat, vids, sc, device)
        ranks = ranks_dev.cpu().numpy()
    if keep is not None:
        keep['ranks'] = ranks_dev
    sums = rankmetrics.rank_sums(ranks, sc.like_ptr, sc.rated_ptr, len(sc.teids), step, total)
    if world > 1:
        import torch.distributed as dist
        on_dev = dist.get_backend() == 'nccl'
        acc = torch.from_numpy(rankmetrics.to_vector(sums))
        acc = acc.to(device) if on_dev else acc
        dist.all_reduce(acc, op=dist.ReduceOp.SUM)
        sums = rankmetrics.from_vector(acc.cpu().numpy(), total // step)
    return rankmetrics.finish(sums, metrics)


def significance_loaded(ranks_dev, umat_b, vmat_b, bmat_b, vids, sc, step, total, metrics, boot, device):
    """the bootstrap figures of an already parsed Scenario (single process) -> significance.report's dict.  ranks_dev: K8's ranks of the
    model under evaluation (device); umat_b (device) / vmat_b / bmat_b: the model of --compare, or None; boot: dict(R, seed, level).
    The line tables of both models are built, joined and resampled on the device (K18); only the column sums come down"""
    if ranks_dev is None:
        raise ZeroDivisionError('--bootstrap: no test line to resample')
    lptr, rptr = _on_device(sc, device, 'like_ptr', 'rated_ptr')
    X = significance.line_table(ranks_dev, lptr, rptr, len(sc.teids), step, total)
    if umat_b is not None:
        ranks_b = like_ranks_loaded(umat_b, vmat_b, bmat_b, vids, sc, device)
        X = torch.cat([X, significance.line_table(ranks_b, lptr, rptr, len(sc.teids), step, total)], dim=1).contiguous()
    reps = significance.bootstrap_sums(X, boot['R'], boot['seed']).cpu().numpy()
    return significance.report(X.sum(dim=0).cpu().numpy(), reps, total // step, metrics, boot['level'], 2 if umat_b is not None else 1)


def negative_rows(sc, n_neg, seed):
    """the candidate rows of the sampled-negatives protocol for a parsed Scenario: one row per liked column that is not train-rated
    -> (line of every row, cand_ptr, cand_cols, like_at) (rankmetrics.sample_negatives)"""
    n, n_te = len(sc.users), max(len(sc.teids), 1)
    line = np.repeat(np.arange(n, dtype=np.int64), np.diff(sc.like_ptr))
    rated_line = np.repeat(np.arange(n, dtype=np.int64), np.diff(sc.rated_ptr))
    rated = np.isin(line * n_te + sc.like_cols, rated_line * n_te + sc.rated_cols)
    lptr, lcols = _group(line[~rated], sc.like_cols[~rated], n, n_te)
    seen_line = np.repeat(np.arange(n, dtype=np.int64), np.diff(sc.seen_ptr))
    xptr, xcols = _group(np.concatenate([rated_line, seen_line]), np.concatenate([sc.rated_cols, sc.seen_cols]).astype(np.int64), n, n_te)
    cand_ptr, cand_cols, like_at = rankmetrics.sample_negatives(lptr, lcols, xptr, xcols, len(sc.teids), n_neg, seed)
    return np.repeat(np.arange(n, dtype=np.int64), np.diff(lptr)), cand_ptr, cand_cols, like_at


def negative_metrics_loaded(umat_dev, vmat, bmat, vids, full, step, total, n_neg, seed, metrics, device):
    """{metric: list of values} of hr / ndcg / mrr against sampled negatives.  The rows are drawn for the whole scenario on every rank
    (a host function of the seed: the same rows whatever the number of ranks); a rank scores the rows of its block of test lines --
    the block shard_scenario gives it -- with K12, and the sums are all-reduced like those of rank_metrics_loaded."""
    rank, world = _world()
    line, cand_ptr, cand_cols, like_at = negative_rows(full, n_neg, seed)
    n = len(full.users)
    lo, hi = (rank * n // world, (rank + 1) * n // world) if world > 1 else (0, n)
    q0, q1 = int(np.searchsorted(line, lo)), int(np.searchsorted(line, hi))
    like_ranks = np.zeros(0, dtype=np.int32)
    if q1 > q0:
        te_rows = np.zeros(len(full.teids), dtype=np.int64)
        for vid, col in full.teids.items():
            te_rows[col] = vids[vid]
        Vt = torch.from_numpy(np.ascontiguousarray(vmat[te_rows])).to(device)
        bias = None if bmat is None else torch.from_numpy(np.ascontiguousarray(bmat.reshape(-1)[te_rows])).to(device)
        user_idx = torch.from_numpy(full.users[line[q0:q1]].astype(np.int32)).to(device)
        ptr = cand_ptr[q0:q1 + 1] - cand_ptr[q0]
        cols = cand_cols[cand_ptr[q0]:cand_ptr[q1]]
        _, ranks = tkr_hip.rank_candidates(umat_dev, Vt, torch.from_numpy(ptr).to(device), torch.from_numpy(cols).to(device), bias=bias,
                                           user_idx=user_idx)
        like_ranks = ranks.cpu().numpy()[like_at[q0:q1] - cand_ptr[q0]]
    sums = rankmetrics.negative_sums(like_ranks, step, total)
    if world > 1:
        import torch.distributed as dist
        on_dev = dist.get_backend() == 'nccl'
        acc = torch.from_numpy(rankmetrics.neg_to_vector(sums))
        acc = acc.to(device) if on_dev else acc
        dist.all_reduce(acc, op=dist.ReduceOp.SUM)
        sums = rankmetrics.neg_from_vector(acc.cpu().numpy(), total // step)
    return rankmetrics.finish(sums, metrics)


def list_metrics_loaded(umat_dev, vmat, bmat, vids, sc, step, total, metrics, div, device, anchors=None):
    """the list metrics of an already parsed Scenario (single process) -> (plain, mmr): {metric: values at step, 2 step, ...} of the
    ordinary top-`total` lists for the `metrics` of diversity.LIST_METRICS, and -- with div, the arguments of --diversify -- the same of
    the lists K17 re-ranks out of the div['pool'] best, plus 'acc': K5's hit count on them as evaluate_loaded reports it (else None).
    anchors: (ptr, cols) on the device, the training likes of every test line's user in the `vid` numbering -- both dicts then also
    hold 'unexp', the unexpectedness of the lists against them (K19, explain.list_unexpectedness): the similarity table is the whole
    final-V.dat's, and the lists' test columns are mapped to its rows first"""
    interval = total // step
    grid = [step * (q + 1) for q in range(interval)]
    plain = {m: [0.0] * interval for m in list(metrics) + (['unexp'] if anchors is not None else [])}
    mmr = dict(plain, acc=[0.0] * interval) if div else None
    if not len(sc.users):
        return plain, mmr
    unexp = None
    if anchors is not None:
        te_rows = np.zeros(len(sc.teids), dtype=np.int64)
        for vid, col in sc.teids.items():
            te_rows[col] = vids[vid]
        te_rows = torch.from_numpy(te_rows.astype(np.int32)).to(device)
        S_full = diversity.similarity_table(torch.from_numpy(vmat).to(device), div['similarity'] if div else 'cosine')

        def unexp(lists):
            as_vid = torch.where(lists >= 0, te_rows[lists.clamp(min=0).long()], torch.full_like(lists, -1)).contiguous()
            return explain.list_unexpectedness(S_full, as_vid, anchors[0], anchors[1], grid)
    Vt, bias, user_idx, mask, pitch = _scenario_operands(vmat, bmat, vids, sc, device)
    S = diversity.similarity_table(Vt, div['similarity'] if div else 'cosine')
    n_cols = len(sc.teids)
    ids, scores = tkr_hip.score_topk(umat_dev, Vt, div['pool'] if div else total, bias=bias, user_idx=user_idx, mask=mask, mask_pitch=pitch,
                                     want_scores=True)
    if metrics:
        every = diversity.list_metrics(S, ids[:, :total].contiguous(), n_cols, grid)
        plain = {m: every[m] for m in metrics}
    if unexp:
        plain['unexp'] = unexp(ids[:, :total])
    if div:
        picked, _ = diversity.rerank(S, diversity.relevance(ids, scores), ids, scores, div['diversify'], total)
        lptr, lcols = _on_device(sc, device, 'like_ptr', 'like_cols')
        hits = tkr_hip.count_hits(picked, lptr, lcols, step, interval).cpu().numpy()
        mmr = {'acc': [float(h) / sc.tcount for h in hits]}
        if metrics:
            every = diversity.list_metrics(S, picked, n_cols, grid)
            mmr.update({m: every[m] for m in metrics})
        if unexp:
            mmr['unexp'] = unexp(picked)
    return plain, mmr


def main(argv=None):
    parser = argparse.ArgumentParser(description="Evaluate weighted matrix factorization based methods.")
    parser.add_argument('-d', '--data', required=True, help="The data path for the evaluation")
    parser.add_argument('-m', '--model', required=True, help="The work path for the model")
    parser.add_argument('-f', '--fold', type=int, default=0, help="The index of evaluation fold")
    parser.add_argument('-s', '--step', type=int, default=5, help="The number of evaluation step")
    parser.add_argument('-t', '--total', type=int, default=30, help="The number of total predictions")
    parser.add_argument('-sl', '--scenarios', nargs='+', default=None, help="The test scenario list")
    parser.add_argument('-M', '--metrics', nargs='+', default=None, choices=rankmetrics.METRICS + ('hr',) + diversity.LIST_METRICS + explain.METRICS,
                        help="Rank metrics from one full-rank pass, printed after the accuracy lines as S.metric,... (hr: only with --negatives); "
                             "ild cov gini: diversity, coverage and exposure Gini of the top-k lists; unexp: their unexpectedness against the "
                             "users' training likes")
    parser.add_argument('--negatives', type=int, default=None, metavar='N',
                        help="With -M: also rank every held-out like among N sampled unrated columns; prints S.negN.hr / .ndcg / .mrr")
    parser.add_argument('--neg-seed', type=int, default=0, help="The seed of the negatives' draw")
    diversity.add_arguments(parser)
    parser.add_argument('--bootstrap', type=int, default=None, metavar='R',
                        help="With -M acc auc mrr ndcg map: the percentile interval of every metric over R resamples of the test lines; "
                             "prints S.metric.lo / .hi")
    parser.add_argument('--boot-seed', type=int, default=0, help="The seed of the resampling")
    parser.add_argument('--level', type=float, default=0.95, help="The level of the bootstrap intervals, inside (0, 1)")
    parser.add_argument('--compare', default=None, metavar='MODEL_B',
                        help="With --bootstrap: a second model directory, resampled on the same lines; prints S.vs.metric, S.diff.metric, "
                             "its interval and its two-sided p")
    args = parser.parse_args(argv)
    div = diversity.check_arguments(parser, args)
    list_metrics = [m for m in args.metrics or () if m in diversity.LIST_METRICS]
    if (div or list_metrics) and int(os.environ.get('WORLD_SIZE', '1')) > 1:
        parser.error('ild / cov / gini and --diversify look at whole lists and are not sharded over ranks yet: run them in a single process')
    unexp = 'unexp' in (args.metrics or ())
    if unexp and int(os.environ.get('WORLD_SIZE', '1')) > 1:
        parser.error('unexp looks at whole lists and is not sharded over ranks yet: run it in a single process')
    if unexp and (args.bootstrap is not None or args.compare is not None):
        parser.error('unexp looks at whole lists and is not resampled yet: run it without --bootstrap / --compare')
    if args.negatives is not None and not args.metrics:
        parser.error('--negatives needs -M (hr, ndcg and / or mrr)')
    if args.negatives is not None and args.negatives < 1:
        parser.error('--negatives must be at least 1')
    if args.metrics and 'hr' in args.metrics and args.negatives is None:
        parser.error('-M hr is defined against sampled negatives only: add --negatives N')
    full_metrics = [m for m in args.metrics or () if m in rankmetrics.METRICS]
    if args.compare is not None and args.bootstrap is None:
        parser.error('--compare needs --bootstrap R')
    if args.bootstrap is not None and not full_metrics:
        parser.error('--bootstrap needs -M with at least one of acc auc mrr ndcg map')
    if args.bootstrap is not None and not 1 <= args.bootstrap < 2 ** 31:
        parser.error('--bootstrap must be at least 1')
    if not 0 <= args.boot_seed < 2 ** 64:
        parser.error('--boot-seed must be a 64-bit unsigned integer')
    if not 0.0 < args.level < 1.0:
        parser.error('--level must lie inside (0, 1)')
    if args.bootstrap is not None and int(os.environ.get('WORLD_SIZE', '1')) > 1:
        parser.error('--bootstrap and --compare look at whole lists and are not sharded over ranks yet: run them in a single process')
    boot = dict(R=args.bootstrap, seed=args.boot_seed, level=args.level) if args.bootstrap is not None else None
    neg_metrics = [m for m in args.metrics or () if m in rankmetrics.NEG_METRICS] if args.negatives is not None else []

    if not torch.cuda.is_available():
        raise tkr_hip.TkrError('evaluate.py scores on the GPU through libtkr_hip.so; no MI355X is visible')
    started_group = _init_distributed()
    rank, _ = _world()
    device = torch.device('cuda', torch.cuda.current_device())
    uids = read_ids(os.path.join(args.data, 'uid'))
    vids = read_ids(os.path.join(args.data, 'vid'))
    umat = read_matrix(os.path.join(args.model, 'final-U.dat'), uids)
    vmat = read_matrix(os.path.join(args.model, 'final-V.dat'), vids)
    bmat = None
    if os.path.exists(os.path.join(args.model, 'final-B.dat')):
        bmat = read_matrix(os.path.join(args.model, 'final-B.dat'), vids)
    umat_dev = torch.from_numpy(umat).to(device)
    umap = textio.IdMap(uids)
    umat_b = vmat_b = bmat_b = None
    if args.compare is not None:                                     # model B: the same uid / vid lists
        umat_b = torch.from_numpy(read_matrix(os.path.join(args.compare, 'final-U.dat'), uids)).to(device)
        vmat_b = read_matrix(os.path.join(args.compare, 'final-V.dat'), vids)
        if os.path.exists(os.path.join(args.compare, 'final-B.dat')):
            bmat_b = read_matrix(os.path.join(args.compare, 'final-B.dat'), vids)
    results, extra, negs, lists, boots = {}, {}, {}, {}, {}
    liked = textio.parse_ratings(os.path.join(args.data, 'f%dtr.txt' % args.fold), umap, textio.IdMap(vids)) if unexp else None
    for scenario in args.scenarios:
        if args.metrics or div:
            full = load_scenario(args.data, args.fold, scenario, uids, umap)
            acc = evaluate_loaded(umat_dev, vmat, bmat, vids, full, args.step, args.total, device)
            if scenario not in extra:                                # (a scenario listed twice: its metric lines are not doubled)
                kept = {} if boot else None
                extra[scenario] = rank_metrics_loaded(umat_dev, vmat, bmat, vids, full, args.step, args.total, full_metrics, device, kept)
                if boot:
                    boots[scenario] = significance_loaded(kept['ranks'], umat_b, vmat_b, bmat_b, vids, full, args.step, args.total,
                                                          full_metrics, boot, device)
                if neg_metrics:
                    negs[scenario] = negative_metrics_loaded(umat_dev, vmat, bmat, vids, full, args.step, args.total, args.negatives,
                                                             args.neg_seed, neg_metrics, device)
                if list_metrics or div or unexp:
                    anchors = explain.anchors_csr([liked], full.users, len(vmat), device) if unexp else None
                    lists[scenario] = list_metrics_loaded(umat_dev, vmat, bmat, vids, full, args.step, args.total, list_metrics, div, device,
                                                          anchors)
        else:
            acc = evaluate_scenario(umat_dev, vmat, bmat, uids, vids, args.data, args.fold, scenario, args.step, args.total, device, umap)
        if scenario not in results:                                  # evaluate.py:109-112 ACCUMULATES per scenario name: a scenario
            results[scenario] = [0.0] * len(acc)                     # listed twice ("-sl im im") prints doubled values, twice
        for k, v in enumerate(acc):
            results[scenario][k] += v
    lines = []
    for scenario in args.scenarios:
        lines.append(scenario + ''.join(',%.6f' % v for v in results[scenario]))
        if rank == 0:                                                # one report, like the single process
            print(lines[-1])
    for scenario in args.scenarios if args.metrics else ():
        for m in full_metrics:
            lines.append('%s.%s' % (scenario, m) + ''.join(',%.6f' % v for v in extra[scenario][m]))
            if rank == 0:
                print(lines[-1])
    for scenario in args.scenarios if neg_metrics else ():
        for m in neg_metrics:
            lines.append('%s.neg%d.%s' % (scenario, args.negatives, m) + ''.join(',%.6f' % v for v in negs[scenario][m]))
            if rank == 0:
                print(lines[-1])
    list_names = list_metrics + (['unexp'] if unexp else [])
    for which, names in ((0, list_names), (1, (['acc'] + list_names) if div else [])):
        for scenario in args.scenarios if names else ():
            for m in names:
                lines.append('%s.%s%s' % (scenario, 'mmr.' if which else '', m) + ''.join(',%.6f' % v for v in lists[scenario][which][m]))
                print(lines[-1])                                     # (single process: refused above otherwise)
    named = [('%s.lo', 'lo'), ('%s.hi', 'hi')]                       # (the line's name after 'S.', significance.report's key)
    if args.compare is not None:
        named += [('vs.%s', 'vs'), ('diff.%s', 'diff'), ('diff.%s.lo', 'diff.lo'), ('diff.%s.hi', 'diff.hi'), ('diff.%s.p', 'diff.p')]
    for scenario in args.scenarios if boot else ():
        for m in full_metrics:
            for name, key in named:
                lines.append('%s.%s' % (scenario, name % m) + ''.join(',%.6f' % v for v in boots[scenario][m][key]))
                print(lines[-1])                                     # (single process: refused above otherwise)
    if started_group:
        import torch.distributed as dist
        dist.destroy_process_group()
    return lines


def _init_distributed():
    """One process per GPU when started by a launcher (python -m torch.distributed.run --nproc-per-node N evaluate.py ...):
    RANK / WORLD_SIZE / LOCAL_RANK in the environment.  Backend 'nccl' (= RCCL over xGMI) unless TKR_DIST_BACKEND says
    otherwise; TKR_SINGLE_DEVICE=1 puts every rank on GPU 0 (tests on a one-GPU box, with gloo).  Returns True when this
    call created the process group."""
    import torch.distributed as dist
    world = int(os.environ.get('WORLD_SIZE', '1'))
    if world <= 1 or not dist.is_available() or dist.is_initialized():
        return False
    local = 0 if os.environ.get('TKR_SINGLE_DEVICE') == '1' else int(os.environ.get('LOCAL_RANK', '0'))
    torch.cuda.set_device(local)
    backend = os.environ.get('TKR_DIST_BACKEND', 'nccl')
    if backend == 'nccl':
        dist.init_process_group('nccl', device_id=torch.device('cuda', local))
    else:
        dist.init_process_group(backend)
    return True


if __name__ == '__main__':
    main()
