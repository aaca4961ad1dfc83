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

  * ``-m DIR`` (or ``--compare DIR``) where DIR holds ``knn.npz`` is a neighbourhood model (knn.ItemKNN, K28): it has no
    ``final-*.dat``.  A test line's history is its user's like == 1 entries of ``f{fold}tr.txt`` in the ``vid`` numbering, the mask is
    the scenario's rated mask as for any model, and K29 (tkr_hip.knn_score) gives the lists and the ranks (``KnnRanker``).  The accuracy
    lines, ``-M acc auc mrr ndcg map``, ``--bootstrap`` and ``--compare`` in both directions work; ``--negatives``, ``--diversify``,
    ``-M ild cov gini unexp`` and a multi-process launch end in a parser error: there are no item factors to sample against, to
    measure similarity in or to replicate.

How a scenario is ranked: once per entry of ``-sl``, ``main`` makes the ``Lines`` of this rank's shard (user rows, like CSR and, on first
use, the rated mask on the device; they depend on the Scenario alone) and a ``Ranker`` of the user table and the model on them, which
builds the model's ``Items`` (the test ids' rows of final-V.dat and final-B.dat) on first use and offers K4, K8 and K5.  Every
``*_loaded`` function of ``main`` takes that Ranker; ``--compare``'s model gets a Ranker of its own on the same Lines.
"""
from __future__ import annotations

import argparse
import collections
import functools
import os

os.environ.setdefault('HSA_ENABLE_IPC_MODE_LEGACY', '0')     # multi-process GPU work on this driver needs dmabuf IPC; must be set before
                                                             # the HIP runtime starts, i.e. before the first torch.cuda call
import numpy as np
import torch

import diversity
import explain
import foldin
import knn
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


def read_model(model_dir, uids=None, vids=None):
    """a model directory through the id lists -> (U, V, b): final-U.dat when ``uids`` is given, final-V.dat and final-B.dat ([n, 1];
    None when the file is absent) when ``vids`` is; None for what was not asked for, whose files are not opened"""
    U = V = b = None
    if uids is not None:
        U = read_matrix(os.path.join(model_dir, 'final-U.dat'), uids)
    if vids is not None:
        V = read_matrix(os.path.join(model_dir, 'final-V.dat'), vids)
        if os.path.exists(os.path.join(model_dir, 'final-B.dat')):
            b = read_matrix(os.path.join(model_dir, 'final-B.dat'), vids)
    return U, V, b


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


class Lines:
    """The test lines of a Scenario -- whole, or one rank's shard -- on the device.  It depends on the Scenario alone, so every model
    ranked on these lines shares it.  The rated mask is built on first use and kept: a path that needs none launches none."""

    def __init__(self, sc, device):
        self.sc, self.device = sc, device
        users, self.like_ptr, self.like_cols, self.rated_ptr = _on_device(sc, device, 'users', 'like_ptr', 'like_cols', 'rated_ptr')
        self.user_idx = users.to(torch.int32)

    @functools.cached_property
    def mask(self):
        """(the bit mask of every line's train-rated test columns, its pitch)"""
        return tkr_hip.build_rated_mask(self.rated_ptr, *_on_device(self.sc, self.device, 'rated_cols'), len(self.sc.users), len(self.sc.teids))


Items = collections.namedtuple('Items', 'te_rows Vt bias')


def scenario_items(vmat, bmat, vids, teids, device):
    """a model's rows of a scenario's test ids -> Items: ``te_rows`` int64 [n_te], the row of final-V.dat of every test column; those
    rows of it (``Vt``) and of final-B.dat (``bias``, None without one) on the device"""
    te_rows = np.zeros(len(teids), dtype=np.int64)
    for vid, col in teids.items():
        te_rows[col] = vids[vid]                                     # evaluate.py:75-77 (KeyError: a test id that `vid` lacks)
    Vt = torch.from_numpy(np.ascontiguousarray(vmat[te_rows])).to(device)
    return Items(te_rows, Vt, None if bmat is None else torch.from_numpy(np.ascontiguousarray(bmat.reshape(-1)[te_rows])).to(device))


class Ranker:
    """A user table on the device, a model (vmat, bmat, vids) and the Lines it is ranked on: the operands of K4 (score_topk), K8
    (like_ranks) and K5 (count_hits).  The model's Items are built on first use, as the mask is: a shard without lines builds neither."""

    def __init__(self, umat_dev, model, lines):
        self.umat, self.model, self.lines = umat_dev, model, lines

    @functools.cached_property
    def items(self):
        return scenario_items(*self.model, self.lines.sc.teids, self.lines.device)

    def _filter(self):
        mask, pitch = self.lines.mask
        return dict(bias=self.items.bias, user_idx=self.lines.user_idx, mask=mask, mask_pitch=pitch)

    def score_topk(self, K, want_scores=False):
        return tkr_hip.score_topk(self.umat, self.items.Vt, K, want_scores=want_scores, **self._filter())

    def like_ranks(self):
        return tkr_hip.like_ranks(self.umat, self.items.Vt, self.lines.like_ptr, self.lines.like_cols, **self._filter())

    def count_hits(self, ids, step, interval):
        return tkr_hip.count_hits(ids, self.lines.like_ptr, self.lines.like_cols, step, interval)


class KnnRanker:
    """Ranker's three methods for a neighbourhood model (knn.ItemKNN, a directory with knn.npz): K29 (tkr_hip.knn_score) in place of K4
    and K8.  liked: the (ptr, cols) CSR over the uid indices of the like == 1 entries of the fold's train file in the `vid` numbering --
    a line's history is its user's row.  The test columns are a subset of `vid`: col_of_item maps a catalogue item to its column or -1"""

    def __init__(self, model, liked, vids, lines):
        if model.n_items != max(vids.values()) + 1:
            raise ValueError('the neighbourhood model holds %d items, the vid list %d' % (model.n_items, max(vids.values()) + 1))
        self.model, self.liked, self.vids, self.lines = model, liked, vids, lines

    @functools.cached_property
    def items(self):
        """(history ptr, history cols, col_of_item) of the lines on the device"""
        sc, device = self.lines.sc, self.lines.device
        col_of_item = np.full(self.model.n_items, -1, dtype=np.int32)
        for vid, col in sc.teids.items():
            col_of_item[self.vids[vid]] = col                        # (KeyError: a test id that `vid` lacks, as scenario_items)
        ptr, cols = _take_rows(self.liked[0], self.liked[1], np.asarray(sc.users, dtype=np.int64))
        return tuple(torch.from_numpy(np.ascontiguousarray(a)).to(device) for a in (ptr, cols, col_of_item))

    def _call(self, K, **kw):
        mask, pitch = self.lines.mask
        ptr, cols, col_of_item = self.items
        return tkr_hip.knn_score(ptr, cols, *self.model.table(self.lines.device), K, col_of_item=col_of_item, n_cols=len(self.lines.sc.teids),
                                 mask=mask, mask_pitch=pitch, **kw)

    def score_topk(self, K, want_scores=False):
        return self._call(K, want_scores=want_scores)

    def like_ranks(self):
        return self._call(0, like_ptr=self.lines.like_ptr, like_cols=self.lines.like_cols)

    def count_hits(self, ids, step, interval):
        return tkr_hip.count_hits(ids, self.lines.like_ptr, self.lines.like_cols, step, interval)


def knn_refusals(parser, args, what='the model'):
    """the flags a neighbourhood model (a directory with knn.npz) cannot serve: it has no factors to sample against, to measure
    similarity in or to shard"""
    tail = 'is not available for a neighbourhood model (%s holds knn.npz): it has no item factors' % what
    if args.negatives is not None:
        parser.error('--negatives ' + tail)
    if args.diversify is not None:
        parser.error('--diversify ' + tail)
    listy = [m for m in args.metrics or () if m in diversity.LIST_METRICS + explain.METRICS]
    if listy:
        parser.error('-M %s %s' % (' '.join(listy), tail))
    if int(os.environ.get('WORLD_SIZE', '1')) > 1:
        parser.error('a multi-process launch (WORLD_SIZE > 1) is not available for a neighbourhood model (%s holds knn.npz): run it in a '
                     'single process' % what)


def rank_scenario(umat_dev, vmat, bmat, vids, sc, total, device, want_scores=False):
    """filtered top-`total` test columns of every test line -> int32 [n_lines, total] (device)"""
    return Ranker(umat_dev, (vmat, bmat, vids), Lines(sc, device)).score_topk(total, want_scores)


def _block(n, rank, world):
    """the lines [lo, hi) of n that rank `rank` of `world` ranks takes"""
    return rank * n // world, (rank + 1) * n // world


def shard_scenario(sc, rank, world):
    """the contiguous block of test lines rank `rank` of `world` ranks scores (users are independent: SURVEY.md §8e)"""
    lo, hi = _block(len(sc.users), rank, world)
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


def _shard(full):
    """-> (the Scenario this rank ranks -- `full` itself in a single process --, rank, world)"""
    rank, world = _world()
    return (shard_scenario(full, rank, world) if world > 1 else full), rank, world


def _sum_over_ranks(vec, device):
    """a host vector summed over the ranks, on every rank (one all-reduce: RCCL reduces device tensors, gloo host tensors)"""
    import torch.distributed as dist
    acc = torch.from_numpy(vec)
    acc = acc.to(device) if dist.get_backend() == 'nccl' else acc
    dist.all_reduce(acc, op=dist.ReduceOp.SUM)
    return acc.cpu().numpy()


def evaluate_scenario(umat_dev, vmat, bmat, uids, vids, data_dir, fold, scenario, step, total, device, umap=None):
    """accuracy@(step, 2*step, ...) of one scenario (evaluate.py:72-112).  Under torch.distributed every rank ranks its
    block of the scenario's test lines; what the reference accumulates over users -- tresults[k] and tcount, :106-112 --
    is summed over the ranks by one all-reduce of interval + 1 integers (no other exchange: the factors are replicated)."""
    full = load_scenario(data_dir, fold, scenario, uids, umap)
    return evaluate_loaded(umat_dev, vmat, bmat, vids, full, step, total, device)


def evaluate_loaded(umat_dev, vmat, bmat, vids, full, step, total, device):
    """the ranking + counting half of evaluate_scenario on an already parsed Scenario (the same on every rank)"""
    return accuracy_loaded(Ranker(umat_dev, (vmat, bmat, vids), Lines(_shard(full)[0], device)), step, total)


def accuracy_loaded(ops, step, total):
    """evaluate_loaded on a Ranker over this rank's shard: K4, K5 and the all-reduce"""
    sc = ops.lines.sc
    interval = total // step
    hits, tcount = np.zeros(interval, dtype=np.int64), sc.tcount
    if len(sc.users):
        hits = ops.count_hits(ops.score_topk(total), step, interval).cpu().numpy()
    if _world()[1] > 1:
        acc = _sum_over_ranks(np.r_[hits, tcount].astype(np.int64), ops.lines.device)
        hits, tcount = acc[:interval], int(acc[interval])
    return [float(h) / tcount for h in hits]                          # ZeroDivisionError like evaluate.py:112


def like_ranks_loaded(umat_dev, vmat, bmat, vids, sc, device):
    """K8 on an already parsed Scenario with at least one line -> the filtered rank of every liked column, int32 [n_likes] (device)"""
    return Ranker(umat_dev, (vmat, bmat, vids), Lines(sc, device)).like_ranks()


def rank_metrics_loaded(ops, step, total, metrics, keep=None):
    """{metric: list of values} (rankmetrics.py) from one full-rank pass of a Ranker over this rank's shard: K8 gives the filtered rank
    of every liked column of the shard's test lines, the metric sums and counts are all-reduced like the hits of accuracy_loaded (one
    fp64 vector; the same on every rank afterwards).  keep: a dict that receives K8's output, still on the device, as 'ranks' (None
    without a test line)."""
    sc = ops.lines.sc
    ranks, ranks_dev = np.zeros(0, dtype=np.int32), None
    if len(sc.users):
        ranks_dev = ops.like_ranks()
        ranks = ranks_dev.cpu().numpy()
    if keep is not None:
        keep['ranks'] = ranks_dev
    sums = rankmetrics.rank_sums(ranks, sc.like_ptr, sc.rated_ptr, len(sc.teids), step, total)
    if _world()[1] > 1:
        sums = rankmetrics.from_vector(_sum_over_ranks(rankmetrics.to_vector(sums), ops.lines.device), total // step)
    return rankmetrics.finish(sums, metrics)


def significance_loaded(ranks_dev, lines, other, step, total, metrics, boot):
    """the bootstrap figures of a scenario's Lines (single process) -> significance.report's dict.  ranks_dev: K8's ranks of the model
    under evaluation (device); other: the Ranker of --compare's model on the same Lines, or None; boot: dict(R, seed, level).
    The line tables of both models are built, joined and resampled on the device (K18); only the column sums come down"""
    if ranks_dev is None:
        raise ZeroDivisionError('--bootstrap: no test line to resample')
    n_cols = len(lines.sc.teids)
    X = significance.line_table(ranks_dev, lines.like_ptr, lines.rated_ptr, n_cols, step, total)
    if other is not None:
        X = torch.cat([X, significance.line_table(other.like_ranks(), lines.like_ptr, lines.rated_ptr, n_cols, step, total)], dim=1).contiguous()
    reps = significance.bootstrap_sums(X, boot['R'], boot['seed']).cpu().numpy()
    return significance.report(X.sum(dim=0).cpu().numpy(), reps, total // step, metrics, boot['level'], 2 if other is not None else 1)


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


def negative_metrics_loaded(ops, full, step, total, n_neg, seed, metrics):
    """{metric: list of values} of hr / ndcg / mrr of a Ranker's model against sampled negatives.  The rows are drawn for the whole
    Scenario `full` on every rank (a host function of the seed: the same rows whatever the number of ranks); a rank scores the rows of
    its block of test lines -- the block shard_scenario gives it -- with K12, and the sums are all-reduced like those of
    rank_metrics_loaded."""
    rank, world = _world()
    device = ops.lines.device
    line, cand_ptr, cand_cols, like_at = negative_rows(full, n_neg, seed)
    lo, hi = _block(len(full.users), rank, world)
    q0, q1 = int(np.searchsorted(line, lo)), int(np.searchsorted(line, hi))
    like_ranks = np.zeros(0, dtype=np.int32)
    if q1 > q0:
        user_idx = torch.from_numpy(full.users[line[q0:q1]].astype(np.int32)).to(device)
        ptr = cand_ptr[q0:q1 + 1] - cand_ptr[q0]
        cols = cand_cols[cand_ptr[q0]:cand_ptr[q1]]
        _, ranks = tkr_hip.rank_candidates(ops.umat, ops.items.Vt, torch.from_numpy(ptr).to(device), torch.from_numpy(cols).to(device),
                                           bias=ops.items.bias, user_idx=user_idx)
        like_ranks = ranks.cpu().numpy()[like_at[q0:q1] - cand_ptr[q0]]
    sums = rankmetrics.negative_sums(like_ranks, step, total)
    if world > 1:
        sums = rankmetrics.neg_from_vector(_sum_over_ranks(rankmetrics.neg_to_vector(sums), device), total // step)
    return rankmetrics.finish(sums, metrics)


def list_metrics_loaded(ops, step, total, metrics, div, anchors=None):
    """the list metrics of a Ranker over a whole Scenario (single process) -> (plain, mmr): {metric: values at step, 2 step, ...} of the
    ordinary top-`total` lists for the `metrics` of diversity.LIST_METRICS, and -- with div, the arguments of --diversify -- the same of
    the lists K17 re-ranks out of the div['pool'] best, plus 'acc': K5's hit count on them as accuracy_loaded reports it (else None).
    anchors: (ptr, cols) on the device, the training likes of every test line's user in the `vid` numbering -- both dicts then also
    hold 'unexp', the unexpectedness of the lists against them (K19, explain.list_unexpectedness): the similarity table is the whole
    final-V.dat's, and the lists' test columns are mapped to its rows first"""
    sc, device = ops.lines.sc, ops.lines.device
    interval = total // step
    grid = [step * (q + 1) for q in range(interval)]
    plain = {m: [0.0] * interval for m in list(metrics) + (['unexp'] if anchors is not None else [])}
    mmr = dict(plain, acc=[0.0] * interval) if div else None
    if not len(sc.users):
        return plain, mmr
    unexp = None
    if anchors is not None:
        te_rows = torch.from_numpy(ops.items.te_rows.astype(np.int32)).to(device)
        S_full = diversity.similarity_table(torch.from_numpy(ops.model[0]).to(device), div['similarity'] if div else 'cosine')

        def unexp(lists):
            as_vid = torch.where(lists >= 0, te_rows[lists.clamp(min=0).long()], torch.full_like(lists, -1)).contiguous()
            return explain.list_unexpectedness(S_full, as_vid, anchors[0], anchors[1], grid)
    S = diversity.similarity_table(ops.items.Vt, div['similarity'] if div else 'cosine')
    n_cols = len(sc.teids)
    ids, scores = ops.score_topk(div['pool'] if div else total, want_scores=True)
    if metrics:
        every = diversity.list_metrics(S, ids[:, :total].contiguous(), n_cols, grid)
        plain = {m: every[m] for m in metrics}
    if unexp:
        plain['unexp'] = unexp(ids[:, :total])
    if div:
        picked, _ = diversity.rerank(S, diversity.relevance(ids, scores), ids, scores, div['diversify'], total)
        hits = ops.count_hits(picked, step, interval).cpu().numpy()
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
    is_knn = {path: knn.is_model_dir(path) for path in (args.model, args.compare)}
    for path in (p for p in (args.model, args.compare) if is_knn[p]):
        knn_refusals(parser, args, path)
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
    umap = textio.IdMap(uids)
    liked_csr = None
    if any(is_knn.values()):                                         # a line's history: its user's like == 1 entries of the train file
        n_users = max(int(max(uids.values())) + 1 if uids else 0, 1)
        liked_csr = foldin.liked_csr(textio.parse_ratings(os.path.join(args.data, 'f%dtr.txt' % args.fold), umap, textio.IdMap(vids)),
                                     n_users, max(vids.values()) + 1)

    def ranker_of(path):
        """lines -> the Ranker of a model directory: a neighbourhood model where it holds knn.npz, else final-U.dat / final-V.dat"""
        if is_knn[path]:
            model = knn.load(path)
            return lambda lines: KnnRanker(model, liked_csr, vids, lines)
        umat, vmat, bmat = read_model(path, uids, vids)
        umat_dev = torch.from_numpy(umat).to(device)
        return lambda lines: Ranker(umat_dev, (vmat, bmat, vids), lines)

    ranker_a = ranker_of(args.model)
    ranker_b = ranker_of(args.compare) if args.compare is not None else None      # model B: the same uid / vid lists
    results, extra, negs, lists, boots = {}, {}, {}, {}, {}
    liked = textio.parse_ratings(os.path.join(args.data, 'f%dtr.txt' % args.fold), umap, textio.IdMap(vids)) if unexp else None

    def rank_entry(scenario):
        """the accuracy of one entry of -sl, and its other figures when the scenario is named for the first time.  One set of operands
        serves all of them; it is released on return, so the next entry is loaded into the device memory this one leaves"""
        full = load_scenario(args.data, args.fold, scenario, uids, umap)
        ops = ranker_a(Lines(_shard(full)[0], device))
        acc = accuracy_loaded(ops, args.step, args.total)
        if (args.metrics or div) and scenario not in extra:          # (a scenario listed twice: its metric lines are not doubled)
            kept = {} if boot else None
            extra[scenario] = rank_metrics_loaded(ops, args.step, args.total, full_metrics, kept)
            if boot:
                other = ranker_b(ops.lines) if ranker_b is not None else None
                boots[scenario] = significance_loaded(kept['ranks'], ops.lines, other, args.step, args.total, full_metrics, boot)
            if neg_metrics:
                negs[scenario] = negative_metrics_loaded(ops, full, args.step, args.total, args.negatives, args.neg_seed, neg_metrics)
            if list_metrics or div or unexp:
                anchors = explain.anchors_csr([liked], full.users, len(ops.model[0]), device) if unexp else None
                lists[scenario] = list_metrics_loaded(ops, args.step, args.total, list_metrics, div, anchors)
        return acc

    for scenario in args.scenarios:
        acc = rank_entry(scenario)
        if scenario not in results:                                  # evaluate.py:109-112 ACCUMULATES per scenario name: a scenario
            results[scenario] = [0.0] * len(acc)                     # listed twice ("-sl im im") prints doubled values, twice
        for k, v in enumerate(acc):
            results[scenario][k] += v
    lines = []

    def report(name, values, every_rank=False):
        lines.append(name + ''.join(',%.6f' % v for v in values))
        if rank == 0 or every_rank:                                  # one report, like the single process
            print(lines[-1])

    for scenario in args.scenarios:
        report(scenario, results[scenario])
    for scenario in args.scenarios if args.metrics else ():
        for m in full_metrics:
            report('%s.%s' % (scenario, m), extra[scenario][m])
    for scenario in args.scenarios if neg_metrics else ():
        for m in neg_metrics:
            report('%s.neg%d.%s' % (scenario, args.negatives, m), negs[scenario][m])
    list_names = list_metrics + (['unexp'] if unexp else [])         # (from here on a single process: refused above otherwise)
    for which, names in ((0, list_names), (1, (['acc'] + list_names) if div else [])):
        for scenario in args.scenarios if names else ():
            for m in names:
                report('%s.%s%s' % (scenario, 'mmr.' if which else '', m), lists[scenario][which][m], every_rank=True)
    named = [('%s.lo', 'lo'), ('%s.hi', 'hi')]                       # (the line's name after 'S.', significance.report's key)
    if args.compare is not None:
        named += [('vs.%s', 'vs'), ('diff.%s', 'diff'), ('diff.%s.lo', 'diff.lo'), ('diff.%s.hi', 'diff.hi'), ('diff.%s.p', 'diff.p')]
    for scenario in args.scenarios if boot else ():
        for m in full_metrics:
            for name, key in named:
                report('%s.%s' % (scenario, name % m), boots[scenario][m][key], every_rank=True)
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
