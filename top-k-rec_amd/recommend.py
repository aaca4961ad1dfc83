"""recommend.py -- write every user's top-k items and their scores, scored on MI355X; new users are folded in first.

    python recommend.py -d DATA -m MODEL -f 0 -t 30 -o out.txt [-u USERS_FILE | --candidates FILE]
                        [--new-uid FILE --new-history FILE --fold-steps 50 --fold-triplets 16 --fold-lr 0.05 --fold-lu 2.5e-3 --seed 0]
                        [--new-vid FILE --new-ratings FILE --fold-li 2.5e-3 --fold-lj 2.5e-4 --fold-lb 0]
                        [--diversify LAMBDA --pool 100 --similarity cosine|dot]
                        [--explain E --explain-output FILE --similarity cosine|dot]

Inputs as evaluate.py: ``DATA/uid``, ``DATA/vid``, ``DATA/f{fold}tr.txt`` (the histories), ``MODEL/final-U.dat``, ``final-V.dat``,
optional ``final-B.dat``.  For every requested user -- the tokens of USERS_FILE, one per line; default: every line of ``uid`` -- the
``-t`` best items of the whole ``vid`` catalogue, every item on the user's history line excluded whatever its like value (the
``rated`` set of evaluate.py:30-45; a user without a line excludes nothing).  One output line per user in the ratings layout,

    uid,iid:%f,iid:%f,...

best first, ties in K4's order (higher catalogue index first); fewer than ``-t`` fields when the user has fewer unrated items.

``--new-uid`` / ``--new-history`` (both or neither): the users of that id file are not in the model; their vectors are folded in
from the like == 1 entries of their lines in the history file (K9, foldin.py) and ranked the same way, their own history file
supplying the excluded items; their lines follow the model users' lines.  With ``--new-uid`` and no ``-u``, ``-u`` defaults to every
model user as usual; an empty USERS_FILE writes the new users only.

``--new-vid`` / ``--new-ratings`` (both or neither): the items of that id file are not in the model; their rows (and biases, when the
model has ``final-B.dat``) are folded in from the like == 1 entries of the model's users in the ratings file (K10,
foldin.fold_in_items: the users' training positives are the like == 1 entries of ``f{fold}tr.txt``), appended to the catalogue in
file order and ranked with it under their own tokens; what a user rated in that file is excluded for that user like the history
line.  Together with ``--new-uid`` the items go first and the users are folded in against the grown catalogue.

``--candidates FILE`` (not with ``-u``): re-rank shortlists instead of the catalogue.  FILE is in the ratings layout,
``uid,iid:like,...``; every known item on a line is a candidate of that line's user whatever its like value, unknown items are dropped
as in the history, an item listed twice counts once.  Every line gives one output line in the format above -- the ``-t`` best of ITS
candidates, the history excluded as always; a user may appear on several lines.  The lines of the model's users come first, in file
order, then those of the ``--new-uid`` users; a uid that is in neither id list raises KeyError.  After ``--new-vid`` the candidates are
looked up in the grown catalogue.  Scores and order are those the full ranking gives the same items (K12, tkr_hip.rank_candidates).

``--diversify LAMBDA`` (0 <= LAMBDA <= 1): every line is re-ranked by greedy Maximal Marginal Relevance (K17, diversity.py).  The
``--pool`` best items of the line (default max(100, -t); at most 1024) are ranked as above, their scores scaled onto [0, 1] per line, and
``-t`` of them are picked one by one, each time the item with the largest  LAMBDA * relevance - (1 - LAMBDA) * (its largest similarity to
an item already picked);  ``--similarity``: the cosine (default) or the dot product of the item factors.  The format is unchanged and
the scores are the model's own, so they are no longer monotone along a line.  LAMBDA = 1 writes the file written without the flag.
It applies to every kind of line: model users, ``--new-uid``, ``--new-vid`` and ``--candidates``.

``--explain E --explain-output FILE`` (both or neither, 1 <= E <= 8): FILE gets one line per output line, in the same order,

    uid,iid:aid:%f:aid:%f,iid:aid:%f,...

one comma field per recommended item in list order: the item's token, then up to E (anchor token, similarity) pairs, best first -- the
user's own liked items whose factors are most similar to the item's (K19, explain.py; ``--similarity`` as above, default cosine, on the
catalogue the lists were ranked against).  The anchors of a line are the like == 1 entries of exactly the sources whose items the
line excludes: the user's last line of ``f{fold}tr.txt``, with ``--new-vid`` also of ``--new-ratings``, for ``--new-uid`` users
``--new-history``.  An item never explains itself; an item without an anchor is its bare token.  With ``--diversify`` the final lists
are explained.  The main output is byte for byte what it is without the two flags.

A MODEL that holds ``knn.npz`` is a neighbourhood model (knn.ItemKNN, K28 / K29): model users are ranked from their like == 1 entries
of ``f{fold}tr.txt``, ``--new-uid`` users from those of ``--new-history`` with no fold-in step (the ``--fold-*`` flags mean nothing
there); the excluded items, the output format and the writers are the same.  ``--candidates``, ``--new-vid``, ``--diversify`` and
``--explain`` need item factors and end in a parser error.

The scores, the filter and the selection run on the GPU (tkr_hip.build_rated_mask, tkr_hip.score_topk); single process.
"""
from __future__ import annotations

import argparse
import os

import numpy as np
import torch

import diversity
import explain as expl
import foldin
import knn
import textio
import tkr_hip
from evaluate import _group, _take_rows, read_ids, read_matrix, read_model     # noqa: F401  (read_matrix: tests/test_gpu_item_foldin.py reads through it)
from textio import format_lines      # noqa: F401  (the host formatter of the output lines; textio.write_lists writes them)


def row_tokens(users):
    """the uid tokens of the ranked rows (a user may be asked for twice) -> (IdMap of the distinct tokens, its index per row): the
    table textio.write_lists prints the rows' uids from"""
    table = {}
    rows = np.fromiter((table.setdefault(u, len(table)) for u in users), dtype=np.int32, count=len(users))
    return textio.IdMap(table), rows


def read_user_list(path, uids):
    """the requested users: one known uid token per line -> tokens in file order"""
    with open(path) as fh:
        users = [ln.strip() for ln in fh if ln.strip()]
    for u in users:
        if u not in uids:
            raise KeyError('%s: user %r is not in the uid list' % (path, u))
    return users


def rated_csr(R, rows_of_user, n_rows, n_items):
    """the excluded items of every ranked row: all known items on the LAST line of its user in the parsed ratings file R
    (evaluate.py:34: rated[uid] = set() per line).  rows_of_user: user index -> list of ranked rows (a user may be asked for twice)"""
    last = {}
    for line in np.flatnonzero(R.line_user >= 0):
        last[int(R.line_user[line])] = int(line)
    rr, cc = [], []
    for user, line in last.items():
        cols = R.item[R.line_ptr[line]:R.line_ptr[line + 1]]
        cols = cols[cols >= 0]
        for row in rows_of_user.get(user, ()):
            rr.append(np.full(len(cols), row, dtype=np.int64))
            cc.append(cols.astype(np.int64))
    if not rr:
        return np.zeros(n_rows + 1, dtype=np.int64), np.zeros(0, dtype=np.int32)
    return _group(np.concatenate(rr), np.concatenate(cc), n_rows, n_items)


def _rated_csr_device(sources, user_rows, n_items, dev):
    """rated_csr (and the union over a second file) by K15 -> (ptr, cols) on the device.  sources: parsed ratings files"""
    n = len(user_rows)
    rows = torch.from_numpy(np.asarray(user_rows, dtype=np.int64)).to(dev)
    n_users = int(max(user_rows)) + 1 if n else 0
    segs = []
    for R in sources:
        Rd = textio.ratings_to_device(R, dev)
        last = tkr_hip.last_line_of_user(Rd.line_user, n_users)      # a user without a line: -1, excludes nothing
        segs.append((Rd.line_ptr, Rd.item, None, last[rows].contiguous()))
    textio.group_fits(4 * sum(int(s[1].numel()) for s in segs) + 8 * n + 64, dev, 'the excluded items')
    return tkr_hip.group_segments(segs, n, max(n_items, 1))


def candidate_lines(path, umap, vmap, n_items, where=None):
    """the lines of the candidates file whose uid `umap` knows -> (known: bool per line of the file, the user index of each known line,
    and the CSR of their known items: ascending, unique).  where / TKR_GROUP: which code groups them (textio.group_on_device)"""
    where = textio._group_where(where)
    Cf = textio.parse_ratings(path, umap, vmap)
    if textio.group_on_device(where, len(Cf.item), max(n_items, 1)):
        try:
            dev = torch.device('cuda', torch.cuda.current_device())
            Cd = textio.ratings_to_device(Cf, dev)
            lines = torch.nonzero(Cd.line_user >= 0).reshape(-1)
            ptr, cols = tkr_hip.group_segments([(Cd.line_ptr, Cd.item, None, lines)], int(lines.numel()), max(n_items, 1))
            textio.group_counts['device'] += 1
            return Cf.line_user >= 0, Cd.line_user[lines].to(torch.int64).cpu().numpy(), ptr.cpu().numpy(), cols.cpu().numpy()
        except textio.DeviceGroupTooLarge:
            if where == 'device':
                raise
    textio.group_counts['host'] += 1
    lines = np.flatnonzero(Cf.line_user >= 0)
    row_of_line = np.full(len(Cf.line_user), -1, dtype=np.int64)
    row_of_line[lines] = np.arange(len(lines))
    keep = (Cf.item >= 0) & (row_of_line[Cf.entry_line] >= 0)
    ptr, cols = _group(row_of_line[Cf.entry_line[keep]], Cf.item[keep].astype(np.int64), len(lines), max(n_items, 1))
    return Cf.line_user >= 0, Cf.line_user[lines].astype(np.int64), ptr, cols


def rank(U_dev, user_rows, V_dev, bias_dev, R, total, also_rated=None, candidates=None, on_device=False, where=None, diversify=None,
         pool=None, similarity='cosine', explain=None):
    """top-`total` unrated items of the users `user_rows` (indices into U_dev and into R's user numbering); `also_rated`: a second
    parsed ratings file in the same numbering whose lines exclude items too; `candidates`: (ptr, cols), a CSR over the ranked rows --
    then only these items of a row are ranked (K12) instead of the catalogue (K4)
    -> (ids int32 [n, total], scores fp32 [n, total]) as numpy, with on_device=True as tensors left on the GPU.  where / TKR_GROUP:
    which code builds the excluded-items CSR (textio.group_on_device); on the device it goes to the mask without a download.
    diversify: a lambda in [0, 1] -- the `pool` best (default diversity.default_pool(total)) are ranked instead and `total` of them
    picked by greedy MMR under `similarity` (K17, diversity.rerank); the scores stay the model's own, in pick order.
    explain: a number of anchors E -- a third value is returned, (cols int32 [n, total, E], sims fp32 [n, total, E]): for every entry of
    the final lists the E like == 1 items of the row's user in R (and also_rated) that are most similar to it under `similarity`, -1 /
    -inf padded (K19, explain.explain)"""
    where = textio._group_where(where)
    want = total
    if diversify is not None:
        total = diversity.default_pool(want) if pool is None else int(pool)
        if not want <= total <= tkr_hip.MMR_MAX_POOL:
            raise ValueError('rank: the pool must hold between total = %d and %d entries, got %d' % (want, tkr_hip.MMR_MAX_POOL, total))
    n, n_items = len(user_rows), int(V_dev.shape[0])
    dev = V_dev.device
    sources = [R] if also_rated is None else [R, also_rated]
    ptr_dev = None
    if n and textio.group_on_device(where, sum(textio.n_entries_of(S) for S in sources), n_items):
        try:
            ptr_dev, cols_dev = _rated_csr_device(sources, user_rows, n_items, dev)
            textio.group_counts['device'] += 1
        except textio.DeviceGroupTooLarge:
            if where == 'device':
                raise
    if ptr_dev is None:
        textio.group_counts['host'] += 1
        rows_of_user = {}
        for row, user in enumerate(user_rows):
            rows_of_user.setdefault(int(user), []).append(row)
        R, also_rated = textio.ratings_to_host(R), None if also_rated is None else textio.ratings_to_host(also_rated)
        ptr, cols = rated_csr(R, rows_of_user, n, n_items)
        if also_rated is not None:
            ptr2, cols2 = rated_csr(also_rated, rows_of_user, n, n_items)
            rows = np.concatenate([np.repeat(np.arange(n), np.diff(ptr)), np.repeat(np.arange(n), np.diff(ptr2))])
            ptr, cols = _group(rows, np.concatenate([cols, cols2]).astype(np.int64), n, n_items)
        ptr_dev, cols_dev = torch.from_numpy(ptr).to(dev), torch.from_numpy(cols).to(dev)
    mask, pitch = tkr_hip.build_rated_mask(ptr_dev, cols_dev, n, n_items)
    idx = torch.from_numpy(np.asarray(user_rows, dtype=np.int32)).to(dev)
    if candidates is not None:
        cptr, ccols = torch.from_numpy(candidates[0]).to(dev), torch.from_numpy(candidates[1]).to(dev)
        s, r = tkr_hip.rank_candidates(U_dev, V_dev, cptr, ccols, bias=bias_dev, user_idx=idx, mask=mask, mask_pitch=pitch)
        ids, scores = tkr_hip.topk_from_ranks(cptr, ccols, s, r, total)
    else:
        ids, scores = tkr_hip.score_topk(U_dev, V_dev, total, bias=bias_dev, user_idx=idx, mask=mask, mask_pitch=pitch, want_scores=True)
    S = None
    if diversify is not None:
        S, rel = diversity.prepare(V_dev, ids, scores, similarity)
        ids, scores = diversity.rerank(S, rel, ids, scores, diversify, want)
    if explain is not None:
        S = diversity.similarity_table(V_dev, similarity) if S is None else S
        aptr, acols = expl.anchors_csr(sources, user_rows, n_items, dev, where)
        why = expl.explain(S, ids, aptr, acols, explain)
        if on_device:
            return ids, scores, why
        return ids.cpu().numpy(), scores.cpu().numpy(), tuple(x.cpu().numpy() for x in why)
    if on_device:
        return ids, scores
    return ids.cpu().numpy(), scores.cpu().numpy()


def fold_in_new_items(args, uids, vids, new_vids, umat, vmat, bmat, device):
    """-> (vmat, bmat, vids) grown by the items of `new_vids` in file order, their rows folded in (K10) from the model users' likes in
    args.new_ratings against final-U.dat (`umat`) and the users' positives in the fold's train file, and that ratings file parsed over
    the grown catalogue"""
    n_users, n_items, m = len(uids), len(vmat), max(new_vids.values()) + 1
    umap = textio.IdMap(uids)
    user_pos = foldin.liked_csr(textio.parse_ratings(os.path.join(args.data, 'f%dtr.txt' % args.fold), umap, textio.IdMap(vids)), n_users, n_items)
    likers = foldin.liked_csr(textio.parse_ratings(args.new_ratings, umap, textio.IdMap(new_vids)), m, n_users, by='item')
    V_new, b_new = foldin.fold_in_items(umat, vmat, bmat, user_pos, likers, li=args.fold_li, lj=args.fold_lj, lb=args.fold_lb, lr=args.fold_lr,
                                        steps=args.fold_steps, triplets=args.fold_triplets, seed=args.seed, device=device)
    grown = dict(vids)
    for tok, idx in new_vids.items():
        grown[tok] = n_items + idx
    vmat = np.concatenate([vmat, V_new])
    if bmat is not None:
        bmat = np.concatenate([bmat, b_new.reshape(-1)])
    return vmat, bmat, grown, textio.parse_ratings(args.new_ratings, umap, textio.IdMap(grown))


def rank_knn(model, liked, user_rows, R, total, device):
    """rank() for a neighbourhood model (knn.ItemKNN): the history of a ranked row is its user's row of `liked`, the (ptr, cols) CSR of
    the like == 1 entries of R by user index; every known item on the user's last line of R is excluded, as rank() excludes it
    -> (ids int32 [n, total], scores fp32 [n, total]) on the device (K29, tkr_hip.knn_score)"""
    n = len(user_rows)
    rows_of_user = {}
    for row, user in enumerate(user_rows):
        rows_of_user.setdefault(int(user), []).append(row)
    ptr, cols = rated_csr(textio.ratings_to_host(R), rows_of_user, n, model.n_items)
    mask, pitch = tkr_hip.build_rated_mask(torch.from_numpy(ptr).to(device), torch.from_numpy(cols).to(device), n, model.n_items)
    hptr, hcols = _take_rows(liked[0], liked[1], np.asarray(user_rows, dtype=np.int64))
    return tkr_hip.knn_score(torch.from_numpy(hptr).to(device), torch.from_numpy(np.ascontiguousarray(hcols)).to(device), *model.table(device),
                             total, mask=mask, mask_pitch=pitch, want_scores=True)


def main_knn(parser, args, uids, vids, users, new_uids):
    """main() for a model directory that holds knn.npz: model users are ranked from their like == 1 entries of the train file, the
    --new-uid users from those of --new-history, with no fold-in step (the --fold-* flags mean nothing here).  Same output, same writers"""
    for flag, given in (('--candidates', args.candidates), ('--new-vid', args.new_vid), ('--diversify', args.diversify), ('--explain', args.explain)):
        if given is not None:
            parser.error('%s is not available for a neighbourhood model (%s holds knn.npz): it has no item factors' % (flag, args.model))
    if not torch.cuda.is_available():
        raise tkr_hip.TkrError('recommend.py scores on the GPU through libtkr_hip.so; no MI355X is visible')
    device = torch.device('cuda', torch.cuda.current_device())
    model = knn.load(args.model)
    n_items = max(vids.values()) + 1
    if model.n_items != n_items:
        raise ValueError('%s holds %d items, the vid list %d' % (args.model, model.n_items, n_items))
    vmap = textio.IdMap(vids)
    wrote = False
    for tokens_of, table, path in ((users, uids, os.path.join(args.data, 'f%dtr.txt' % args.fold)), (list(new_uids), new_uids, args.new_history)):
        if not tokens_of:
            continue
        R = textio.parse_ratings(path, textio.IdMap(table), vmap)
        liked = foldin.liked_csr(R, max(table.values()) + 1, n_items)
        ids, scores = rank_knn(model, liked, [table[u] for u in tokens_of], R, args.total, device)
        tokens, rows = row_tokens(tokens_of)
        textio.write_lists(args.output, tokens, ids, scores, rows, vmap, where=args.format, append=wrote)
        wrote = True
    if not wrote:
        open(args.output, 'wb').close()
    with open(args.output, 'rb') as fh:
        return fh.read().decode().split('\n')[:-1]


def main(argv=None):
    parser = argparse.ArgumentParser(description="Write the top-k items of every user, scored on the GPU.")
    parser.add_argument('-d', '--data', required=True, help="The data path (uid, vid, f{fold}tr.txt)")
    parser.add_argument('-m', '--model', required=True, help="The work path for the model")
    parser.add_argument('-f', '--fold', type=int, default=0, help="The index of the fold whose train file holds the histories")
    parser.add_argument('-t', '--total', type=int, default=30, help="The number of items per user")
    parser.add_argument('-o', '--output', required=True, help="The file the lines are written to")
    parser.add_argument('-u', '--users', default=None, help="A file of uid tokens, one per line (default: every user of uid)")
    parser.add_argument('--candidates', default=None, help="A ratings-layout file of shortlists: every line is re-ranked on its own (not with -u)")
    parser.add_argument('--new-uid', default=None, help="An id file of users that are not in the model: folded in, then ranked")
    parser.add_argument('--new-history', default=None, help="The ratings file of the new users")
    parser.add_argument('--fold-steps', type=int, default=50)
    parser.add_argument('--fold-triplets', type=int, default=16)
    parser.add_argument('--fold-lr', type=float, default=0.05)
    parser.add_argument('--fold-lu', type=float, default=2.5e-3)
    parser.add_argument('--new-vid', default=None, help="An id file of items that are not in the model: folded in, then ranked with the rest")
    parser.add_argument('--new-ratings', default=None, help="The ratings file that holds the model users' likes of the new items")
    parser.add_argument('--fold-li', type=float, default=2.5e-3)
    parser.add_argument('--fold-lj', type=float, default=2.5e-4)
    parser.add_argument('--fold-lb', type=float, default=0.0)
    parser.add_argument('--seed', type=int, default=0)
    diversity.add_arguments(parser)
    expl.add_arguments(parser)
    parser.add_argument('--format', default=None, choices=textio.FORMAT_WHERE,
                        help="Where the output lines are formatted (default: TKR_FORMAT, else auto: on the GPU from TKR_FORMAT_DEVICE_FROM list entries upward)")
    parser.add_argument('--group', default=None, choices=textio.GROUP_WHERE,
                        help="Where the excluded items and the candidates are grouped into rows (default: TKR_GROUP, else auto: on the GPU from TKR_GROUP_DEVICE_FROM parsed entries upward)")
    args = parser.parse_args(argv)
    if (args.new_uid is None) != (args.new_history is None):
        parser.error('--new-uid and --new-history go together')
    if (args.new_vid is None) != (args.new_ratings is None):
        parser.error('--new-vid and --new-ratings go together')
    if args.total < 1:
        parser.error('-t must be at least 1')
    if args.candidates is not None and args.users is not None:
        parser.error('--candidates names its users line by line: it does not go with -u')
    div = dict(diversity.check_arguments(parser, args), **expl.check_arguments(parser, args))
    why_path = args.explain_output

    uids = read_ids(os.path.join(args.data, 'uid'))
    vids = read_ids(os.path.join(args.data, 'vid'))
    users = list(uids) if args.users is None else read_user_list(args.users, uids)
    new_uids = {}
    if args.new_uid is not None:
        new_uids = read_ids(args.new_uid)
        clash = [u for u in new_uids if u in uids]
        if clash:
            raise KeyError('%s: user %r is in the model already' % (args.new_uid, clash[0]))
    new_vids = {}
    if args.new_vid is not None:
        new_vids = read_ids(args.new_vid)
        clash = [v for v in new_vids if v in vids]
        if clash:
            raise KeyError('%s: item %r is in the model already' % (args.new_vid, clash[0]))
    if knn.is_model_dir(args.model):
        return main_knn(parser, args, uids, vids, users, new_uids)
    if not torch.cuda.is_available():
        raise tkr_hip.TkrError('recommend.py scores on the GPU through libtkr_hip.so; no MI355X is visible')
    device = torch.device('cuda', torch.cuda.current_device())

    _, vmat, bmat = read_model(args.model, vids=vids)
    bmat = None if bmat is None else bmat.reshape(-1)
    umat = R_new_items = None                                       # final-U.dat is read once, and only when something needs it
    if new_vids:
        umat = read_model(args.model, uids=uids)[0]
        vmat, bmat, vids, R_new_items = fold_in_new_items(args, uids, vids, new_vids, umat, vmat, bmat, device)
    V_dev = torch.from_numpy(vmat).to(device)
    bias_dev = None if bmat is None else torch.from_numpy(np.ascontiguousarray(bmat)).to(device)
    vmap = textio.IdMap(vids)
    wrote = False                                                   # one output file: the model users' lines, then the new users'
    cand_model = cand_new = None
    if args.candidates is not None:
        cand_model = candidate_lines(args.candidates, textio.IdMap(uids), vmap, len(vmat), where=args.group)
        cand_new = candidate_lines(args.candidates, textio.IdMap(new_uids), vmap, len(vmat), where=args.group) if new_uids else None
        stray = np.flatnonzero(~(cand_model[0] | cand_new[0]) if cand_new else ~cand_model[0])
        if len(stray):
            with open(args.candidates) as fh:
                tokens = [ln.split(',')[0].strip() for ln in fh]
            who = repr(tokens[stray[0]]) if len(tokens) == len(cand_model[0]) else 'on line %d' % (stray[0] + 1)
            raise KeyError('%s: user %s is neither in the uid list nor a new user' % (args.candidates, who))
        tok = {idx: t for t, idx in uids.items()}
        users = [tok[int(x)] for x in cand_model[1]]
    if users:
        umat = read_model(args.model, uids=uids)[0] if umat is None else umat
        R = textio.parse_ratings(os.path.join(args.data, 'f%dtr.txt' % args.fold), textio.IdMap(uids), vmap)
        ids, scores, *why = rank(torch.from_numpy(umat).to(device), [uids[u] for u in users], V_dev, bias_dev, R, args.total, also_rated=R_new_items,
                                 candidates=cand_model[2:] if cand_model else None, on_device=True, where=args.group, **div)
        tokens, rows = row_tokens(users)
        textio.write_lists(args.output, tokens, ids, scores, rows, vmap, where=args.format)
        if why:
            expl.write_lines(why_path, tokens, ids, *why[0], rows, vmap)
        wrote = True
    if new_uids:
        m = max(new_uids.values()) + 1
        R = textio.parse_ratings(args.new_history, textio.IdMap(new_uids), vmap)
        hist = foldin.liked_csr(R, m, len(vmat))
        U_new = foldin.fold_in(vmat, bmat, hist, lu=args.fold_lu, lr=args.fold_lr, steps=args.fold_steps, triplets=args.fold_triplets,
                               seed=args.seed, device=device)
        new_users = list(new_uids)
        if cand_new is not None:
            tok = {idx: t for t, idx in new_uids.items()}
            new_users = [tok[int(x)] for x in cand_new[1]]
        if new_users:
            ids, scores, *why = rank(torch.from_numpy(U_new).to(device), [new_uids[u] for u in new_users], V_dev, bias_dev, R, args.total,
                                     candidates=cand_new[2:] if cand_new else None, on_device=True, where=args.group, **div)
            tokens, rows = row_tokens(new_users)
            textio.write_lists(args.output, tokens, ids, scores, rows, vmap, where=args.format, append=wrote)
            if why:
                expl.write_lines(why_path, tokens, ids, *why[0], rows, vmap, append=wrote)
            wrote = True
    if not wrote:
        open(args.output, 'wb').close()
        if why_path is not None:
            open(why_path, 'wb').close()
    with open(args.output, 'rb') as fh:
        return fh.read().decode().split('\n')[:-1]               # the lines as written (one C-level call each, not one per line)


if __name__ == '__main__':
    main()
