"""K12 (tkr_rank_candidates, csrc/candidates.hip), tkr_hip.topk_from_ranks, recommend.py --candidates and evaluate.py --negatives on the
GPU, against tests/_candidates_oracle.py and against K4 / K8.  Scores are compared bit for bit, ranks are integers: no tolerance."""
import ctypes as C
import os
import shutil
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _candidates_oracle as O

import tkr_hip
from oracle import ref_np as R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LENGTHS = [0, 1, 63, 64, 65, 129, 500]


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to('cuda')


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _run(U, V, cands, bias=None, user_idx=None, rated=None):
    """-> (scores, ranks) as numpy, cand_ptr, cand_cols"""
    ptr, cols = O.csr(cands)
    mask, pitch = None, 0
    if rated is not None:
        rptr, rcols = O.csr(rated)
        mask, pitch = tkr_hip.build_rated_mask(_dev(rptr), _dev(rcols), len(cands), V.shape[0])
    s, r = tkr_hip.rank_candidates(_dev(U), _dev(V), _dev(ptr), _dev(cols), bias=None if bias is None else _dev(bias),
                                   user_idx=None if user_idx is None else _dev(user_idx), mask=mask, mask_pitch=pitch)
    return s.cpu().numpy(), r.cpu().numpy(), ptr, cols


@pytest.mark.parametrize('k', [1, 7, 8, 17, 50, 128, 130, 136, 264, 1000])
def test_exact_arithmetic_with_ties_matches_oracle(k):
    """factors m * 2^-6 with small integer m, biases m * 2^-12: every order of summation gives the same bits and equal scores are
    everywhere; two columns planted to tie for every user sit in every list that is long enough.  1, 3, 5 and 70 rows (70: not a
    multiple of the four waves of a workgroup) of 0, 1, 63, 64, 65, 129 and 500 candidates; with and without bias, user_idx
    (permuted, one user twice) and mask.  score_out and rank_out equal the oracle bit for bit."""
    rng = np.random.Generator(np.random.PCG64(5000 + k))
    n_cols, n_users = 600, 79
    U_all = rng.integers(-3, 4, (n_users, k)).astype(np.float32) / 64
    V = rng.integers(-3, 4, (n_cols, k)).astype(np.float32) / 64
    V[400] = V[200]                                                   # planted: columns 200 and 400 tie for EVERY user
    b = rng.integers(-2, 3, n_cols).astype(np.float32) / 4096
    b[400] = b[200]
    full = {True: R.mfma_chain_scores(U_all, V, b), False: R.mfma_chain_scores(U_all, V, None)}     # the oracle's scores, once
    plans = {1: [129], 3: [0, 65, 500], 5: [1, 63, 64, 0, 129], 70: [LENGTHS[(3 * r) % 7] for r in range(70)]}
    for n_rows, lengths in plans.items():
        cands = []
        for n in lengths:
            c = rng.choice(n_cols, n, replace=False)
            if n >= 63:
                c = np.union1d(np.setdiff1d(c, [200, 400])[:n - 2], [200, 400])
            cands.append(np.sort(c).astype(np.int32))
        rated = [np.sort(rng.choice(n_cols, int(rng.integers(0, n_cols // 2)), replace=False)).astype(np.int32) for _ in range(n_rows)]
        idx = rng.permutation(n_users)[:n_rows].astype(np.int32)
        if n_rows > 1:
            idx[-1] = idx[0]                                          # one user twice
        for with_bias, with_mask, with_idx in ((False, False, False), (True, True, True), (True, False, False), (False, True, True)):
            U = U_all if with_idx else U_all[:n_rows]
            rows = idx if with_idx else np.arange(n_rows)
            ws, wr = O.rank_candidates_np(U_all, V, b if with_bias else None, rows, cands, rated if with_mask else None, full=full[with_bias])
            gs, gr, ptr, cols = _run(U, V, cands, bias=b if with_bias else None, user_idx=idx if with_idx else None,
                                     rated=rated if with_mask else None)
            what = str((k, n_rows, with_bias, with_mask, with_idx))
            np.testing.assert_array_equal(_bits(gs), _bits(ws), err_msg=what)
            np.testing.assert_array_equal(gr, wr, err_msg=what)
            for r, c in enumerate(cands):                             # the planted tie: the higher column first
                if len(c) >= 63 and gr[ptr[r] + np.searchsorted(c, 200)] >= 0 and gr[ptr[r] + np.searchsorted(c, 400)] >= 0:
                    assert gr[ptr[r] + np.searchsorted(c, 200)] > gr[ptr[r] + np.searchsorted(c, 400)], what
            if with_mask and n_rows > 1:
                assert np.any(wr < 0) and np.any(wr >= 0)
            ids, top = tkr_hip.topk_from_ranks(_dev(ptr), _dev(cols), _dev(gs), _dev(gr), 30)
            wi, wt = O.topk_from_ranks_np(ptr, cols, ws, wr, 30)
            np.testing.assert_array_equal(ids.cpu().numpy(), wi, err_msg=what)
            np.testing.assert_array_equal(_bits(top.cpu().numpy()), _bits(wt), err_msg=what)


def _generic(seed, n_rows, n_cols, k):
    rng = np.random.Generator(np.random.PCG64(seed))
    U = np.round(rng.standard_normal((n_rows, k)) * 0.01, 6).astype(np.float32)
    V = np.round(rng.standard_normal((n_cols, k)) * 0.01, 6).astype(np.float32)
    b = np.round(rng.standard_normal(n_cols) * 0.01, 6).astype(np.float32)
    rated = [np.sort(rng.choice(n_cols, int(rng.integers(0, 60)), replace=False)).astype(np.int32) for _ in range(n_rows)]
    return rng, U, V, b, rated


@pytest.mark.parametrize('k', [50, 128, 130])
def test_whole_catalogue_lists_reproduce_score_topk(k):
    """N(0, 0.01^2) factors rounded like '%f', 300 columns, every row lists all of them: the entries of rank < 30 are K4's list, ids and
    score bits, under both arithmetic modes of K4"""
    n_rows, n_cols, K = 203, 300, 30
    rng, U, V, b, rated = _generic(900 + k, n_rows, n_cols, k)
    cands = [np.arange(n_cols, dtype=np.int32)] * n_rows
    gs, gr, ptr, cols = _run(U, V, cands, bias=b, rated=rated)
    ids, top = tkr_hip.topk_from_ranks(_dev(ptr), _dev(cols), _dev(gs), _dev(gr), K)
    rptr, rcols = O.csr(rated)
    mask, pitch = tkr_hip.build_rated_mask(_dev(rptr), _dev(rcols), n_rows, n_cols)
    try:
        for mode in ('fp32', 'refine'):
            tkr_hip.set_topk_math(mode)
            ki, ks = tkr_hip.score_topk(_dev(U), _dev(V), K, bias=_dev(b), mask=mask, mask_pitch=pitch, want_scores=True)
            np.testing.assert_array_equal(ids.cpu().numpy(), ki.cpu().numpy(), err_msg=mode)
            np.testing.assert_array_equal(_bits(top.cpu().numpy()), _bits(ks.cpu().numpy()), err_msg=mode)
    finally:
        tkr_hip.set_topk_math(tkr_hip.TOPK_MATH_DEFAULT)
    for r in range(n_rows):                                           # rated columns have no rank, the others are a permutation
        kept = gr[ptr[r]:ptr[r + 1]]
        assert np.array_equal(np.flatnonzero(kept < 0), rated[r]) and np.array_equal(np.sort(kept[kept >= 0]), np.arange(n_cols - len(rated[r])))


@pytest.mark.parametrize('k', [50, 264, 1000])
def test_whole_catalogue_lists_reproduce_like_ranks_and_sub_lists_are_consistent(k):
    """the same lists against K8 for random like sets (rated likes included: -1 on both sides); random sub-lists carry the
    whole-catalogue scores of their columns bit for bit, and their ranks are those recomputed on the host from these GPU scores"""
    n_rows, n_cols = 97, 300
    rng, U, V, b, rated = _generic(1900 + k, n_rows, n_cols, k)
    cands = [np.arange(n_cols, dtype=np.int32)] * n_rows
    gs, gr, ptr, cols = _run(U, V, cands, bias=b, rated=rated)
    likes = [np.sort(rng.choice(n_cols, int(rng.integers(0, 25)), replace=False)).astype(np.int32) for _ in range(n_rows)]
    lptr, lcols = O.csr(likes)
    rptr, rcols = O.csr(rated)
    mask, pitch = tkr_hip.build_rated_mask(_dev(rptr), _dev(rcols), n_rows, n_cols)
    lr = tkr_hip.like_ranks(_dev(U), _dev(V), _dev(lptr), _dev(lcols), bias=_dev(b), mask=mask, mask_pitch=pitch).cpu().numpy()
    line = np.repeat(np.arange(n_rows), np.diff(lptr))
    np.testing.assert_array_equal(gr.reshape(n_rows, n_cols)[line, lcols], lr)
    assert np.any(lr < 0) and np.any(lr > 0)
    full = gs.reshape(n_rows, n_cols)
    subs = [np.sort(rng.choice(n_cols, int(rng.integers(0, 140)), replace=False)).astype(np.int32) for _ in range(n_rows)]
    ss, sr, sptr, _ = _run(U, V, subs, bias=b, rated=rated)
    for r, c in enumerate(subs):
        got = ss[sptr[r]:sptr[r + 1]]
        np.testing.assert_array_equal(_bits(got), _bits(full[r][c]))
        np.testing.assert_array_equal(sr[sptr[r]:sptr[r + 1]], O.ranks_fast(got, c, np.isin(c, rated[r])))


def test_a_row_longer_than_the_resident_list_next_to_short_rows():
    """40,000 columns at k = 8: one row lists all of them, one lists TKR_CANDIDATES_RESIDENT + 1, one exactly TKR_CANDIDATES_RESIDENT
    (the longest a wave keeps), the others are short.  Exact small-integer factors: thousands of equal scores, the tie rule decides
    everywhere.  Every rank equals the oracle's, the short rows are what they are without the long ones."""
    cap = tkr_hip.CANDIDATES_RESIDENT
    rng = np.random.Generator(np.random.PCG64(41))
    n_cols, k = 40000, 8
    assert n_cols > 4 * cap
    U = rng.integers(-3, 4, (6, k)).astype(np.float32) / 64
    V = rng.integers(-3, 4, (n_cols, k)).astype(np.float32) / 64
    b = rng.integers(-2, 3, n_cols).astype(np.float32) / 4096
    lengths = [10, n_cols, 64, cap + 1, cap, 333]
    cands = [np.sort(rng.choice(n_cols, n, replace=False)).astype(np.int32) for n in lengths]
    rated = [np.sort(rng.choice(n_cols, n // 3, replace=False)).astype(np.int32) for n in lengths]
    ws, wr = O.rank_candidates_np(U, V, b, np.arange(6), cands, rated)
    gs, gr, ptr, _ = _run(U, V, cands, bias=b, rated=rated)
    np.testing.assert_array_equal(_bits(gs), _bits(ws))
    np.testing.assert_array_equal(gr, wr)
    short = [0, 2, 4, 5]
    ss, sr, sptr, _ = _run(U[short], V, [cands[r] for r in short], bias=b, rated=[rated[r] for r in short])
    for i, r in enumerate(short):
        np.testing.assert_array_equal(_bits(ss[sptr[i]:sptr[i + 1]]), _bits(gs[ptr[r]:ptr[r + 1]]))
        np.testing.assert_array_equal(sr[sptr[i]:sptr[i + 1]], gr[ptr[r]:ptr[r + 1]])


def test_two_runs_and_a_block_of_rows_alone_are_bitwise_equal():
    n_rows, n_cols, k = 150, 2000, 64
    rng, U, V, b, _ = _generic(7, n_rows, n_cols, k)
    cands = [np.sort(rng.choice(n_cols, int(rng.integers(0, 300)), replace=False)).astype(np.int32) for _ in range(n_rows)]
    cands[77] = np.arange(n_cols, dtype=np.int32)[:1500]
    a = _run(U, V, cands, bias=b)
    c = _run(U, V, cands, bias=b)
    np.testing.assert_array_equal(_bits(a[0]), _bits(c[0]))
    np.testing.assert_array_equal(a[1], c[1])
    lo, hi = 41, 103                                                  # neither end on a workgroup's first row
    part = _run(U, V, cands[lo:hi], bias=b, user_idx=np.arange(lo, hi, dtype=np.int32))
    np.testing.assert_array_equal(_bits(part[0]), _bits(a[0][a[2][lo]:a[2][hi]]))
    np.testing.assert_array_equal(part[1], a[1][a[2][lo]:a[2][hi]])


def test_wrapper_refuses_a_bad_row_pointer():
    U, V = torch.zeros((3, 8), device='cuda'), torch.zeros((10, 8), device='cuda')
    cols = torch.tensor([1, 2, 3], dtype=torch.int32, device='cuda')
    for ptr in ([0, 2, 1, 3], [0, 1, 2, 2], [1, 1, 2, 3], [0, 1, 3]):
        with pytest.raises(ValueError, match='cand_ptr'):
            tkr_hip.rank_candidates(U, V, torch.tensor(ptr, dtype=torch.int64, device='cuda'), cols)
    s, r = tkr_hip.rank_candidates(U, V, torch.zeros(4, dtype=torch.int64, device='cuda'), cols[:0])      # nothing to rank
    assert s.numel() == 0 and r.numel() == 0


def test_raw_abi_through_ctypes():
    """the symbol as a maintainer of the reference would bind it: no helper module in between"""
    lib = C.CDLL(os.path.join(ROOT, 'top-k-rec_amd', 'libtkr_hip.so'))
    fn = lib.tkr_rank_candidates
    fn.restype = C.c_int
    fn.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p,
                   C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p]
    rng = np.random.Generator(np.random.PCG64(3))
    n_rows, n_cols, k = 9, 120, 24
    U = rng.integers(-3, 4, (n_rows, k)).astype(np.float32) / 64
    V = rng.integers(-3, 4, (n_cols, k)).astype(np.float32) / 64
    cands = [np.sort(rng.choice(n_cols, int(n), replace=False)).astype(np.int32) for n in rng.integers(0, 90, n_rows)]
    ptr, cols = O.csr(cands)
    Ud, Vd, pd, cd = _dev(U), _dev(V), _dev(ptr), _dev(cols)
    s = torch.empty(len(cols), dtype=torch.float32, device='cuda')
    r = torch.empty(len(cols), dtype=torch.int32, device='cuda')
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    p = lambda t: C.c_void_p(t.data_ptr())
    assert fn(p(Ud), None, n_rows, p(Vd), None, n_cols, k, p(pd), p(cd), None, 0, p(s), p(r), stream) == 0
    torch.cuda.synchronize()
    ws, wr = O.rank_candidates_np(U, V, None, np.arange(n_rows), cands)
    np.testing.assert_array_equal(_bits(s.cpu().numpy()), _bits(ws))
    np.testing.assert_array_equal(r.cpu().numpy(), wr)
    # null and zero arguments: TKR_E_INVAL, nothing is launched
    good = [p(Ud), None, n_rows, p(Vd), None, n_cols, k, p(pd), p(cd), None, 0, p(s), p(r), stream]
    for at, bad in ((0, None), (3, None), (7, None), (8, None), (11, None), (12, None), (2, 0), (5, 0), (6, 0)):
        args = list(good)
        args[at] = bad
        assert fn(*args) == -1, at
    args = list(good)
    args[9], args[10] = p(pd), n_rows - 1                             # a mask whose pitch is below n_rows
    assert fn(*args) == -1
    torch.cuda.synchronize()


# ---- recommend.py --candidates ----------------------------------------------------------------------------------------------------
def _g4(golden_dir):
    d = os.path.join(golden_dir, 'g4')
    return os.path.join(d, 'data'), os.path.join(d, 'model')


def _parse_lines(path):
    out = []
    for ln in open(path).read().strip().split('\n'):
        f = ln.split(',')
        out.append((f[0], [t.split(':')[0] for t in f[1:]], [float(t.split(':')[1]) for t in f[1:]]))
    return out


def _reranked(s_row, rated_cols, cand_cols, total):
    """the oracle's line: the candidates that are not rated, in the canonical order of the full ranking, the first `total`"""
    order = R.filtered_topk(s_row, rated_cols, len(s_row), canonical=True)
    return [c for c in order if c in cand_cols][:total]


def test_recommend_candidates_on_golden_g4(golden_dir, tmp_path):
    import recommend
    data, model = _g4(golden_dir)
    uids, vids = R.read_id_list(os.path.join(data, 'uid')), R.read_id_list(os.path.join(data, 'vid'))
    ivt = {i: v for v, i in vids.items()}
    users, items = list(uids), list(vids)
    base = ['-d', data, '-m', model, '-f', '0', '-t', '30']
    plain, out = tmp_path / 'plain.txt', tmp_path / 'cand.txt'
    recommend.main(base + ['-o', str(plain)])
    # every user's line lists the whole catalogue (unknown items are dropped): the file of the full ranking, byte for byte
    whole = tmp_path / 'whole'
    whole.write_text(''.join('%s,%s,nothing:1\n' % (u, ','.join('%s:%d' % (v, x % 2) for x, v in enumerate(items))) for u in users))
    recommend.main(base + ['-o', str(out), '--candidates', str(whole)])
    assert open(str(out), 'rb').read() == open(str(plain), 'rb').read()
    # a random subset per user, in random order; user 5 on two lines with different shortlists
    rng = np.random.Generator(np.random.PCG64(8))
    rated = R.read_history(os.path.join(data, 'f0tr.txt'))
    umat = R.read_embed_text(os.path.join(model, 'final-U.dat'), uids)
    vmat = R.read_embed_text(os.path.join(model, 'final-V.dat'), vids)
    s = R.mfma_chain_scores(umat, vmat, None)
    asked = [users[x] for x in rng.permutation(len(users))[:60]] + [users[5], users[5]]
    lists = [[items[c] for c in rng.choice(len(items), int(rng.integers(1, 80)), replace=False)] for _ in asked]
    some = tmp_path / 'some'
    some.write_text(''.join('%s,%s\n' % (u, ','.join('%s:0' % v for v in l)) for u, l in zip(asked, lists)))
    lines = recommend.main(base[:-1] + ['12', '-o', str(out), '--candidates', str(some)])
    got = _parse_lines(str(out))
    assert [g[0] for g in got] == asked and open(str(out)).read() == '\n'.join(lines) + '\n'
    excluded = 0
    for (u, ids, scores), l in zip(got, lists):
        rated_cols = {vids[v] for v in rated.get(u, ()) if v in vids}
        want = _reranked(s[uids[u]], rated_cols, {vids[v] for v in l}, 12)
        assert ids == [ivt[c] for c in want], u
        np.testing.assert_allclose(scores, s[uids[u]][want], rtol=1e-6, atol=1.1e-6)
        excluded += len({vids[v] for v in l} & rated_cols)
        assert not set(ids) & rated.get(u, set())
    assert excluded > 0                                               # shortlists did name items of the history
    assert got[-1][0] == got[-2][0] == users[5] and got[-1][1] != got[-2][1]
    # a user the model does not know
    some.write_text('%s,%s:1\nnobody,%s:1\n' % (users[0], items[0], items[1]))
    with pytest.raises(KeyError, match='nobody'):
        recommend.main(base + ['-o', str(out), '--candidates', str(some)])


def test_recommend_candidates_with_new_users(golden_dir, tmp_path):
    """the fold-in fixture of tests/test_gpu_foldin.py: the last three users of G4 presented as new.  Their candidate lines follow the
    model users', whatever the order in the file, and are the full ranking's lines of those users restricted to the shortlist"""
    import recommend
    data, model = _g4(golden_dir)
    work = tmp_path / 'data'
    shutil.copytree(data, str(work))
    tokens = open(os.path.join(data, 'uid')).read().split()
    new = tokens[-3:]
    (work / 'uid').write_text('\n'.join(tokens[:-3]) + '\n')
    (tmp_path / 'new_uid').write_text('\n'.join(new) + '\n')
    items = list(R.read_id_list(os.path.join(data, 'vid')))
    fold = ['--new-uid', str(tmp_path / 'new_uid'), '--new-history', os.path.join(data, 'f0tr.txt'), '--seed', '3']
    base = ['-d', str(work), '-m', model, '-t', str(len(items))]
    full, out = tmp_path / 'full.txt', tmp_path / 'cand.txt'
    recommend.main(base + ['-o', str(full)] + fold)
    every = {g[0]: g for g in _parse_lines(str(full))}               # -t = the catalogue: every unrated item of every user, in order
    rng = np.random.Generator(np.random.PCG64(9))
    asked = [new[1], tokens[4], new[0], tokens[9], new[1], tokens[4]]
    lists = [[items[c] for c in rng.choice(len(items), 40, replace=False)] for _ in asked]
    cand = tmp_path / 'cand'
    cand.write_text(''.join('%s,%s\n' % (u, ','.join('%s:1' % v for v in l)) for u, l in zip(asked, lists)))
    recommend.main(base + ['-o', str(out), '--candidates', str(cand)] + fold)
    got = _parse_lines(str(out))
    dropped, order = 0, [1, 3, 5, 0, 2, 4]                                        # the model users' lines in file order, then the new users'
    assert [g[0] for g in got] == [asked[i] for i in order]
    for g, i in zip(got, order):
        _, ids, scores = every[asked[i]]
        keep = [j for j, v in enumerate(ids) if v in set(lists[i])]
        assert g[1] == [ids[j] for j in keep] and g[2] == [scores[j] for j in keep] and 0 < len(keep) <= 40
        dropped += 40 - len(keep)
    assert dropped > 0                                                # the histories cut into the shortlists


# ---- evaluate.py -M ... --negatives -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize('g,scs', [('g4', ['im', 'om']), ('g6', ['all'])])
def test_evaluate_negatives_on_goldens(golden_dir, capsys, g, scs):
    import evaluate as E
    import rankmetrics
    d = os.path.join(golden_dir, g)
    data, model = os.path.join(d, 'data'), os.path.join(d, 'model')
    args = ['-d', data, '-m', model, '-s', '5', '-t', '30', '-sl'] + scs
    before = E.main(args + ['-M', 'ndcg', 'mrr'])
    capsys.readouterr()
    got = E.main(args + ['-M', 'hr', 'ndcg', 'mrr', '--negatives', '20', '--neg-seed', '3'])
    assert capsys.readouterr().out.strip().split('\n') == got
    assert got[:len(before)] == before                                # the lines printed without --negatives: unchanged, and first
    want, like_ranks = O.negatives_lines(data, model, 0, 5, 30, scs, 20, 3, ['hr', 'ndcg', 'mrr'], rankmetrics.sample_negatives)
    assert got[len(before):] == want
    assert [l.split(',')[0] for l in want] == ['%s.neg20.%s' % (sc, m) for sc in scs for m in ('hr', 'ndcg', 'mrr')]
    assert 0 < min(like_ranks) or max(like_ranks) > 0                 # (not every like is first: the lines say something)
    # only the metrics -M names; more negatives than any line has eligible columns: the seed no longer matters
    a = E.main(args + ['-M', 'mrr', '--negatives', '500', '--neg-seed', '1'])
    b = E.main(args + ['-M', 'mrr', '--negatives', '500', '--neg-seed', '2'])
    assert a == b and [l.split(',')[0] for l in a[len(scs):]] == ['%s.mrr' % sc for sc in scs] + ['%s.neg500.mrr' % sc for sc in scs]
    c = E.main(args + ['-M', 'mrr', '--negatives', '5', '--neg-seed', '1'])
    assert c[:2 * len(scs)] == a[:2 * len(scs)] and c[2 * len(scs):] != a[2 * len(scs):]
