"""-m gpu: utils.get_score / utils.evaluate through K4 + K6 + K7 against the reference's own outputs
(golden G9) and against the oracle restatement on exact-arithmetic inputs with deliberate ties.
Index work (raw ranks, hit counts): bit-exact.  Reciprocal-rank sums: fp64, |d| <= 1e-12 relative (the reference adds
the same terms in a different order).

From test_raw_ranks_are_the_oracles_on_the_chain on: K6 (tkr_raw_ranks) held to the library's one fp32 score chain
(oracle/ref_np.mfma_chain_scores, exact_score in csrc/score_chain.h) at any factor width, on generic inputs and on
mirror pairs (tests/_chain_oracle.mirror_case: every column has a twin whose score is equal in real arithmetic, so
only the order of summation separates the two), and K7 alone on raw ranks made up by the test.

What these tests found on the kernel before them (a strided partial sum per lane, reduced across the wave; k <= 256
only) -- 57 of the 84 new cases fail there:
  test_raw_ranks_are_the_oracles_on_the_chain, mirror set, K = 256, differing entries of 15,872 with bias / without:
    k = 1: 0 / 0; 7: 122 / 2,567; 50: 706 / 3,597; 64: 846 / 3,320; 65: 887 / 3,465; 128: 1,422 / 3,644; 129: 1,493 / 3,605;
    200: 2,186 / 3,754; 256: 2,361 / 3,728 -- in 51 to 60 of the 62 rows, at K = 1 already (0 to 6 of 62 with bias, 11 to 22
    without), the same counts for the kept lists of K4 under either mode and of the oracle and with or without user_idx;
    generic set: 1 of 33,280 at k = 129 without bias (K = 256), none at the other widths <= 256;
    k = 257, 300, 387, 513, 769, 1032, both sets: tkr_raw_ranks returns TKR_E_UNSUPPORTED.
  test_raw_ranks_agree_with_k8_and_k12: fails in the same 21 cases (mirror k >= 7, generic k = 129 and k > 256).
  test_get_score_and_evaluate_on_the_chain: mirror set at k = 128 -- first-bucket hits 14 for 15 at (5, 30), 14 for 13 at (7, 64),
    trrs off by up to 2.8 % at (50, 300); generic k = 128 passes; k = 300 and 1032: utils.evaluate raises.
  test_k7_alone_on_made_up_raw_ranks and the argument checks pass.
On the kernel that runs exact_score (csrc/rr_eval.hip) all pass."""
import ctypes as C
import functools
import json
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _chain_oracle as CO
import _rank_oracle as RO

import tkr_hip
from oracle import ref_np as R

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def hip():
    import tkr_hip
    tkr_hip.lib()
    return tkr_hip


def _likes(path):
    likes = {}
    for line in open(path):
        terms = line.strip().split(',')
        likes[terms[0]] = set(t.split(':')[0] for t in terms[1:] if t.split(':')[1] == '1')
    return likes


def test_g9_reference_outputs(hip, golden_dir):
    import utils
    exp = json.load(open(os.path.join(golden_dir, 'g9', 'expected.json')))
    data, model = os.path.join(golden_dir, 'g4', 'data'), os.path.join(golden_dir, 'g4', 'model')
    uids = utils.get_id_dict_from_file(os.path.join(data, 'uid'))
    vids = utils.get_id_dict_from_file(os.path.join(data, 'vid'))
    U = utils.get_embed_from_file(os.path.join(model, 'final-U.dat'), uids)
    V = utils.get_embed_from_file(os.path.join(model, 'final-V.dat'), vids)
    rated, counter = utils.get_history_from_file(os.path.join(data, 'f0tr.txt'))
    assert counter == exp['counter']
    for run in exp['runs']:
        sc = run['scenario']
        te_iids = utils.get_id_dict_from_file(os.path.join(data, 'f0te.%s.idl' % sc))
        te_ivt = utils.get_iv_dict_from_file(os.path.join(data, 'f0te.%s.idl' % sc))
        score = utils.get_score(U, V, vids, te_iids)
        assert score.shape == (len(uids), len(te_iids))
        if sc == 'im':                                                # the dense view, for callers that want it
            np.testing.assert_allclose(np.asarray(score), np.load(os.path.join(golden_dir, 'g9', 'score_im.npy')), rtol=2e-5, atol=1e-7)
        hits, trrs, count = utils.evaluate(score, rated, _likes(os.path.join(data, 'f0te.%s.txt' % sc)), uids, te_iids, te_ivt,
                                           run['step'], run['total'], run['total'] // run['step'])
        assert hits == run['hits'] and count == run['count']
        np.testing.assert_allclose(trrs, run['trrs'], rtol=1e-12)
    with pytest.raises(TypeError):
        utils.evaluate(np.zeros((2, 2), np.float32), {}, {}, {}, {}, {}, 5, 30, 6)


@pytest.mark.parametrize('n_users,n_te,k,step,total', [(150, 90, 8, 5, 30), (64, 400, 16, 7, 64), (40, 700, 4, 50, 300),
                                                        (30, 20, 8, 3, 30)])
def test_exact_arithmetic_with_ties_matches_oracle(hip, n_users, n_te, k, step, total):
    """small-integer factors: every score is exact in fp32 and ties are frequent; canonical order on both sides.
    Covers total > 32 (several K4 launches), total > 256 (several K6 launches) and total > unrated columns."""
    import utils
    rng = np.random.Generator(np.random.PCG64(n_users + n_te))
    U = rng.integers(-3, 4, (n_users, k)).astype(np.float32) / 2
    V = rng.integers(-3, 4, (n_te + 5, k)).astype(np.float32) / 2
    uids = {'u%d' % x: x for x in range(n_users)}
    iids = {'i%d' % x: x for x in range(n_te + 5)}
    order = rng.permutation(n_te + 5)[:n_te]
    te_iids = {'i%d' % x: c for c, x in enumerate(order)}
    te_ivt = {c: t for t, c in te_iids.items()}
    rated, likes = {}, {}
    for uid in uids:
        rated[uid] = set('i%d' % x for x in rng.choice(n_te + 5, int(rng.integers(0, n_te // 2)), replace=False))
        likes[uid] = set('i%d' % x for x in rng.choice(n_te + 5, int(rng.integers(0, 12)), replace=False))
    interval = total // step
    score = utils.get_score(U, V, iids, te_iids)
    hits, trrs, count = utils.evaluate(score, rated, likes, uids, te_iids, te_ivt, step, total, interval)
    ref_score = R.utils_get_score(U, V, iids, te_iids)
    np.testing.assert_array_equal(np.asarray(score), ref_score)       # exact arithmetic
    eh, er, ec = R.utils_evaluate(ref_score, rated, likes, uids, te_iids, te_ivt, step, total, interval, canonical=True)
    assert hits == eh and count == ec
    np.testing.assert_allclose(trrs, er, rtol=1e-12)


def test_raw_ranks_direct(hip):
    """K6 alone: raw rank = position among ALL columns for kept columns, -1 padding untouched, bias honoured"""
    rng = np.random.Generator(np.random.PCG64(3))
    n_rows, n_cols, k, K = 37, 130, 200, 24
    U = rng.integers(-4, 5, (n_rows, k)).astype(np.float32) / 4
    V = rng.integers(-4, 5, (n_cols, k)).astype(np.float32) / 4
    b = rng.integers(-8, 9, n_cols).astype(np.float32) / 8
    s = U @ V.T + b
    rated = [np.sort(rng.choice(n_cols, int(rng.integers(0, 110)), replace=False)) for _ in range(n_rows)]
    ptr = np.zeros(n_rows + 1, np.int64)
    np.cumsum([len(x) for x in rated], out=ptr[1:])
    ids = np.full((n_rows, K), -1, np.int32)
    want = np.full((n_rows, K), -1, np.int32)
    for r in range(n_rows):
        order = np.argsort(s[r], kind='stable')[::-1]
        pos = {int(c): t for t, c in enumerate(order)}
        kept = [int(c) for c in order if c not in set(rated[r].tolist())][:K]
        ids[r, :len(kept)] = kept
        want[r, :len(kept)] = [pos[c] for c in kept]
    dev = torch.device('cuda')
    got = hip.raw_ranks(torch.from_numpy(U).to(dev), torch.from_numpy(V).to(dev), torch.from_numpy(ids).to(dev),
                        torch.from_numpy(ptr).to(dev), torch.from_numpy(np.concatenate(rated).astype(np.int32)).to(dev),
                        bias=torch.from_numpy(b).to(dev))
    np.testing.assert_array_equal(got.cpu().numpy(), want)


# ---- K6 on the one score chain, any factor width ---------------------------------------------------------------------
F32 = np.float32
KS = (1, 30, 64, 65, 256)                    # one kept column; fewer than a wave; a wave; a wave and one; the most a launch takes
KINDS = ('mirror', 'generic')


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to('cuda')


def _csr(rows):
    ptr = np.zeros(len(rows) + 1, dtype=np.int64)
    np.cumsum([len(x) for x in rows], out=ptr[1:])
    return ptr, (np.concatenate(rows) if len(rows) else np.zeros(0)).astype(np.int32)


@functools.lru_cache(maxsize=None)
def _inputs(kind, k):
    """one input set of width k on the host and on the device, with the oracle's chain scores without bias (s[False]) and with it
    (s[True]: one more fp32 add, so no hazard of its own) and their hazard marks: built once per process, never written"""
    c = dict(CO.mirror_case(k) if kind == 'mirror' else CO.case(k))
    s0, hz = CO.chain_scores_checked(c['rows'], c['V'], None)
    sb = (s0 + c['b'].reshape(1, -1)).astype(F32) + F32(0.0)
    for a in (s0, sb, hz):
        a.setflags(write=False)
    c['s'], c['hz'] = {False: s0, True: sb}, hz
    n_rows = c['rows'].shape[0]
    c['sets'] = [set(x.tolist()) for x in c['rated']]
    rptr, rcols = _csr(c['rated'])
    c['rptr'], c['rcols'] = _dev(rptr), _dev(rcols)
    c['mask'], c['pitch'] = tkr_hip.build_rated_mask(c['rptr'], c['rcols'], n_rows, c['V'].shape[0])
    c['Vd'], c['bd'], c['rows_d'] = _dev(c['V']), _dev(c['b']), _dev(c['rows'])
    # the same rows through user_idx: the set's own table where it has one, else the rows backwards with a few more behind them
    if c['user_idx'] is not None:
        c['table_d'], c['idx_d'] = _dev(c['U']), _dev(c['user_idx'])
    else:
        c['table_d'] = _dev(np.concatenate([c['rows'][::-1], c['rows'][:5]]))
        c['idx_d'] = _dev(np.arange(n_rows - 1, -1, -1, dtype=np.int32))
    return c


@functools.lru_cache(maxsize=None)
def _kept256(kind, k, source, with_bias):
    """the first 256 kept columns of every row, -1 padded: 'oracle' -- R.filtered_topk of the oracle's scores, K6 apart from K4;
    'fp32' / 'refine' -- tkr_score_topk under that TKR_TOPK_MATH mode"""
    c = _inputs(kind, k)
    if source == 'oracle':
        ids = np.full((len(c['sets']), 256), -1, dtype=np.int32)
        for r, rated in enumerate(c['sets']):
            kept = R.filtered_topk(c['s'][with_bias][r], rated, 256, canonical=True)
            ids[r, :len(kept)] = kept
    else:
        tkr_hip.set_topk_math(source)
        try:
            ids = tkr_hip.score_topk(c['rows_d'], c['Vd'], 256, bias=c['bd'] if with_bias else None, mask=c['mask'],
                                 mask_pitch=c['pitch']).cpu().numpy()
        finally:
            tkr_hip.set_topk_math(tkr_hip.TOPK_MATH_DEFAULT)
    ids.setflags(write=False)
    return ids


def _clean_rows(c):
    """the rows without a hazard entry: the others are not compared (the CPU tests show how few there are: none on the mirror sets)"""
    return np.flatnonzero(~c['hz'].any(axis=1))


@pytest.mark.parametrize('k', CO.MIRROR_WIDTHS)
@pytest.mark.parametrize('kind', KINDS)
def test_raw_ranks_are_the_oracles_on_the_chain(hip, kind, k):
    """tkr_raw_ranks == RO.raw_ranks_np on the oracle's chain scores, every entry, with and without bias, with and without user_idx,
    for the kept lists of K4 (both modes) and of the oracle, at every K of KS"""
    c = _inputs(kind, k)
    rows = _clean_rows(c)
    assert len(rows) == c['hz'].shape[0] if kind == 'mirror' else len(rows) >= 0.9 * c['hz'].shape[0]
    report = []
    for with_bias in (False, True):
        s = c['s'][with_bias]
        for source in ('oracle', 'fp32', 'refine'):
            ids256 = _kept256(kind, k, source, with_bias)
            for K in KS:
                ids = np.ascontiguousarray(ids256[:, :K])
                want = np.stack([RO.raw_ranks_np(s[r], c['sets'][r], ids[r]) for r in rows])
                for U, idx in ((c['rows_d'], None), (c['table_d'], c['idx_d'])):
                    got = hip.raw_ranks(U, c['Vd'], _dev(ids), c['rptr'], c['rcols'], bias=c['bd'] if with_bias else None,
                                        user_idx=idx).cpu().numpy()[rows]
                    bad = got != want
                    if bad.any():
                        report.append('bias %d, %s, K %d, idx %d: %d of %d entries differ, in %d of %d rows'
                                      % (with_bias, source, K, idx is not None, int(bad.sum()), bad.size, int(bad.any(axis=1).sum()), len(rows)))
    print('%s k = %d: %s' % (kind, k, '; '.join(report) or 'every entry equal'))
    assert not report, report[:6]


@pytest.mark.parametrize('k', CO.MIRROR_WIDTHS)
@pytest.mark.parametrize('kind', KINDS)
def test_raw_ranks_agree_with_k8_and_k12(hip, kind, k):
    """no oracle, no allowance: the raw rank of a kept column is K8's unfiltered rank of it (like_ranks without a mask over the kept
    columns, ascending per row, mapped back) and K12's rank of it when every row lists the whole catalogue unmasked"""
    c = _inputs(kind, k)
    n_rows, n_cols = c['rows'].shape[0], c['V'].shape[0]
    cptr, ccols = _csr([np.arange(n_cols, dtype=np.int32)] * n_rows)
    cptr, ccols = _dev(cptr), _dev(ccols)
    for with_bias in (False, True):
        bd = c['bd'] if with_bias else None
        _, r12 = hip.rank_candidates(c['rows_d'], c['Vd'], cptr, ccols, bias=bd)
        r12 = r12.cpu().numpy().reshape(n_rows, n_cols)
        for K in (65, 256):
            ids = np.ascontiguousarray(_kept256(kind, k, 'refine', with_bias)[:, :K])
            raw = hip.raw_ranks(c['rows_d'], c['Vd'], _dev(ids), c['rptr'], c['rcols'], bias=bd).cpu().numpy()
            live = ids >= 0
            np.testing.assert_array_equal(raw[~live], -1)
            asc = [np.sort(ids[r][live[r]]) for r in range(n_rows)]
            lptr, lcols = _csr(asc)
            r8 = hip.like_ranks(c['rows_d'], c['Vd'], _dev(lptr), _dev(lcols), bias=bd).cpu().numpy()
            for r in range(n_rows):
                kept = ids[r][live[r]]
                got = raw[r][live[r]]
                np.testing.assert_array_equal(got, r12[r, kept], err_msg='K12 %s' % ((kind, k, with_bias, K, r),))
                np.testing.assert_array_equal(got[np.argsort(kept)], r8[lptr[r]:lptr[r + 1]], err_msg='K8 %s' % ((kind, k, with_bias, K, r),))


@pytest.mark.parametrize('step,total', [(5, 30), (7, 64), (50, 300)])
@pytest.mark.parametrize('k', [128, 300, 1032])
@pytest.mark.parametrize('kind', KINDS)
def test_get_score_and_evaluate_on_the_chain(hip, kind, k, step, total):
    """utils.get_score + utils.evaluate against R.utils_evaluate(canonical=True) on the oracle's chain scores: hits and count exact,
    trrs to the file's 1e-12.  total = 300 takes two K6 launches and is more than some rows have unrated columns (on the mirror set
    row 1 keeps 3 and row 2 none; on the generic set 274 to 333)."""
    import utils
    c = _inputs(kind, k)
    assert not c['hz'].any()                                          # a condition on the inputs (tests/test_chain_oracle_cpu.py)
    s = c['s'][False]                                                 # utils.evaluate ranks without a bias
    n_rows, n_cols = s.shape
    rng = np.random.Generator(np.random.PCG64(9400 + k))
    uids = {'u%d' % r: r for r in range(n_rows)}
    iids = {'i%d' % x: x for x in range(n_cols)}
    te_ivt = {x: t for t, x in iids.items()}
    rated = {'u%d' % r: set('i%d' % x for x in c['rated'][r]) for r in range(n_rows)}
    likes = {}
    for r in range(n_rows):
        near = RO.kept_order(s[r], c['sets'][r])[:total + 20]
        picks = np.r_[near[rng.permutation(len(near))[:6]], rng.choice(n_cols, 6, replace=False)] if r % 9 else []      # every ninth: no like
        likes['u%d' % r] = set('i%d' % int(x) for x in picks)
    interval = total // step
    score = utils.get_score(c['rows'], c['V'], iids, iids)
    hits, trrs, count = utils.evaluate(score, rated, likes, uids, iids, te_ivt, step, total, interval)
    eh, er, ec = R.utils_evaluate(s, rated, likes, uids, iids, te_ivt, step, total, interval, canonical=True)
    assert eh[-1] > 30                                                # the likes do reach the lists
    assert hits == eh and count == ec
    np.testing.assert_allclose(trrs, er, rtol=1e-12)


def _k7(ids, raw, lptr, lcols, step, interval):
    """tkr_count_hits_rr through the raw ABI -> (hit_first int32 [n_rows, interval], rr_first float64 [n_rows, interval])"""
    lib = tkr_hip.lib()
    n_rows, K = ids.shape
    d = [_dev(ids), _dev(raw), _dev(lptr), _dev(lcols if len(lcols) else np.zeros(1, np.int32))]
    hit = torch.zeros((n_rows, interval), dtype=torch.int32, device='cuda')
    rr = torch.zeros((n_rows, interval), dtype=torch.float64, device='cuda')
    p = [C.c_void_p(t.data_ptr()) for t in d]
    rc = lib.tkr_count_hits_rr(p[0], p[1], C.c_int32(n_rows), C.c_int32(K), p[2], p[3], C.c_int32(step), C.c_int32(interval),
                               C.c_void_p(hit.data_ptr()), C.c_void_p(rr.data_ptr()), C.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0
    torch.cuda.synchronize()
    return hit.cpu().numpy(), rr.cpu().numpy()


@pytest.mark.parametrize('K,step,interval,no_likes', [(64, 5, 6, False),       # most made-up ranks have t // step >= interval
                                                      (30, 100, 3, False),     # step > K
                                                      (64, 2, 3, False),       # interval * step < K
                                                      (256, 50000, 20, False), # buckets that reach ranks of ~10^6
                                                      (30, 5, 6, True)])       # an empty like CSR
def test_k7_alone_on_made_up_raw_ranks(hip, K, step, interval, no_likes):
    """tkr_count_hits_rr on kept ids and raw ranks the test makes up (strictly increasing per row, gaps of 1 to 30,000: up to ~4 10^6),
    -1 padding from some position on (from position 0 in row 5), empty like rows: per-row hit_first exact; per-row rr_first equal bit
    for bit to a float64 loop that adds 1.0 / (t + 1) in list order, since the kernel is sequential per row"""
    rng = np.random.Generator(np.random.PCG64(9500 + K + step))
    n_rows, n_cols = 70, 2000
    ids = np.stack([rng.choice(n_cols, K, replace=False) for _ in range(n_rows)]).astype(np.int32)
    gaps = np.stack([rng.integers(1, (2, 3, 50, 30000)[r % 4], K, endpoint=True) for r in range(n_rows)])
    raw = (np.cumsum(gaps, axis=1) - 1).astype(np.int32)
    for r in range(0, n_rows, 5):                                     # rows 0, 5, 10, ...: padded from a position on; row 5 from 0
        cut = 0 if r == 5 else int(rng.integers(1, K + 1))
        ids[r, cut:], raw[r, cut:] = -1, -1
    likes = []
    for r in range(n_rows):
        mine = ids[r][ids[r] >= 0]
        n = 0 if (no_likes or r % 7 == 3) else int(rng.integers(1, 20))
        likes.append(np.unique(np.r_[mine[rng.permutation(len(mine))[:n]], rng.choice(n_cols, n // 2)]).astype(np.int32))
    lptr, lcols = _csr(likes)
    hit, rr = _k7(ids, raw, lptr, lcols, step, interval)
    want_hit, want_rr = np.zeros((n_rows, interval), dtype=np.int32), np.zeros((n_rows, interval), dtype=np.float64)
    for r in range(n_rows):
        mine = set(likes[r].tolist())
        for p in range(K):
            if ids[r, p] < 0:
                break
            if int(ids[r, p]) in mine:
                t = int(raw[r, p])
                if t // step < interval:
                    want_hit[r, t // step] += 1
                    want_rr[r, t // step] = want_rr[r, t // step] + 1.0 / (t + 1)
    assert no_likes or (want_hit.sum() > 20 and (want_hit.sum(axis=1) == 0).any())
    assert K < 256 or raw.max() > 10 ** 6
    np.testing.assert_array_equal(hit, want_hit)
    np.testing.assert_array_equal(rr.view(np.uint64), want_rr.view(np.uint64))


def test_k6_k7_bad_arguments_are_refused_before_any_device_access(hip):
    """null pointers and non-positive sizes: TKR_E_INVAL; more kept columns than a launch takes: TKR_E_UNSUPPORTED; any factor width is
    taken.  The pointer passed is never dereferenced: every call below fails its checks"""
    lib = hip.lib()
    k6, k7 = lib.tkr_raw_ranks, lib.tkr_count_hits_rr
    k6.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32,
                   C.c_void_p, C.c_void_p]
    k7.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p,
                   C.c_void_p]
    try:
        p = 4096
        good = dict(U=p, idx=None, n_rows=4, Vt=p, bias=None, k=300, rptr=p, rcols=p, ids=p, K=30, out=p, stream=None)
        for change in (dict(U=None), dict(Vt=None), dict(rptr=None), dict(ids=None), dict(out=None), dict(n_rows=0), dict(n_rows=-3),
                       dict(k=0), dict(k=-1), dict(K=0), dict(K=-5)):
            assert k6(*dict(good, **change).values()) == -1, change                  # TKR_E_INVAL
        for change in (dict(K=257), dict(K=1 << 20), dict(K=257, k=8)):
            assert k6(*dict(good, **change).values()) == -2, change                  # TKR_E_UNSUPPORTED
        good = dict(ids=p, raw=p, n_rows=4, K=30, lptr=p, lcols=p, step=5, interval=6, hit=p, rr=p, stream=None)
        for change in (dict(ids=None), dict(raw=None), dict(lptr=None), dict(hit=None), dict(rr=None), dict(n_rows=0), dict(K=0),
                       dict(step=0), dict(step=-1), dict(interval=0), dict(interval=-2)):
            assert k7(*dict(good, **change).values()) == -1, change
    finally:
        k6.argtypes = k7.argtypes = None
