"""K4 (tkr_score_topk) at EVERY factor width on generic inputs, held to the one fma chain of the library -- oracle/ref_np.mfma_chain_scores,
exact_score in csrc/score_chain.h -- bit for bit, and K12 / K8 / evaluate.py -M held to K4.  The other K4 tests reach widths above 256
only with exact arithmetic, where any order of summation gives the same bits; here the factors are N(0, 0.01^2) rounded like '%f', on
which the order shows in most score bits (tests/test_chain_oracle_cpu.py).  The oracle's double rounding is marked entry by entry
(tests/_chain_oracle.chain_scores_checked), so no share of mismatches is allowed anywhere.

What this file found: score_topk_slab_kernel (256 < k <= 768) interleaved the k-halves inside every 256 factors instead of over the
whole width.  On that kernel test_k4_scores_are_the_oracles_chain and test_k12_whole_catalogue_lists_reproduce_k4 fail at every slab
width -- 13.1, 18.6, 29.3, 40.8, 48.0, 46.0 and 57.2 % of the 3,900 returned score bits differ at k = 257, 264, 300, 387, 512, 513 and
768, 6.2 % of the 1,200 at 40 x 66,000, no id -- and pass at every other width.

test_mirror_pairs_k4_is_the_oracles_chain_and_k12_k8_reproduce_it runs the three kernels on a catalogue of built near-ties
(CO.mirror_case: every column has a twin whose score differs by the order of summation alone), where bound-and-refine finds a twin
inside the fp16 margin of every candidate; it passed when it was written."""
import functools
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

K = CO.TOP
MODES = ('fp32', 'refine')


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to('cuda')


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _csr(rows):
    ptr = np.zeros(len(rows) + 1, dtype=np.int64)
    np.cumsum([len(x) for x in rows], out=ptr[1:])
    return ptr, (np.concatenate(rows) if len(rows) else np.zeros(0)).astype(np.int32)


@functools.lru_cache(maxsize=None)
def _case(k):
    """the input set of width k (or 'big'), on the host and on the device, with its rated mask: built once per process"""
    c = dict(CO.case(CO.BIG[2], CO.BIG[:2]) if k == 'big' else CO.case(k))
    rptr, rcols = _csr(c['rated'])
    c['mask'], c['pitch'] = tkr_hip.build_rated_mask(_dev(rptr), _dev(rcols), len(c['rated']), c['V'].shape[0])
    c['Ud'], c['Vd'], c['bd'] = _dev(c['U']), _dev(c['V']), _dev(c['b'])
    c['idx_d'] = None if c['user_idx'] is None else _dev(c['user_idx'])
    return c


@functools.lru_cache(maxsize=None)
def _oracle(k):
    """(scores, hazard) of the input set: computed once, read by every test, never written"""
    c = _case(k)
    s, hz = CO.chain_scores_checked(c['rows'], c['V'], c['b'])
    s.setflags(write=False)
    hz.setflags(write=False)
    return s, hz


def _k4(c, mode, split=True):
    tkr_hip.set_topk_math(mode)
    try:
        ids, sc = tkr_hip.score_topk(c['Ud'], c['Vd'], K, bias=c['bd'], user_idx=c['idx_d'], mask=c['mask'], mask_pitch=c['pitch'],
                                     want_scores=True, split=split)
        return ids.cpu().numpy(), sc.cpu().numpy()
    finally:
        tkr_hip.set_topk_math(tkr_hip.TOPK_MATH_DEFAULT)


@pytest.mark.parametrize('k', CO.WIDTHS + ['big'])
def test_k4_scores_are_the_oracles_chain(k):
    """under both arithmetic modes: every returned score that is no hazard entry of the oracle has the oracle's bits; on every row
    without a hazard entry and without an exact tie at the cut the ids are R.filtered_topk of the oracle's scores"""
    c = _case(k)
    want, hz = _oracle(k)
    n_rows = want.shape[0]
    assert hz.mean() <= 1e-4                                          # a condition on the inputs (tests/test_chain_oracle_cpu.py)
    for mode in MODES:
        ids, sc = _k4(c, mode)
        assert ids.shape == (n_rows, K) and ids.min() >= 0            # at most 59 rated columns of 333: every list is full
        rows = np.repeat(np.arange(n_rows), K).reshape(n_rows, K)
        ok = ~hz[rows, ids]
        differ = _bits(sc)[ok] != _bits(want[rows, ids])[ok]
        print('k = %s, %s: %d of %d returned score bits differ from the oracle (%.1f %%)' % (k, mode, int(differ.sum()), differ.size,
                                                                                             100.0 * differ.mean()))
        assert not differ.any(), (k, mode)
        checked = 0
        for r in range(n_rows):
            rated = set(c['rated'][r].tolist())
            assert not rated & set(ids[r].tolist())
            if hz[r].any():
                continue
            kept = np.sort(np.delete(want[r], c['rated'][r]))[::-1]
            if kept[K - 1] == kept[K]:
                continue
            assert ids[r].tolist() == R.filtered_topk(want[r], rated, K, canonical=True), (k, mode, r)
            checked += 1
        assert checked >= 0.9 * n_rows


@pytest.mark.parametrize('k', CO.WIDTHS)
def test_k12_whole_catalogue_lists_reproduce_k4(k):
    """every row lists the whole catalogue: topk_from_ranks of K12's scores and ranks is K4's list, ids and score bits, under both modes
    of K4.  Two kernels, no oracle: no allowance."""
    c = _case(k)
    n_rows, n_cols = len(c['rated']), c['V'].shape[0]
    ptr, cols = _csr([np.arange(n_cols, dtype=np.int32)] * n_rows)
    s, r = tkr_hip.rank_candidates(c['Ud'], c['Vd'], _dev(ptr), _dev(cols), bias=c['bd'], user_idx=c['idx_d'], mask=c['mask'],
                                   mask_pitch=c['pitch'])
    ids, top = tkr_hip.topk_from_ranks(_dev(ptr), _dev(cols), s, r, K)
    ids, top = ids.cpu().numpy(), top.cpu().numpy()
    for mode in MODES:
        ki, ks = _k4(c, mode)
        differ = _bits(top) != _bits(ks)
        print('k = %d, %s: %d of %d score bits differ between K12 and K4, %d ids' % (k, mode, int(differ.sum()), differ.size,
                                                                                    int((ids != ki).sum())))
        np.testing.assert_array_equal(ids, ki, err_msg=str((k, mode)))
        np.testing.assert_array_equal(_bits(top), _bits(ks), err_msg=str((k, mode)))


@pytest.mark.parametrize('k', CO.WIDTHS)
def test_k8_like_ranks_agree_with_k4_lists(k):
    """likes drawn partly from the row's approximate best 40, a few of those rated as well: a like at position p of K4's list has rank
    p; a like outside the list has rank >= K, or -1 exactly when it is rated"""
    c = _case(k)
    n_rows, n_cols = len(c['rated']), c['V'].shape[0]
    rng = np.random.Generator(np.random.PCG64(8100 + k))
    best = np.argsort(-(c['rows'] @ c['V'].T + c['b']), axis=1)[:, :40]
    likes, rated = [], []
    for r in range(n_rows):
        near = rng.choice(best[r], int(rng.integers(0, 6)), replace=False)
        far = rng.choice(n_cols, int(rng.integers(1, 12)), replace=False)
        likes.append(np.unique(np.r_[near, far]).astype(np.int32))
        rated.append(np.unique(np.r_[c['rated'][r], rng.choice(best[r], 3, replace=False)]).astype(np.int32))
    lptr, lcols = _csr(likes)
    rptr, rcols = _csr(rated)
    mask, pitch = tkr_hip.build_rated_mask(_dev(rptr), _dev(rcols), n_rows, n_cols)
    ranks = tkr_hip.like_ranks(c['Ud'], c['Vd'], _dev(lptr), _dev(lcols), bias=c['bd'], user_idx=c['idx_d'], mask=mask,
                               mask_pitch=pitch).cpu().numpy()
    line = np.repeat(np.arange(n_rows), np.diff(lptr))
    is_rated = np.zeros((n_rows, n_cols), dtype=bool)
    is_rated[np.repeat(np.arange(n_rows), np.diff(rptr)), rcols] = True
    like_rated = is_rated[line, lcols]
    assert like_rated.any() and not like_rated.all()
    try:
        for mode in MODES:
            tkr_hip.set_topk_math(mode)
            ids = tkr_hip.score_topk(c['Ud'], c['Vd'], K, bias=c['bd'], user_idx=c['idx_d'], mask=mask, mask_pitch=pitch).cpu().numpy()
            where = np.full((n_rows, n_cols), -1, dtype=np.int16)
            where[np.repeat(np.arange(n_rows), K), ids.reshape(-1)] = np.tile(np.arange(K), n_rows)
            p = where[line, lcols]
            listed = p >= 0
            assert listed.sum() > 100                                  # the likes do reach the lists
            np.testing.assert_array_equal(ranks[listed], p[listed], err_msg=str((k, mode)))
            np.testing.assert_array_equal(ranks[~listed] == -1, like_rated[~listed], err_msg=str((k, mode)))
            assert np.all(ranks[~listed & ~like_rated] >= K)
            assert not np.any(listed & like_rated)
    finally:
        tkr_hip.set_topk_math(tkr_hip.TOPK_MATH_DEFAULT)


MIRROR_WIDTHS = [50, 128, 256, 300, 769]      # refine's widths (k <= 128), the widest single tile, a slab width, the generic kernel


@functools.lru_cache(maxsize=None)
def _mirror(k):
    """CO.mirror_case(k) with its device copies, rated mask and oracle scores: every column has a twin inside its fp16 margin"""
    c = dict(CO.mirror_case(k))
    rptr, rcols = _csr(c['rated'])
    c['mask'], c['pitch'] = tkr_hip.build_rated_mask(_dev(rptr), _dev(rcols), len(c['rated']), c['V'].shape[0])
    c['Ud'], c['Vd'], c['bd'] = _dev(c['U']), _dev(c['V']), _dev(c['b'])
    c['idx_d'] = None if c['user_idx'] is None else _dev(c['user_idx'])
    c['want'], c['hz'] = CO.chain_scores_checked(c['rows'], c['V'], c['b'])
    c['want'].setflags(write=False)
    return c


@pytest.mark.parametrize('k', MIRROR_WIDTHS)
def test_mirror_pairs_k4_is_the_oracles_chain_and_k12_k8_reproduce_it(k):
    """a catalogue of near-ties (62 rows x 600 mirror pairs, half the columns rated; row 1 keeps 3 columns, row 2 none): K4 under both
    modes returns the oracle's score bits and, on every row without an exact tie at the cut, R.filtered_topk's ids, -1 / -inf behind
    a short list; K12's whole-catalogue lists are K4's, ids and bits; a like at position p of K4's list has K8 rank p, one outside it
    a rank >= K, or -1 exactly when it is rated"""
    c = _mirror(k)
    want = c['want']
    n_rows, n_cols = want.shape
    assert not c['hz'].any()                                          # a condition on the inputs (tests/test_chain_oracle_cpu.py)
    ptr, cols = _csr([np.arange(n_cols, dtype=np.int32)] * n_rows)
    s12, r12 = tkr_hip.rank_candidates(c['Ud'], c['Vd'], _dev(ptr), _dev(cols), bias=c['bd'], user_idx=c['idx_d'], mask=c['mask'],
                                       mask_pitch=c['pitch'])
    ids12, top12 = tkr_hip.topk_from_ranks(_dev(ptr), _dev(cols), s12, r12, K)
    ids12, top12 = ids12.cpu().numpy(), top12.cpu().numpy()
    is_rated = np.zeros((n_rows, n_cols), dtype=bool)
    for r in range(n_rows):
        is_rated[r, c['rated'][r]] = True
    for mode in MODES:
        ids, sc = _k4(c, mode)
        checked = 0
        for r in range(n_rows):
            n = min(K, n_cols - len(c['rated'][r]))
            assert np.all(ids[r, n:] == -1) and np.all(ids[r, :n] >= 0), (k, mode, r)
            assert not is_rated[r, ids[r, :n]].any()
            np.testing.assert_array_equal(_bits(sc[r, :n]), _bits(want[r, ids[r, :n]]), err_msg=str((k, mode, r)))
            kept = np.sort(want[r][~is_rated[r]])[::-1]
            if len(kept) > K and kept[K - 1] == kept[K]:
                continue
            assert ids[r, :n].tolist() == R.filtered_topk(want[r], set(c['rated'][r].tolist()), K, canonical=True), (k, mode, r)
            checked += 1
        # a kept column's twin is kept as well in half the cases and then sits next to it, so about a third of the lists end between
        # two twins, and these have equal bits in up to 77 % of the pairs (k = 50): up to a quarter of the rows are left out here;
        # K12 below compares every row
        assert checked >= 0.6 * n_rows
        np.testing.assert_array_equal(ids12, ids, err_msg=str((k, mode)))
        np.testing.assert_array_equal(_bits(top12), _bits(sc), err_msg=str((k, mode)))
        # K8: the list itself, the twin of every listed column and the row's first five rated columns as likes
        m = n_cols // 2
        likes = [np.unique(np.r_[ids[r][ids[r] >= 0], (ids[r][ids[r] >= 0] + m) % n_cols, c['rated'][r][:5]]).astype(np.int32)
                 for r in range(n_rows)]
        lptr, lcols = _csr(likes)
        ranks = tkr_hip.like_ranks(c['Ud'], c['Vd'], _dev(lptr), _dev(lcols), bias=c['bd'], user_idx=c['idx_d'], mask=c['mask'],
                                   mask_pitch=c['pitch']).cpu().numpy()
        for r in range(n_rows):
            where = {int(col): p for p, col in enumerate(ids[r]) if col >= 0}
            for col, rank in zip(likes[r].tolist(), ranks[lptr[r]:lptr[r + 1]].tolist()):
                if col in where:
                    assert rank == where[col], (k, mode, r, col)
                elif is_rated[r, col]:
                    assert rank == -1, (k, mode, r, col)
                else:
                    assert rank >= K, (k, mode, r, col)


def test_item_range_split_is_invisible_at_a_slab_width():
    """700 rows x 20,000 columns at k = 300 (two slabs, scalar staging), every seventh column a copy of column 1 -- exact ties across the
    item ranges: the split launch and the unsplit one return equal ids and score bits"""
    rng = np.random.Generator(np.random.PCG64(8300))
    n_rows, n_cols, k = 700, 20000, 300
    U = np.round(rng.standard_normal((n_rows, k)) * 0.01, 6).astype(np.float32)
    V = np.round(rng.standard_normal((n_cols, k)) * 0.01, 6).astype(np.float32)
    V[::7] = V[1]
    ptr = np.arange(0, (n_rows + 1) * 20, 20, dtype=np.int64)
    cols = np.sort(rng.integers(0, n_cols, (n_rows, 20)), axis=1).reshape(-1).astype(np.int32)
    mask, pitch = tkr_hip.build_rated_mask(_dev(ptr), _dev(cols), n_rows, n_cols)
    Ud, Vd = _dev(U), _dev(V)
    try:
        for mode in MODES:
            tkr_hip.set_topk_math(mode)
            a = tkr_hip.score_topk(Ud, Vd, K, mask=mask, mask_pitch=pitch, want_scores=True, split=True)
            b = tkr_hip.score_topk(Ud, Vd, K, mask=mask, mask_pitch=pitch, want_scores=True, split=False)
            torch.cuda.synchronize()
            assert torch.equal(a[0], b[0]) and torch.equal(a[1].view(torch.int32), b[1].view(torch.int32)), mode
    finally:
        tkr_hip.set_topk_math(tkr_hip.TOPK_MATH_DEFAULT)


def test_fused_model_of_width_387_end_to_end(tmp_path, capsys):
    """three k = 128 models with a bias, 300 users x 400 items, written by the project's writers and fused by fuse.py --method w: width
    3 x (128 + 1) = 387 -- odd, two slabs, scalar staging.  evaluate.py -M acc on it: the S.acc lines (K8) equal the plain lines (K4 +
    K5), and both equal tests/_rank_oracle.metric_lines on the fused tables"""
    import evaluate as E
    import fuse
    import synth
    import textio
    data, out = str(tmp_path / 'data'), str(tmp_path / 'fused')
    r = synth.make_ratings(300, 320, 80, seed=23, mu=3.0, sigma=0.5, min_r=6, max_r=50, om_per_user=4)
    synth.write_dataset(data, r)
    rng = np.random.Generator(np.random.PCG64(8400))
    models = []
    for m in range(3):
        d = str(tmp_path / ('m%d' % m))
        os.mkdir(d)
        textio.write_matrix(os.path.join(d, 'final-U.dat'), (rng.standard_normal((300, 128)) * 0.05).astype(np.float32), where='host')
        textio.write_matrix(os.path.join(d, 'final-V.dat'), (rng.standard_normal((400, 128)) * 0.05).astype(np.float32), where='host')
        textio.write_matrix(os.path.join(d, 'final-B.dat'), (rng.standard_normal((400, 1)) * 0.05).astype(np.float32), where='host')
        models.append(d)
    fuse.main(['-d', data, '-m'] + models + ['-o', out, '--method', 'w', '--weights', '0.5', '1', '2'])
    uids = R.read_id_list(os.path.join(data, 'uid'))
    assert R.read_embed_text(os.path.join(out, 'final-U.dat'), uids).shape == (300, 387)
    capsys.readouterr()
    scs = ['im', 'om']
    got = E.main(['-d', data, '-m', out, '-s', '5', '-t', '30', '-sl'] + scs + ['-M', 'acc'])
    assert capsys.readouterr().out.strip().split('\n') == got and len(got) == 4
    want = RO.metric_lines(data, out, 0, 5, 30, scs, ['acc'])
    assert got[2:] == want
    assert [l.replace('.acc', '', 1) for l in got[2:]] == got[:2]
    assert any(float(x) > 0 for x in got[0].split(',')[1:])           # the lines say something
