"""K4, K12, K8, K6 and evaluate.py on scores that leave the finite normal range: NaN and infinite factors, products and bias adds that
overflow, user rows whose sum of squares overflows or underflows, subnormal scores (tests/_nonfinite_oracle.py).  The contract is
include/tkr.h, K4: NaN > +inf > finite > -inf, every NaN one score, ties -> higher column first -- np.argsort(kind='stable') read
backwards, which R.filtered_topk, RO.like_ranks_np and RO.raw_ranks_np already state (tests/test_nonfinite_cpu.py).  Every factor is a
small integer times a power of two: no row and no entry is left out of any comparison.  Every case runs at 130 x 333 at every width;
the 700 x 20,000 shape runs the integer-factor cases (NF.SPLIT_CASES: the only ones whose oracle does not have to walk the chain over
14 M entries), and K12 runs the small shape only.  `overflow` holds +-inf and no NaN: the chain's steps are fused.

On the kernels before this file: K4 never listed a NaN column and returned -1 for a whole row whose user row
held a NaN under bound-and-refine, K6 counted no NaN rated column in front of anything, K8 and K12 ranked a NaN by its sign bit."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _nonfinite_oracle as NF
import _rank_oracle as RO

import tkr_hip
from oracle import ref_np as R

pytestmark = pytest.mark.gpu

K = NF.TOP
RUNS = [('fp32', True), ('fp32', False), ('refine', True), ('refine', False)]
SMALL = [(name, k) for name in NF.CASES for k in NF.WIDTHS]
EVERY = SMALL + [(name, 'split') for name in NF.SPLIT_CASES]


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to('cuda')


def _csr(rows):
    ptr = np.zeros(len(rows) + 1, dtype=np.int64)
    np.cumsum([len(x) for x in rows], out=ptr[1:])
    return ptr, (np.concatenate(rows) if len(rows) else np.zeros(0)).astype(np.int32)


@functools.lru_cache(maxsize=None)
def _case(name, k):
    """the input set on the host and on the device with its rated mask, the chain's scores (`want`) and the oracle's lists: built once"""
    if k == 'split':
        c = dict(NF.split_case(name))
        want = c['scores']
    else:
        c = dict(NF.case(name, k))
        want = NF.scores(name, k)
    n_rows, n_cols = want.shape
    c['want'] = want
    c['rptr'], c['rcols'] = _csr(c['rated'])
    c['rptr_d'], c['rcols_d'] = _dev(c['rptr']), _dev(c['rcols'])
    c['mask'], c['pitch'] = tkr_hip.build_rated_mask(c['rptr_d'], c['rcols_d'], n_rows, n_cols)
    c['Ud'], c['Vd'], c['bd'] = _dev(c['U']), _dev(c['V']), _dev(c['b'])
    ids = np.full((n_rows, K), -1, dtype=np.int32)
    sc = np.full((n_rows, K), -np.inf, dtype=np.float32)
    for r in range(n_rows):
        top = R.filtered_topk(want[r], set(c['rated'][r].tolist()), K, canonical=True)
        ids[r, :len(top)] = top
        sc[r, :len(top)] = want[r, top]
    c['ids'], c['top'] = ids, sc
    return c


@functools.lru_cache(maxsize=None)
def _k4(name, k, mode, split):
    c = _case(name, k)
    tkr_hip.set_topk_math(mode)
    try:
        ids, sc = tkr_hip.score_topk(c['Ud'], c['Vd'], K, bias=c['bd'], mask=c['mask'], mask_pitch=c['pitch'], want_scores=True, split=split)
        torch.cuda.synchronize()
        return ids.cpu().numpy(), sc.cpu().numpy()
    finally:
        tkr_hip.set_topk_math(tkr_hip.TOPK_MATH_DEFAULT)


def _report(what, got, want):
    bad = np.flatnonzero((got != want).any(axis=1))
    print('%s: %d of %d rows differ from the oracle%s' % (what, len(bad), len(got), '' if not len(bad) else ', first %d: got %s want %s' % (
        bad[0], got[bad[0]].tolist(), want[bad[0]].tolist())))


@pytest.mark.parametrize('name,k', EVERY)
def test_k4_lists_are_the_oracles(name, k):
    """both arithmetic modes, split and unsplit: the ids are R.filtered_topk of the chain's scores on every row, the scores have the
    oracle's bits where it is not NaN and are NaN where it is, a short list ends in -1 / -inf (and a true -inf entry keeps its id), no
    rated id appears, and the four runs are equal to each other"""
    c = _case(name, k)
    n_rows, n_cols = c['want'].shape
    is_rated = np.zeros((n_rows, n_cols + 1), dtype=bool)            # (column n_cols: where the -1 padding points)
    for r in range(n_rows):
        is_rated[r, c['rated'][r]] = True
    n_kept = np.minimum(K, n_cols - np.diff(c['rptr']))
    assert n_kept[NF.SHORT_ROW] == 3 and n_kept[NF.EMPTY_ROW] == 0
    runs = []
    for mode, split in RUNS:
        ids, sc = _k4(name, k, mode, split)
        _report('%s k = %s, %s, split = %s' % (name, k, mode, split), ids, c['ids'])
        runs.append((ids, sc))
    for (mode, split), (ids, sc) in zip(RUNS, runs):
        where = str((name, k, mode, split))
        np.testing.assert_array_equal(ids, c['ids'], err_msg=where)
        assert NF.same_scores(sc, c['top']), where
        pad = np.arange(K)[None, :] >= n_kept[:, None]
        assert np.all(ids[pad] == -1) and np.all(ids[~pad] >= 0) and np.all(sc[pad] == -np.inf), where
        assert not is_rated[np.arange(n_rows)[:, None], ids].any(), where
        np.testing.assert_array_equal(ids, runs[0][0], err_msg=where)
        assert NF.same_scores(sc, runs[0][1]) and NF.same_scores(runs[0][1], sc), where
    if name == 'inf_in' and k != 'split':                             # a true -inf score is an entry, not the padding
        ids, sc = runs[2]
        assert ids[NF.SHORT_ROW, :3].tolist() == c['ids'][NF.SHORT_ROW, :3].tolist() and (sc[NF.SHORT_ROW, 1:3] == -np.inf).all()
        assert (ids[NF.SHORT_ROW, 1:3] >= 0).all()


@pytest.mark.parametrize('name,k', SMALL)
def test_k12_whole_catalogue_lists_are_k4s_and_the_oracles_ranks(name, k):
    """every row lists the whole catalogue: every rank is the oracle's (-1 where the column is rated), every score the chain's, and
    topk_from_ranks gives K4's ids and scores.  The small shape only: at 700 x 20,000 a whole-catalogue list is 14 M entries in rows
    ten times K12's resident length, its quadratic form (include/tkr.h sends such callers to K4 / K8)"""
    c = _case(name, k)
    n_rows, n_cols = c['want'].shape
    ptr, cols = _csr([np.arange(n_cols, dtype=np.int32)] * n_rows)
    s, r = tkr_hip.rank_candidates(c['Ud'], c['Vd'], _dev(ptr), _dev(cols), bias=c['bd'], mask=c['mask'], mask_pitch=c['pitch'])
    ids, top = tkr_hip.topk_from_ranks(_dev(ptr), _dev(cols), s, r, K)
    s, r = s.cpu().numpy().reshape(n_rows, n_cols), r.cpu().numpy().reshape(n_rows, n_cols)
    want_r = np.stack([RO.like_ranks_np(c['want'][row], set(c['rated'][row].tolist()), range(n_cols)) for row in range(n_rows)])
    _report('%s k = %s, K12 ranks' % (name, k), r, want_r)
    np.testing.assert_array_equal(r, want_r)
    for row in range(n_rows):
        assert (r[row, c['rated'][row]] == -1).all()
    assert NF.same_scores(s, c['want'])
    ki, ks = _k4(name, k, 'refine', True)
    np.testing.assert_array_equal(ids.cpu().numpy(), ki)
    assert NF.same_scores(top.cpu().numpy(), ks)


@pytest.mark.parametrize('name,k', EVERY)
def test_k8_like_ranks_are_the_oracles(name, k):
    """likes: K4's list, every NaN, +inf and -inf column of the row, five rated columns.  Every rank is RO.like_ranks_np's; a listed
    like at position p has rank p; in nan_in a like whose score is the NaN 0x7fffffff -- its ordered bits were K8's own "no rank"
    word -- is ranked"""
    c = _case(name, k)
    want = c['want']
    n_rows = want.shape[0]
    ki, _ = _k4(name, k, 'refine', True)
    likes = [NF.likes_of(want[r], c['rated'][r], ki[r]) for r in range(n_rows)]
    lptr, lcols = _csr(likes)
    ranks = tkr_hip.like_ranks(c['Ud'], c['Vd'], _dev(lptr), _dev(lcols), bias=c['bd'], mask=c['mask'], mask_pitch=c['pitch']).cpu().numpy()
    want_ranks = np.concatenate([RO.like_ranks_np(want[r], set(c['rated'][r].tolist()), likes[r].tolist()) for r in range(n_rows)])
    bad = np.flatnonzero(ranks != want_ranks)
    print('%s k = %s: %d of %d like ranks differ from the oracle' % (name, k, len(bad), len(ranks)))
    np.testing.assert_array_equal(ranks, want_ranks)
    listed = 0
    for r in range(n_rows):
        where = {int(col): p for p, col in enumerate(ki[r]) if col >= 0}
        for col, rank in zip(likes[r].tolist(), ranks[lptr[r]:lptr[r + 1]].tolist()):
            if col in where:
                assert rank == where[col], (name, k, r, col)
                listed += 1
    assert listed > 20 * n_rows
    if name == 'nan_in':
        col = c['special'][2]                                        # V holds 0x7fffffff there
        assert (c['V'].view(np.uint32)[col] == 0x7fffffff).any()
        rows = [r for r in range(n_rows) if col in likes[r].tolist() and col not in set(c['rated'][r].tolist())]
        assert len(rows) >= n_rows // 4
        for r in rows:
            assert ranks[lptr[r] + likes[r].tolist().index(col)] >= 0, (k, r)


@pytest.mark.parametrize('name,k', EVERY)
def test_k6_raw_ranks_are_the_oracles(name, k):
    """tkr_raw_ranks on K4's lists equals RO.raw_ranks_np; in nan_in the rows whose eight NaN columns are all rated have them in front
    of their best kept column"""
    c = _case(name, k)
    want = c['want']
    n_rows = want.shape[0]
    ki, _ = _k4(name, k, 'refine', True)
    raw = tkr_hip.raw_ranks(c['Ud'], c['Vd'], _dev(ki), c['rptr_d'], c['rcols_d'], bias=c['bd']).cpu().numpy()
    want_raw = np.stack([RO.raw_ranks_np(want[r], c['rated'][r], ki[r]) for r in range(n_rows)])
    _report('%s k = %s, K6' % (name, k), raw, want_raw)
    np.testing.assert_array_equal(raw, want_raw)
    if name in ('nan_in', 'inf_in'):
        front = [r for r in range(n_rows) if ki[r, 0] >= 0 and np.isfinite(want[r, ki[r, 0]])
                 and (np.isnan(want[r, c['rated'][r]]) | (want[r, c['rated'][r]] == np.inf)).any()]
        assert len(front) >= n_rows // 8
        for r in front:
            n_front = int((np.isnan(want[r, c['rated'][r]]) | (want[r, c['rated'][r]] == np.inf)).sum())
            assert raw[r, 0] >= n_front, (name, k, r)


@pytest.mark.parametrize('name', ['nan_in', 'inf_in'])
def test_cli_on_a_model_with_nan_and_inf(name, tmp_path, capsys):
    """the case's k = 128 tables (300 users x 400 items) with a bias, written by the project's writers, read back by evaluate.py -sl im
    om -M acc: the S.acc lines (K8) equal the plain lines (K4 + K5), and both equal tests/_rank_oracle.metric_lines on the written
    tables"""
    import evaluate as E
    import synth
    import textio
    data, model = str(tmp_path / 'data'), str(tmp_path / 'model')
    r = synth.make_ratings(300, 320, 80, seed=23, mu=3.0, sigma=0.5, min_r=6, max_r=50, om_per_user=4)
    synth.write_dataset(data, r)
    c = NF.case(name, 128, (300, 400))
    os.mkdir(model)
    textio.write_matrix(os.path.join(model, 'final-U.dat'), c['U'], where='host')
    textio.write_matrix(os.path.join(model, 'final-V.dat'), c['V'])
    textio.write_matrix(os.path.join(model, 'final-B.dat'), c['b'].reshape(-1, 1), where='host')
    text = open(os.path.join(model, 'final-V.dat')).read() + open(os.path.join(model, 'final-U.dat')).read()
    assert ('nan' in text) if name == 'nan_in' else ('inf' in text and '-inf' in text)
    capsys.readouterr()
    scs = ['im', 'om']
    got = E.main(['-d', data, '-m', model, '-s', '5', '-t', '30', '-sl'] + scs + ['-M', 'acc'])
    assert capsys.readouterr().out.strip().split('\n') == got and len(got) == 4
    with np.errstate(all='ignore'):
        want = RO.metric_lines(data, model, 0, 5, 30, scs, ['acc'])
    print(got, want)
    assert got[2:] == want
    assert [l.replace('.acc', '', 1) for l in got[2:]] == got[:2]
