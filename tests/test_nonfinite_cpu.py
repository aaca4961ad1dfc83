"""Conditions on the inputs of tests/test_gpu_nonfinite_scores.py (tests/_nonfinite_oracle.py), and the project's oracles held to an
independent statement of the contract of include/tkr.h (K4): sorted by (is NaN, score, column), descending."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _chain_oracle as CO
import _nonfinite_oracle as NF
import _rank_oracle as RO

from oracle import ref_np as R

K = NF.TOP
ALL = [(name, k) for name in NF.CASES for k in NF.WIDTHS]


def _unrated(c, r, cols):
    rated = set(c['rated'][r].tolist())
    return [x for x in cols if x not in rated]


@pytest.mark.parametrize('name,k', ALL)
def test_shape_and_rated_sets(name, k):
    c = NF.case(name, k)
    assert c['U'].shape == (NF.N_ROWS, k) and c['V'].shape == (NF.N_COLS, k) and c['b'].shape == (NF.N_COLS,)
    n_rated = np.array([len(x) for x in c['rated']])
    assert n_rated[NF.SHORT_ROW] == NF.N_COLS - 3 and n_rated[NF.EMPTY_ROW] == NF.N_COLS
    others = np.delete(n_rated, [NF.SHORT_ROW, NF.EMPTY_ROW])
    assert others.min() >= 26 and others.max() <= 58 and 35 <= others.mean() <= 48           # "about 40"
    assert all(np.all(np.diff(x) > 0) for x in c['rated'] if len(x) > 1)


@pytest.mark.parametrize('name,k', ALL)
def test_finite_scores_do_not_depend_on_the_order_of_summation(name, k):
    """every finite score of the chain is the float64 dot product (exact: integers times a power of two) rounded once to fp32; no
    rounding hazard of the oracle's double rounding among the finite normal entries"""
    c, s = NF.case(name, k), NF.scores(name, k)
    with np.errstate(all='ignore'):
        d = (c['U'].astype(np.float64) @ c['V'].astype(np.float64).T + c['b'].astype(np.float64)).astype(np.float32) + np.float32(0.0)
        _, hz = CO.chain_scores_checked(c['U'], c['V'], c['b'])
    fin = np.isfinite(s)
    if name not in ('nan_in', 'nan_u', 'inf_in', 'overflow'):
        assert fin.all()
    assert fin.mean() > 0.5
    np.testing.assert_array_equal(s[fin].view(np.uint32), d[fin].view(np.uint32))
    normal = fin & (np.abs(s) >= 2.0 ** -126)
    assert not hz[normal].any()                                      # (the marking gives up below 2^-126; the line above does not)


def test_nan_in_features():
    """per row: 0 unrated NaN columns (rows % 4 == 0), 4 (rows % 4 == 1), 8 (rows % 4 == 3), more than K on the two NaN user rows;
    rated NaN columns; all four payloads in V"""
    for k in NF.WIDTHS:
        c, s = NF.case('nan_in', k), NF.scores('nan_in', k)
        sc = c['special']
        bits = set(int(x) for x in c['V'].view(np.uint32)[np.isnan(c['V'])])
        assert bits == set(NF.NAN_PATTERNS)
        assert np.isnan(c['V']).sum() == 8 and (np.isnan(c['V']).sum(axis=1) <= 1).all()
        nan_rows = np.flatnonzero(np.isnan(c['U']).any(axis=1)).tolist()
        assert nan_rows == [3, NF.N_ROWS - 1] and np.isnan(s[nan_rows]).all()
        counts = {}
        for r in range(NF.N_ROWS):
            n = len(_unrated(c, r, np.flatnonzero(np.isnan(s[r])).tolist()))
            counts.setdefault(n, []).append(r)
            if r not in nan_rows and r not in (NF.SHORT_ROW, NF.EMPTY_ROW):
                assert np.flatnonzero(np.isnan(s[r])).tolist() == sorted(sc)
                assert n == {0: 0, 1: 4, 3: 8}.get(r % 4, n)
        print('k = %d: rows by number of unrated NaN columns: %s' % (k, {n: len(v) for n, v in sorted(counts.items())}))
        assert len(counts[0]) >= 30 and sum(len(v) for n, v in counts.items() if 1 <= n < K) >= 60
        assert sum(len(v) for n, v in counts.items() if n > K) == 2
        assert sum(len(set(c['rated'][r].tolist()) & set(sc)) > 0 for r in range(NF.N_ROWS)) >= 60     # rated NaN columns
    c = NF.split_case('nan_in')                                      # NaN columns in more than one item range of the split launch
    assert len(set(x // 2500 for x in c['special'])) >= 4
    assert np.isnan(c['scores'][:, c['special']]).all()


def test_nan_u_features():
    for k in NF.WIDTHS:
        c, s = NF.case('nan_u', k), NF.scores('nan_u', k)
        assert np.isfinite(c['V']).all() and np.isfinite(c['b']).all()
        assert np.flatnonzero(~np.isfinite(c['U']).all(axis=1)).tolist() == [3, 40, 41, NF.N_ROWS - 1]
        assert np.isnan(s[[3, NF.N_ROWS - 1]]).all() and np.isfinite(np.delete(s, [3, 40, 41, NF.N_ROWS - 1], axis=0)).all()
        assert np.isnan(s[40, c['special'][0]]) and np.isinf(s[40]).sum() > 100 and np.isinf(s[41]).sum() > 100


def test_inf_in_features():
    for k in NF.WIDTHS:
        c, s = NF.case('inf_in', k), NF.scores('inf_in', k)
        sc = c['special']
        assert np.isfinite(c['U']).all() and np.isinf(c['V']).sum() == 10
        n_pinf, n_ninf, n_nan = (s == np.inf).sum(axis=1), (s == -np.inf).sum(axis=1), np.isnan(s).sum(axis=1)
        print('k = %d: rows with +inf ties %d, with -inf %d, with NaN %d' % (k, (n_pinf >= 2).sum(), (n_ninf > 0).sum(), (n_nan > 0).sum()))
        assert (n_pinf >= 3).sum() >= 30 and (n_ninf >= 3).sum() >= 30           # several columns tie at +inf, at -inf
        assert (n_nan > 0).sum() >= 100
        assert np.isnan(s[0, sc[0]]) and np.isnan(s[NF.ZERO_ROWS[0], sc[:3]]).all()      # u == 0 meets inf
        both = s[:, sc[5]]                                                       # both signs in one chain
        assert np.isnan(both).sum() >= 30
        short = NF.SHORT_ROW                                                     # the short row keeps a -inf and a +inf... column
        kept = _unrated(c, short, range(NF.N_COLS))
        assert len(kept) == 3 and s[short, sc[4]] == -np.inf and sc[4] in kept and s[short, sc[1]] == -np.inf and sc[1] in kept
        assert R.filtered_topk(s[short], set(c['rated'][short].tolist()), K)[-1] == sc[1]  # tie at -inf: the higher column (sc[4]) first


def test_overflow_features():
    """finite factors only: +-inf scores, ties at both, a chain in which 2^200 meets -2^200 (the first decides: the steps are fused,
    so no NaN), the bias add that overflows"""
    for k in NF.WIDTHS:
        c, s = NF.case('overflow', k), NF.scores('overflow', k)
        sc = c['special']
        assert np.isfinite(c['U']).all() and np.isfinite(c['V']).all() and np.isfinite(c['b']).all()
        assert not np.isnan(s).any()
        assert ((s == np.inf).sum(axis=1) >= 3).sum() >= 30 and ((s == -np.inf).sum(axis=1) >= 3).sum() >= 30
        with np.errstate(all='ignore'):
            d = c['U'].astype(np.float64) @ c['V'].astype(np.float64).T
        order_matters = np.isinf(s[:, sc[4]]) & (np.abs(d[:, sc[4]]) < 1e30)   # 2^200 - 2^200 in float64, +-inf by the chain
        assert order_matters.sum() >= 10
        assert np.isinf(s[:, sc[6]]).sum() >= 30 and np.isfinite(s[:, sc[6]]).sum() >= 30     # 2^127 + 3e38 / -2^127 + 3e38
        assert np.isinf(s[:, sc[7]]).sum() >= 30


@pytest.mark.parametrize('name', ['huge_u', 'tiny_u'])
def test_row_norms_leave_fp32_but_scores_do_not(name):
    for k in NF.WIDTHS:
        c, s = NF.case(name, k), NF.scores(name, k)
        live = np.delete(np.arange(NF.N_ROWS), NF.ZERO_ROWS)
        with np.errstate(all='ignore'):
            nu = (c['U'] * c['U']).sum(axis=1, dtype=np.float32)[live]
        assert np.isinf(nu).all() if name == 'huge_u' else (nu == 0).all()
        a = np.abs(s[live])
        assert np.isfinite(s).all() and a.max() < 1e6 and a[a > 0].min() > 1e-9


def test_subnormal_features():
    for k in NF.WIDTHS:
        c, s = NF.case('subnormal', k), NF.scores('subnormal', k)
        assert (np.abs(s) < 2.0 ** -126).all()
        q = s.astype(np.float64) * 2.0 ** 149
        assert np.array_equal(q, np.round(q))
        distinct = np.mean([len(np.unique(s[r])) for r in range(NF.N_ROWS) if r not in NF.ZERO_ROWS])
        print('k = %d: %.0f distinct scores per row of %d' % (k, distinct, NF.N_COLS))
        assert distinct >= 0.5 * NF.N_COLS
        assert ((s == 0).sum(axis=1) >= 4).all()                     # exact ties at zero on every row
        z = NF.ZERO_ROWS[0]
        assert (c['V'][c['special'][4]] < 0).all() and s[z, c['special'][4]] == 0      # -0.0 products
        assert not (np.signbit(s) & (s == 0)).any()                  # the oracle's zeros are +0.0


@pytest.mark.parametrize('name,k', ALL)
def test_oracles_state_the_contract(name, k):
    """R.filtered_topk, RO.like_ranks_np and RO.raw_ranks_np equal the order sorted by (is NaN, score, column), descending"""
    c, s = NF.case(name, k), NF.scores(name, k)
    rows = sorted(set(list(range(0, NF.N_ROWS, 9)) + [3, 5, 7, 11, 40, 41, NF.N_ROWS - 1]))
    for r in rows:
        rated = set(c['rated'][r].tolist())
        order = NF.contract_order(s[r])
        kept = [x for x in order if x not in rated]
        assert R.filtered_topk(s[r], rated, K, canonical=True) == kept[:K]
        likes = NF.likes_of(s[r], c['rated'][r], kept[:K])
        pos = {col: p for p, col in enumerate(kept)}
        assert RO.like_ranks_np(s[r], rated, likes.tolist()).tolist() == [pos.get(int(x), -1) for x in likes]
        ids = np.full(K, -1, dtype=np.int32)
        ids[:len(kept[:K])] = kept[:K]
        raw = {col: p for p, col in enumerate(order)}
        assert RO.raw_ranks_np(s[r], rated, ids).tolist() == [raw[int(x)] if x >= 0 else -1 for x in ids]


@pytest.mark.parametrize('name', NF.SPLIT_CASES)
def test_split_scores_are_the_chain(name):
    """the short cut that scores the 700 x 20,000 case equals the chain, bit for bit and NaN for NaN, at the small shape"""
    for k in (50, 64):
        c = NF.case(name, k)
        with np.errstate(all='ignore'):
            assert NF.same_scores(NF.split_scores(c), R.mfma_chain_scores(c['U'], c['V'], c['b']))
    n_rows, n_cols, k = NF.SPLIT
    c = NF.split_case(name)
    assert c['scores'].shape == (n_rows, n_cols) and c['U'].shape[1] == k
    assert (~np.isfinite(c['scores'])).any(axis=1).sum() >= (4 if name == 'nan_u' else 0.7 * n_rows)


def test_same_scores_tells_nan_from_bits():
    a = np.array([1.0, np.nan, -0.0], dtype=np.float32)
    assert NF.same_scores(a, np.array([1.0, NF.nan32(0xffc00001), -0.0], dtype=np.float32))
    assert not NF.same_scores(a, np.array([1.0, np.nan, 0.0], dtype=np.float32))
    assert not NF.same_scores(a, np.array([1.0, np.inf, -0.0], dtype=np.float32))
