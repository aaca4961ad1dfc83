"""tests/_chain_oracle.py on the CPU: chain_scores_checked is the library oracle's chain bit for bit, its hazard mark covers every entry
where the oracle's two roundings can differ from the hardware's one (proved against an exact integer chain), and the inputs of
tests/test_gpu_score_chain.py are free of such entries and able to tell the slab-wise summation order from the global one; the
mirror-pair inputs of the K6 tests (tests/test_gpu_utils_eval.py) tie exactly in integer arithmetic, carry no hazard entry and tell
another order of summation from the chain in the raw ranks; tests/_rank_oracle.raw_ranks_np agrees with the library oracle."""
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _chain_oracle as CO
import _rank_oracle as RO

from oracle import ref_np as R

F32 = np.float32


def _bits(a):
    return np.ascontiguousarray(a, dtype=F32).view(np.uint32)


@pytest.mark.parametrize('k', CO.WIDTHS)
def test_checked_scores_are_the_library_oracle_and_non_hazard_entries_equal_the_exact_chain(k):
    """on the input set of the GPU test: the scores are R.mfma_chain_scores' bits, with and without bias; 200 sampled entries that carry
    no hazard mark equal the integer chain (one rounding per step) bit for bit"""
    c = CO.case(k)
    U, V, b = c['rows'], c['V'], c['b']
    s, hz = CO.chain_scores_checked(U, V, b)
    np.testing.assert_array_equal(_bits(s), _bits(R.mfma_chain_scores(U, V, b)))
    s0, _ = CO.chain_scores_checked(U, V, None, chunk=5000)          # several column chunks
    np.testing.assert_array_equal(_bits(s0), _bits(R.mfma_chain_scores(U, V, None)))
    rng = np.random.Generator(np.random.PCG64(k))
    checked = 0
    for r, col in zip(rng.integers(0, U.shape[0], 200), rng.integers(0, V.shape[0], 200)):
        if not hz[r, col]:
            assert _bits(CO.exact_chain_score(U[r], V[col], b[col])) == _bits(s[r, col]), (k, r, col)
            checked += 1
    assert checked >= 190


def test_round_to_f32_ties_to_even_and_subnormals():
    for n, e, want in ((1, 0, 1.0), ((1 << 24) + 1, 0, float(1 << 24)), ((1 << 24) + 3, 0, float((1 << 24) + 4)),
                       ((1 << 25) + 2, -3, float((1 << 22))), ((1 << 25) + 6, -3, float((1 << 22) + 1)), (-((1 << 24) + 3), 5, -float(((1 << 24) + 4) << 5)),
                       (3, -150, 2.0 ** -148), (1, -150, 0.0), (5, -151, 2.0 ** -149)):
        q, f = CO.round_to_f32(n, e)
        assert np.ldexp(float(q), f) == want, (n, e)
        assert F32(np.ldexp(float(n), e)) == F32(want)                # numpy's own single rounding of the same dyadic value


def test_a_hand_built_tie_is_flagged_and_is_where_two_roundings_differ():
    """acc = 1 + 2^-23 after the first step; the second product is (2^-12 + 2^-27)(2^-12 - 2^-27) = 2^-24 - 2^-54: the exact sum lies
    just below the tie between 1 + 2^-23 and 1 + 2^-22 and rounds down; its float64 rounding lies ON the tie and rounds to even, up.
    The mark is set, the oracle differs from the exact chain there, and the unmarked neighbour entries still agree."""
    U = np.array([[1.0, 2.0 ** -12 + 2.0 ** -27], [1.0, 2.0 ** -12]], dtype=F32)
    V = np.array([[1.0 + 2.0 ** -23, 2.0 ** -12 - 2.0 ** -27], [1.0, 0.5]], dtype=F32)
    s, hz = CO.chain_scores_checked(U, V)
    np.testing.assert_array_equal(_bits(s), _bits(R.mfma_chain_scores(U, V)))
    assert hz.tolist() == [[True, False], [False, False]]
    assert s[0, 0] == F32(1.0 + 2.0 ** -22) and CO.exact_chain_score(U[0], V[0]) == F32(1.0 + 2.0 ** -23)
    for r, col in ((0, 1), (1, 0), (1, 1)):
        assert _bits(CO.exact_chain_score(U[r], V[col])) == _bits(s[r, col])
    # the same tie reached exactly (product 2^-24): both roundings go to even, no hazard
    s2, hz2 = CO.chain_scores_checked(np.array([[1.0, 2.0 ** -12]], dtype=F32), np.array([[1.0, 2.0 ** -12]], dtype=F32))
    assert not hz2.any() and s2[0, 0] == F32(1.0) == CO.exact_chain_score([1.0, 2.0 ** -12], [1.0, 2.0 ** -12])


@pytest.mark.parametrize('k', CO.WIDTHS + ['big'])
def test_gpu_test_inputs_are_free_of_hazards(k):
    """a condition on the inputs tests/test_gpu_score_chain.py uses (same seeds, same generator): at most a 1e-4 share of hazard
    entries, so that the bit comparison there covers the lists"""
    c = CO.case(CO.BIG[2], CO.BIG[:2]) if k == 'big' else CO.case(k)
    _, hz = CO.chain_scores_checked(c['rows'], c['V'], c['b'])
    print('k = %s: %d hazard entries of %d' % (k, int(hz.sum()), hz.size))
    assert hz.mean() <= 1e-4


# ---- the mirror-pair inputs (CO.mirror_case): conditions on the inputs alone, which the K6 tests of tests/test_gpu_utils_eval.py rest on --
@functools.lru_cache(maxsize=None)
def _mirror(k):
    c = CO.mirror_case(k)
    s, hz = CO.chain_scores_checked(c['rows'], c['V'], c['b'])
    for a in (s, hz):
        a.setflags(write=False)
    return c, s, hz


def _as_ints(a):
    """float32 array -> object array of Python integers, a * 2^64: every '%f'-rounded value of the inputs (0 or |x| >= 1e-6, ulp >=
    2^-43) is a whole multiple of 2^-64"""
    x = np.asarray(a, dtype=np.float64) * 2.0 ** 64
    assert np.all(x == np.rint(x))
    return np.vectorize(int, otypes=[object])(x)


@pytest.mark.parametrize('k', CO.MIRROR_WIDTHS)
def test_mirror_pairs_tie_exactly_and_carry_no_hazard(k):
    """the structure that makes every pair a tie in real arithmetic holds entry by entry -- palindromic user rows, column c + m = column
    c read backwards, equal biases, so the two scores add the same products -- and, in integer arithmetic, the scores of every pair are
    equal for five whole rows; no entry of the oracle is marked a hazard (the other chain inputs allow a 1e-4 share: here none, the GPU
    tests skip nothing); the rated lists have the three special rows and many pairs with exactly one column rated"""
    c, s, hz = _mirror(k)
    U, V, b, m = c['rows'], c['V'], c['b'], CO.MIRROR_M
    assert U.shape == (CO.MIRROR_ROWS, k) and V.shape == (2 * m, k)
    np.testing.assert_array_equal(_bits(U), _bits(U[:, ::-1]))
    np.testing.assert_array_equal(_bits(V[m:]), _bits(V[:m, ::-1]))
    np.testing.assert_array_equal(_bits(b[m:]), _bits(b[:m]))
    rows = [0, 1, 2, 30, CO.MIRROR_ROWS - 1]
    exact = _as_ints(U[rows]).dot(_as_ints(V).T) + _as_ints(b).reshape(1, -1) * (1 << 64)
    assert np.all(exact[:, :m] == exact[:, m:])
    assert float(np.abs(exact.astype(np.float64) * 2.0 ** -128 - s[rows]).max()) < 1e-6        # ... and they are these scores
    print('k = %d: %d hazard entries of %d' % (k, int(hz.sum()), hz.size))
    assert not hz.any()
    rated = c['rated']
    assert len(rated[0]) == 0 and len(rated[1]) == 2 * m - 3 and len(rated[2]) == 2 * m
    is_rated = np.zeros((len(rated), 2 * m), dtype=bool)
    for r, cols in enumerate(rated):
        assert np.all(np.diff(cols) > 0)
        is_rated[r, cols] = True
    assert (is_rated[3:, :m] != is_rated[3:, m:]).mean() > 0.4
    if c['user_idx'] is not None:
        assert k == CO.IDX_WIDTH and c['U'].shape[0] > U.shape[0] and len(set(c['user_idx'].tolist())) == U.shape[0] - 1
    assert (CO.mirror_case(CO.IDX_WIDTH)['user_idx'] is not None)


@pytest.mark.parametrize('k', CO.MIRROR_WIDTHS)
def test_mirror_scores_equal_the_exact_chain_on_a_sample_of_pairs(k):
    c, s, hz = _mirror(k)
    U, V, b, m = c['rows'], c['V'], c['b'], CO.MIRROR_M
    rng = np.random.Generator(np.random.PCG64(9200 + k))
    for r, col in zip(rng.integers(0, U.shape[0], 12), rng.integers(0, m, 12)):
        for cc in (col, col + m):
            assert _bits(CO.exact_chain_score(U[r], V[cc], b[cc])) == _bits(s[r, cc]), (k, r, cc)


E2E_WIDTHS = (128, 300, 1032)                # test_get_score_and_evaluate_on_the_chain compares sums over all rows: no hazard entry at all


@pytest.mark.parametrize('k', CO.MIRROR_WIDTHS)
def test_generic_inputs_of_the_k6_tests_and_the_bias_added_afterwards(k):
    """the generic sets CO.case(k) at the widths of the K6 tests: at most a 1e-4 share of hazard entries (their rows are left out
    there), none at the widths of the end-to-end test; and the scores with bias are the scores without it plus one fp32 add, -0.0 ->
    +0.0, which is how tests/test_gpu_utils_eval.py gets both from one run of the chain"""
    c = CO.case(k)
    s0, hz0 = CO.chain_scores_checked(c['rows'], c['V'], None)
    sb, hzb = CO.chain_scores_checked(c['rows'], c['V'], c['b'])
    print('k = %d: %d hazard entries of %d, in %d rows' % (k, int(hz0.sum()), hz0.size, int(hz0.any(axis=1).sum())))
    assert hz0.mean() <= 1e-4 and hz0.any(axis=1).mean() <= 0.1
    assert k not in E2E_WIDTHS or not hz0.any()
    np.testing.assert_array_equal(hz0, hzb)
    np.testing.assert_array_equal(_bits((s0 + c['b'].reshape(1, -1)).astype(F32) + F32(0.0)), _bits(sb))


def _counted_ranks(scores_row, rated, kept):
    """K6's definition on any scores: position in the kept list + the rated columns in front under the canonical order"""
    sk, sr = scores_row[kept][:, None], scores_row[rated][None, :]
    front = (sr > sk) | ((sr == sk) & (rated[None, :] > kept[:, None]))
    return np.arange(len(kept)) + front.sum(axis=1)


@pytest.mark.parametrize('k', [k for k in CO.MIRROR_WIDTHS if k >= 50])
def test_mirror_inputs_tell_summation_orders_apart_in_the_raw_ranks(k):
    """at every width from 50 on: the chain gives the two columns of at least 10 % of the pairs different bits; and a raw-rank kernel
    that scored with another order of summation -- here plain left to right -- while the kept list comes from the chain would return
    other raw ranks for at least 1 % of the entries of the top-256 lists.  The GPU tests compare every entry without allowance, so such
    a kernel cannot pass them."""
    c, s, hz = _mirror(k)
    m = CO.MIRROR_M
    apart = float((_bits(s[:, :m]) != _bits(s[:, m:])).mean())
    alt = CO.left_to_right_scores(c['rows'], c['V'], c['b'])
    differ = total = rows_hit = 0
    for r in range(s.shape[0]):
        kept = RO.kept_order(s[r], c['rated'][r])[:256]
        if len(kept) == 0:
            continue
        want = RO.raw_ranks_np(s[r], c['rated'][r], kept)
        np.testing.assert_array_equal(want, _counted_ranks(s[r], c['rated'][r], kept))         # the two definitions agree on one score
        n = int((want != _counted_ranks(alt[r], c['rated'][r], kept)).sum())
        differ, total, rows_hit = differ + n, total + len(kept), rows_hit + (n > 0)
    print('k = %d: %.1f %% of the pairs apart in chain bits; %d of %d raw-rank entries differ under a left-to-right sum, in %d rows'
          % (k, 100 * apart, differ, total, rows_hit))
    assert apart >= 0.10
    assert differ >= 0.01 * total


def test_raw_ranks_np_agrees_with_the_library_oracles_utils_evaluate():
    """hits and reciprocal ranks rebuilt from RO.raw_ranks_np on the kept lists equal R.utils_evaluate(canonical=True) on the same
    scores: mirror inputs at k = 50, one like per pair, (step, total) = (7, 64)"""
    c, s, _ = _mirror(50)
    n_rows, n_cols = s.shape
    rng = np.random.Generator(np.random.PCG64(9300))
    uids = {'u%d' % r: r for r in range(n_rows)}
    te_iids = {'i%d' % x: x for x in range(n_cols)}
    te_ivt = {x: t for t, x in te_iids.items()}
    rated = {'u%d' % r: set('i%d' % x for x in c['rated'][r]) for r in range(n_rows)}
    likes = {'u%d' % r: set('i%d' % x for x in rng.choice(n_cols, 40, replace=False)) for r in range(n_rows)}
    step, total = 7, 64
    interval = total // step
    hits, trrs = [0.0] * interval, [0.0] * interval
    for r in range(n_rows):
        kept = RO.kept_order(s[r], c['rated'][r])[:total]
        for col, t in zip(kept, RO.raw_ranks_np(s[r], c['rated'][r], kept)):
            if 'i%d' % col in likes['u%d' % r]:
                for q in range(int(t) // step, interval):
                    hits[q] += 1
                    trrs[q] += 1.0 / (int(t) + 1)
    eh, er, ec = R.utils_evaluate(s, rated, likes, uids, te_iids, te_ivt, step, total, interval, canonical=True)
    assert hits == eh and sum(eh) > 0 and ec == 40 * n_rows
    np.testing.assert_allclose(trrs, er, rtol=1e-12)


@pytest.mark.parametrize('k', CO.SLAB_WIDTHS)
def test_inputs_tell_the_slab_order_from_the_global_order(k):
    """the halves interleaved inside every 256 factors against the halves of ceil(k / 2): the two chains differ in bits on these inputs
    -- in 38 % (k = 257) to 78 % (k = 768) of the entries; the bias add, to a coarser ulp, hides the rest.  The GPU test compares 3,900
    returned scores per width without allowance: a tenth of them differing is hundreds of failures, so a kernel on the slab-wise order
    cannot pass tests/test_gpu_score_chain.py"""
    c = CO.case(k)
    g, _ = CO.chain_scores_checked(c['rows'], c['V'], c['b'])
    s, _ = CO.chain_scores_checked(c['rows'], c['V'], c['b'], order='slabs')
    share = float((_bits(g) != _bits(s)).mean())
    print('k = %d: %.1f %% of the score bits differ between the two orders' % (k, 100 * share))
    assert share > 0.1
    # ... and by no more than two chains of k + 1 roundings can: each is within (k + 1) 2^-24 (sum |u v| + |b|) of the exact score
    absum = np.abs(c['rows']).astype(np.float64) @ np.abs(c['V']).astype(np.float64).T + np.abs(c['b']).astype(np.float64)
    assert np.all(np.abs(s.astype(np.float64) - g) <= 2 * (k + 1) * 2.0 ** -24 * 1.01 * absum)
    assert sorted(CO.chain_order(k, 'slabs')) == sorted(CO.chain_order(k)) == list(range(k))
