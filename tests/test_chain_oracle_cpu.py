"""tests/_chain_oracle.py on the CPU: chain_scores_checked is the library oracle's chain bit for bit, its hazard mark covers every entry
where the oracle's two roundings can differ from the hardware's one (proved against an exact integer chain), and the inputs of
tests/test_gpu_score_chain.py are free of such entries and able to tell the slab-wise summation order from the global one."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _chain_oracle as CO

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
