"""K23 (the SVM fusion) without a GPU: the ABI and the wrapper's refusals, the command line, and the oracle of tests/_svm_oracle.py
against hand values and against scikit-learn's recorded fits (tests/golden/g10, written by make_g10.py beside it)."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _svm_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_header_binding_and_library_declare_the_svm_entry_points():
    import tkr_hip
    header = open(os.path.join(ROOT, 'include', 'tkr.h')).read()
    declared = re.findall(r'^int(?:32_t|64_t)? (tkr_\w+)\(', header, flags=re.M)
    lib = C.CDLL(tkr_hip.LIB_PATH)
    assert 'tkr_fusion_svm_sums' in declared and 'tkr_fusion_svm_sums' in tkr_hip.EXPORTS
    assert 'tkr_fusion_svm_partial_bytes' in declared and 'tkr_fusion_svm_partial_bytes' in tkr_hip.EXPORTS_I64
    getattr(lib, 'tkr_fusion_svm_sums'), getattr(lib, 'tkr_fusion_svm_partial_bytes')
    slab = int(re.search(r'#define TKR_FUSION_SVM_SLAB (\d+)', header).group(1))
    assert slab == tkr_hip.FUSION_SVM_SLAB and slab % 256 == 0
    assert callable(tkr_hip.fusion_svm_sums)
    assert [tkr_hip.fusion_svm_words(M) for M in (1, 3, 16)] == [3 + 4, 10 + 6, 153 + 19]


def test_every_invalid_argument_is_refused_before_any_device_access():
    import tkr_hip
    lib = C.CDLL(tkr_hip.LIB_PATH)
    slab = tkr_hip.FUSION_SVM_SLAB
    size = lib.tkr_fusion_svm_partial_bytes
    size.restype = C.c_int64
    size.argtypes = [C.c_int64, C.c_int32, C.c_int64]
    assert size(1, 1, 0) == 7 * 8 and size(slab, 3, 0) == 16 * 8 and size(slab + 1, 3, 0) == 2 * 16 * 8
    assert size(2, 16, slab - 1) == 2 * 172 * 8 and size(3 * slab + 5, 16, slab + 1) == 4 * 172 * 8
    for bad in ((0, 3, 0), (10, 0, 0), (10, 17, 0), (10, 3, -1), (2 ** 43, 3, 0)):
        assert size(*bad) == -1, bad
    for n, M, first in ((1, 1, 0), (5 * slab, 4, 7), (3 * slab + 5, 16, slab + 1)):
        assert tkr_hip.fusion_svm_partial_bytes(n, M, first) == tkr_hip.fusion_svm_slabs(n, first) * tkr_hip.fusion_svm_words(M) * 8
    with pytest.raises(tkr_hip.TkrError, match='tkr error -1'):
        tkr_hip.fusion_svm_partial_bytes(0, 3)
    sums = lib.tkr_fusion_svm_sums
    sums.restype = C.c_int
    sums.argtypes = [C.c_void_p, C.c_int64, C.c_int32, C.c_int64, C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p]
    p, odd = 4096, 4100                                               # never dereferenced: every call below fails its checks
    good = dict(D=p, n_rows=100, M=3, first_row=0, W=p, partial=p, partial_bytes=16 * 8, slab_offset=0, out=p, status=p, stream=None)
    for change in (dict(D=None), dict(W=None), dict(partial=None), dict(status=None), dict(M=0), dict(M=17), dict(M=-1), dict(n_rows=0),
                   dict(n_rows=-5), dict(first_row=-1), dict(W=odd), dict(partial=odd), dict(out=odd), dict(status=odd), dict(D=4097),
                   dict(slab_offset=-1), dict(slab_offset=1), dict(partial_bytes=16 * 8 - 1), dict(partial_bytes=-1),
                   dict(first_row=slab - 1), dict(n_rows=slab + 1), dict(n_rows=2 ** 43)):
        assert sums(*dict(good, **change).values()) == -1, change


def test_wrapper_refuses_with_tkr_error_and_without_a_launch():
    import tkr_hip
    D, W = torch.zeros((20, 3)), torch.zeros(4, dtype=torch.float64)
    with pytest.raises(tkr_hip.TkrError, match='D must be torch.float32'):
        tkr_hip.fusion_svm_sums(D.double(), W)
    with pytest.raises(tkr_hip.TkrError, match='D must be contiguous'):
        tkr_hip.fusion_svm_sums(torch.zeros((3, 20)).t(), W)
    with pytest.raises(tkr_hip.TkrError, match='D must have 2 dimensions'):
        tkr_hip.fusion_svm_sums(torch.zeros(20), W)
    with pytest.raises(tkr_hip.TkrError, match='1 .. 16 models'):
        tkr_hip.fusion_svm_sums(torch.zeros((20, 17)), torch.zeros(18, dtype=torch.float64))
    with pytest.raises(tkr_hip.TkrError, match='1 .. 16 models'):
        tkr_hip.fusion_svm_sums(torch.zeros((20, 0)), torch.zeros(1, dtype=torch.float64))
    with pytest.raises(tkr_hip.TkrError, match='at least one row'):
        tkr_hip.fusion_svm_sums(torch.zeros((0, 3)), W)
    with pytest.raises(tkr_hip.TkrError, match='must not be negative'):
        tkr_hip.fusion_svm_sums(D, W, -1)
    with pytest.raises(tkr_hip.TkrError, match='must live on the GPU'):      # host tensors: refused, never handed to the library
        tkr_hip.fusion_svm_sums(D, W)
    with pytest.raises(tkr_hip.TkrError, match='row 12345 of the features'):
        tkr_hip.fusion_svm_check(12345)
    tkr_hip.fusion_svm_check(-1)
    import fusion
    import svmfusion
    assert fusion.METHODS == ('a', 'p', 'b', 'e', 'w') and svmfusion.METHODS == ('s',)


def test_unpack_reads_the_triangle_row_by_row():
    import tkr_hip
    M = 2
    words = tkr_hip.fusion_svm_words(M)
    out = np.arange(1, words + 1, dtype=np.float64)
    out[-1:] = np.array([77], dtype=np.int64).view(np.float64)
    S, r, q, count = tkr_hip.fusion_svm_unpack(out, M)
    assert S.tolist() == [[1, 2, 3], [2, 4, 5], [3, 5, 6]] and r.tolist() == [7, 8, 9] and q == 10 and count == 77


def test_fuse_cli_knows_method_s_and_no_method_x(capsys):
    import fuse
    with pytest.raises(SystemExit):
        fuse.main(['-d', 'nowhere', '-m', 'A', '-o', 'out', '--method', 'x'])
    assert "invalid choice: 'x'" in capsys.readouterr().err
    with pytest.raises(SystemExit):
        fuse.main(['-d', 'nowhere', '-m', 'A', '-o', 'out', '--method', 's', '--svm-c', '0'])
    assert '--svm-c positive' in capsys.readouterr().err
    # 's' passes the parser: what stops the call is the missing GPU or, with one, the missing data directory
    import tkr_hip
    with pytest.raises((tkr_hip.TkrError, OSError)):
        fuse.main(['-d', os.path.join(ROOT, 'nowhere'), '-m', 'A', '-o', 'out', '--method', 's', '--svm-c', '0.5', '--samples', '10'])
    import inspect
    import svmfusion
    kw = {k: v.default for k, v in inspect.signature(svmfusion.learn_svm).parameters.items() if v.default is not inspect.Parameter.empty}
    assert (kw['n_samples'], kw['C'], kw['seed'], kw['max_iter'], kw['want_info'], kw['chunk_bytes']) == (1_000_000, 0.01, 0, 50, False, None)


# ---- the oracle ---------------------------------------------------------------------------------------------------------------------
def test_oracle_sums_by_hand():
    rng = np.random.Generator(np.random.PCG64(1))
    D = rng.standard_normal((7, 3)).astype(np.float32)
    for first in (0, 1):
        X = O.rows(D, first)
        assert X[:, 3].tolist() == ([1, -1, 1, -1, 1, -1, 1] if first == 0 else [-1, 1, -1, 1, -1, 1, -1])
        S, r, q, count = O.sums(D, first, np.zeros(4))               # W = 0: z = 0, every row active with 1 - z = 1
        assert count == 7 and q == 7.0
        np.testing.assert_allclose(r, X.sum(axis=0), rtol=1e-15)
        np.testing.assert_allclose(S, X.T @ X, rtol=1e-14)
        assert S[3, 3] == 7.0
    # rows exactly on the hinge (z = 1) are inactive, rows one ulp inside are active
    D = np.array([[1.0, 0.0], [0.5, 0.25], [0.5, 0.25], [-1.0, 3.0]], dtype=np.float32)
    w = np.array([1.0, 0.0, 0.0])
    assert O.margins(O.rows(D, 0), w).tolist() == [1.0, 0.5, 0.5, -1.0]
    S, r, q, count = O.sums(D, 0, w)
    assert count == 3 and q == 0.25 + 0.25 + 4.0
    assert r.tolist() == [0.5 * 0.5 + 0.5 * 0.5 + 2.0 * -1.0, 0.5 * 0.25 + 0.5 * 0.25 + 2.0 * 3.0, 0.5 * -1 + 0.5 * 1 + 2.0 * -1]
    w = np.array([1.0, 0.0, 2.0 ** -52])                              # row 0 (y = +1): z = 1 + 2^-52, outside; as row 1 (y = -1): z = 1 - 2^-52
    assert O.sums(D[:1], 0, w)[3] == 0 and O.sums(D[:1], 1, w)[3] == 1
    # an empty active set: zeros, not an error
    S, r, q, count = O.sums(D[:1], 0, np.array([5.0, 0.0, 0.0]))
    assert count == 0 and q == 0.0 and not S.any() and not r.any()
    for order in ('backward', 'pairwise'):
        np.testing.assert_allclose(O.sums(D, 0, np.zeros(3), order)[0], O.sums(D, 0, np.zeros(3))[0], rtol=1e-15)


def test_oracle_newton_one_row_in_closed_form():
    """N = 1: the minimiser of |w~|^2 / 2 + C (1 - w~ . x~)^2 is w~ = 2 C x~ / (1 + 2 C |x~|^2)"""
    D = np.array([[0.5, -1.25, 2.0]], dtype=np.float32)
    for C_ in (0.01, 3.0):
        res = O.newton(D, C_)
        x = np.array([0.5, -1.25, 2.0, 1.0])
        np.testing.assert_allclose(res['w'], 2 * C_ * x / (1 + 2 * C_ * x @ x), rtol=1e-14)
        assert res['converged'] and res['iterations'] == 1 and res['active'] == 1


def _golden(golden_dir, tag):
    g = np.load(os.path.join(golden_dir, 'g10', 'expected.npz'))
    tight = np.concatenate([g['tight_coef_' + tag], g['tight_intercept_' + tag]])
    default = np.concatenate([g['default_coef_' + tag], g['default_intercept_' + tag]])
    return g['D_' + tag], float(g['C'][0]), tight, default


# what this oracle measured to scikit-learn's default fit on the two fixtures (max over weights and intercept); asserted with a margin of 4
MEASURED_TO_DEFAULT = {'a': 1.9044e-5, 'b': 2.9936e-6}


@pytest.mark.parametrize('tag,shape', [('a', (501, 3)), ('b', (64, 16))])
def test_oracle_newton_against_scikit_learns_recorded_fits(golden_dir, tag, shape):
    """The tight fit is liblinear's dual coordinate descent stopped at a projected gradient of tol = 1e-12 per coordinate.  The dual is
    strongly convex with modulus 1 / (2 C), so |alpha - alpha*|_2 <= |PG|_2 2 C <= sqrt(N) tol 2 C, and w~ = sum alpha_t x~_t moves by
    at most |X~|_F times that; to this comes the rounding of either side's own sums, 64 N 2^-53 max|w~|.  Measured: 6.6e-14 (501 x 3,
    bound 1.7e-11) and 4.8e-14 (64 x 16, bound 3.2e-12); to the default fit 1.9e-5 and 3.0e-6, i.e. 2.5e-5 and 1.4e-5 of the largest
    weight."""
    D, C_, tight, default = _golden(golden_dir, tag)
    assert D.shape == shape and D.dtype == np.float32 and C_ == 0.01
    res = O.newton(D, C_)
    assert res['converged'] and 1 <= res['iterations'] <= 6
    N = len(D)
    bound = 2 * C_ * 1e-12 * np.sqrt(N) * np.linalg.norm(O.rows(D, 0)) + 64 * N * 2.0 ** -53 * np.abs(tight).max()
    to_tight, to_default = float(np.abs(res['w'] - tight).max()), float(np.abs(res['w'] - default).max())
    print('g10 %s: %d Newton steps, max|g| = %.3g, to the tight fit %.3g (bound %.3g), to the default fit %.3g, max|w~| = %.3g'
          % (tag, res['iterations'], res['grad'], to_tight, bound, to_default, np.abs(tight).max()))
    assert to_tight <= bound
    assert to_default <= 4 * MEASURED_TO_DEFAULT[tag]
    # the three orders of the row sums agree far inside either bound
    for order in ('backward', 'pairwise'):
        assert np.abs(O.newton(D, C_, order=order)['w'] - res['w']).max() <= 64 * N * 2.0 ** -53 * np.abs(tight).max()


def test_module_newton_is_the_oracles_newton(golden_dir):
    """svmfusion.newton on the oracle's sums: the same iterates as the oracle's own loop, bit for bit (both solve H p = -g with
    numpy.linalg.solve and halve the step by the same rule)"""
    import svmfusion
    for tag in ('a', 'b'):
        D, C_, _, _ = _golden(golden_dir, tag)
        want = O.newton(D, C_)
        got = svmfusion.newton(lambda w: O.sums(D, 0, w), D.shape[1], len(D), C_, 50)
        assert np.array_equal(got['w'], want['w']) and got['iterations'] == want['iterations'] and got['grad'] == want['grad']
        assert got['active'] == want['active'] and got['objective'] == want['objective'] and got['converged']
    # max_iter stops it, and says so
    D, C_, _, _ = _golden(golden_dir, 'a')
    cut = svmfusion.newton(lambda w: O.sums(D, 0, w), 3, len(D), C_, 1)
    assert cut['iterations'] == 1 and not cut['converged'] and O.newton(D, C_, max_iter=1)['iterations'] == 1
