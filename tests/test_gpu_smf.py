"""K27 on the GPU (csrc/smf.hip, top-k-rec_amd/smf.py) against tests/_smf_oracle.py.

The yardstick is the project's own (tests/test_gpu_lmf.py): with x64 the float64 oracle on the same fp32 inputs and x32 the float32 one
in the kernels' order, e32 = max|x32 - x64| / max|x64| per case, and the kernel has to stay within F * max(e32, 2^-23); F = 16 is a
condition of the design, not a knob.  Every ratio is printed; DESIGN.md section 4 K27 keeps the worst.

The exact tests need no yardstick: exp(+0.0) is 1.0f and exp(-inf) is +0, so with scores of exactly 0 and column offsets of 0 or +inf
D is a sum of rows of Y, and with Y small integers times 2^-6 every order of that sum gives the same bits."""
import ctypes as C
import functools
import os

import numpy as np
import pytest
import torch

import _smf_oracle as O

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = 16.0
FLOOR = 2.0 ** -23
SLAB = O.SLAB
KS = (2, 31, 129)                                                # widths of the tables, K = k + 1
NO_HEAVY = O.NO_HEAVY


def _dev(a):
    return torch.from_numpy(np.array(a, order='C')).cuda()


def _bits(a):
    return np.ascontiguousarray(a).view(np.int32 if a.dtype == np.float32 else np.int64)


def _ratio(got, x64, x32):
    scale = np.abs(x64).max()
    err, e32 = np.abs(got - x64).max() / scale, np.abs(x32 - x64).max() / scale
    return err / max(e32, FLOOR), err, e32


def _held(what, got, x64, x32):
    ratio, err, e32 = _ratio(np.asarray(got, dtype=np.float64), np.asarray(x64, dtype=np.float64), np.asarray(x32, dtype=np.float64))
    print('K27 %s: err %.3g e32 %.3g ratio %.3g' % (what, err, e32, ratio))
    assert ratio <= F, (what, err, e32)
    return ratio


# ---- 1. the dense kernel, exact ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('K', KS)
def test_dense_is_exact_where_p_is_one(K):
    """X = 0 and no offsets: every P is exp(+0.0) = 1.0f; Y small integers times 2^-6: D = the column sums, bit for bit, in every row"""
    import tkr_hip
    rng = np.random.Generator(np.random.PCG64([1, K]))
    for n_y in (1, 31, 32, 33, SLAB, SLAB + 1):
        Y = (rng.integers(-3, 4, (n_y, K)) / 64).astype(np.float32)
        want = np.zeros(K, dtype=np.float32)
        for row in Y:                                             # the NumPy chain
            want += row
        Yd = _dev(Y)
        for n_x in (1, 129):
            D = tkr_hip.smf_dense_rows(torch.zeros((n_x, K), dtype=torch.float32, device='cuda'), Yd).cpu().numpy()
            np.testing.assert_array_equal(_bits(D), _bits(np.broadcast_to(want, (n_x, K))), err_msg='n_x = %d, n_y = %d' % (n_x, n_y))
            lse = tkr_hip.smf_lse_rows(torch.zeros((n_x, K), dtype=torch.float32, device='cuda'), Yd).cpu().numpy()
            assert np.abs(lse - np.log(n_y)).max() <= 4 * FLOOR * max(np.log(n_y), 1), (n_x, n_y)


@pytest.mark.parametrize('K', KS)
def test_column_offset_of_infinity_removes_the_row_bit_for_bit(K):
    """col_off = +inf on half the rows of Y removes exactly those, though they hold +-1e30 and their scores are of that size: P is
    exp(-inf) = +0 and 0 * 1e30 = 0.  The rows that stay have column 0 zero, the only column X is not zero in: their scores are 0"""
    import tkr_hip
    rng = np.random.Generator(np.random.PCG64([2, K]))
    for n_x, n_y in ((33, 100), (129, SLAB + 1)):
        gone = rng.permutation(n_y) < n_y // 2
        Y = (rng.integers(-3, 4, (n_y, K)) / 64).astype(np.float32)
        Y[:, 0] = 0
        Y[gone] = (rng.integers(0, 2, (int(gone.sum()), K)) * 2 - 1) * np.float32(1e30)
        X = np.zeros((n_x, K), dtype=np.float32)
        X[:, 0] = rng.integers(1, 4, n_x) / 64
        off = np.where(gone, np.inf, 0).astype(np.float32)
        want = np.zeros(K, dtype=np.float32)
        for row in Y[~gone]:
            want += row
        S = X.astype(np.float64) @ Y.astype(np.float64).T
        assert np.isfinite(S).all() and (np.abs(S[:, gone]) > 1e27).all() and not S[:, ~gone].any()
        D = tkr_hip.smf_dense_rows(_dev(X), _dev(Y), col_off=_dev(off)).cpu().numpy()
        np.testing.assert_array_equal(_bits(D), _bits(np.broadcast_to(want, (n_x, K))), err_msg='%d x %d' % (n_x, n_y))
        # ... and a row offset of +inf empties the row of D
        ro = np.where(np.arange(n_x) % 3 == 0, np.inf, 0).astype(np.float32)
        D = tkr_hip.smf_dense_rows(_dev(X), _dev(Y[~gone]), row_off=_dev(ro)).cpu().numpy()
        np.testing.assert_array_equal(_bits(D), _bits(np.where(ro[:, None] > 0, np.float32(0), want[None, :])))


# ---- 2. lse and dense, generic ----------------------------------------------------------------------------------------------------------
N_X = 130


@functools.lru_cache(maxsize=None)
def _generic(K, n_y):
    """-> (X, Y, row_off, col_off, lse64, lse32): normal(0, 0.5) tables; row_off = the rounded lse (so that P is the softmax), col_off
    normal(0, 1) with one +inf in seven"""
    rng = np.random.Generator(np.random.PCG64([3, K, n_y]))
    X = (rng.standard_normal((N_X, K)) * 0.5).astype(np.float32)
    Y = (rng.standard_normal((n_y, K)) * 0.5).astype(np.float32)
    lse64, lse32 = O.lse_rows(X, Y), O.lse_rows(X, Y, dtype=np.float32)
    ro = lse64.astype(np.float32)
    co = rng.standard_normal(n_y).astype(np.float32)
    co[rng.permutation(n_y)[:n_y // 7]] = np.inf
    out = (X, Y, ro, co, lse64, lse32)
    for a in out:
        a.flags.writeable = False
    return out


@pytest.mark.parametrize('n_y', [33, SLAB + 1, 8200])
@pytest.mark.parametrize('K', KS)
def test_lse_against_the_oracle(K, n_y):
    import tkr_hip
    X, Y, _, _, lse64, lse32 = _generic(K, n_y)
    lse = tkr_hip.smf_lse_rows(_dev(X), _dev(Y)).cpu().numpy()
    assert lse.dtype == np.float32 and lse.shape == (N_X,)
    _held('lse K=%d n_y=%d' % (K, n_y), lse, lse64, lse32)


@pytest.mark.parametrize('offsets', ['row', 'col', 'both'])
@pytest.mark.parametrize('n_y', [33, SLAB + 1, 8200])
@pytest.mark.parametrize('K', KS)
def test_dense_against_the_oracle(K, n_y, offsets):
    import tkr_hip
    X, Y, ro, co, _, _ = _generic(K, n_y)
    ro, co = (ro if offsets != 'col' else None), (co if offsets != 'row' else None)
    D64, D32 = O.dense_rows(X, Y, ro, co), O.dense_rows(X, Y, ro, co, dtype=np.float32)
    D = tkr_hip.smf_dense_rows(_dev(X), _dev(Y), row_off=None if ro is None else _dev(ro), col_off=None if co is None else _dev(co))
    _held('dense K=%d n_y=%d offsets=%s' % (K, n_y, offsets), D.cpu().numpy(), D64, D32)


def test_scores_of_magnitude_1e4():
    """tables of multiples of 16: every score is a multiple of 256 of size up to 7e4 and exact in fp32.  The lse is finite and holds to
    the oracle; with it as row offset the sum of P over the catalogue -- column K - 1 of D, where Y holds ones and X zeros -- is 1
    within the yardstick of that sum: x64 = 1, x32 = the float32 restatement's sum (an lse of 5e4 is rounded to 4e-3)"""
    import tkr_hip
    K, n_y = 31, SLAB + 1
    rng = np.random.Generator(np.random.PCG64(4))
    X = (rng.integers(-3, 4, (N_X, K)) * 16).astype(np.float32)
    Y = (rng.integers(-3, 4, (n_y, K)) * 16).astype(np.float32)
    X[:, K - 1], Y[:, K - 1] = 0, 1
    S = X.astype(np.float64) @ Y.astype(np.float64).T
    assert 1e4 < np.abs(S).max() < 1e5 and np.abs(S).max(axis=1).min() > 5e3
    Xd, Yd = _dev(X), _dev(Y)
    lse = tkr_hip.smf_lse_rows(Xd, Yd)
    lse64, lse32 = O.lse_rows(X, Y), O.lse_rows(X, Y, dtype=np.float32)
    got = lse.cpu().numpy()
    assert np.isfinite(got).all()
    _held('lse at |s| = 1e4', got, lse64, lse32)
    D = tkr_hip.smf_dense_rows(Xd, Yd, row_off=lse).cpu().numpy()
    assert np.isfinite(D).all()
    D32 = O.dense_rows(X, Y, row_off=lse32, dtype=np.float32)
    _held('sum of P at |s| = 1e4', D[:, K - 1], np.ones(N_X), D32[:, K - 1])
    _held('dense at |s| = 1e4', D, O.dense_rows(X, Y, row_off=got), O.dense_rows(X, Y, row_off=got, dtype=np.float32))


# ---- 3. repeatability -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('K', [31, 129])
def test_bits_are_a_function_of_the_row(K):
    """300 rows against two slabs: a second run, the same rows in reversed order, and single rows alone give the same bits"""
    import tkr_hip
    X0, Y, _, co, _, _ = _generic(K, SLAB + 1)
    rng = np.random.Generator(np.random.PCG64([5, K]))
    X = np.concatenate([X0, (rng.standard_normal((300 - N_X, K)) * 0.5).astype(np.float32)])
    ro = (8 + rng.standard_normal(300)).astype(np.float32)
    Yd, cod = _dev(Y), _dev(co)
    run = lambda x, r: (tkr_hip.smf_lse_rows(_dev(x), Yd).cpu().numpy(), tkr_hip.smf_dense_rows(_dev(x), Yd, row_off=_dev(r), col_off=cod).cpu().numpy())
    lse, D = run(X, ro)
    lse2, D2 = run(X, ro)
    np.testing.assert_array_equal(_bits(lse), _bits(lse2))
    np.testing.assert_array_equal(_bits(D), _bits(D2))
    lse_r, D_r = run(X[::-1], ro[::-1])
    np.testing.assert_array_equal(_bits(lse_r[::-1]), _bits(lse))
    np.testing.assert_array_equal(_bits(D_r[::-1]), _bits(D))
    for r in (0, 31, 128, 299):
        lse1, D1 = run(X[r:r + 1], ro[r:r + 1])
        np.testing.assert_array_equal(_bits(lse1), _bits(lse[r:r + 1]), err_msg='row %d alone' % r)
        np.testing.assert_array_equal(_bits(D1[0]), _bits(D[r]), err_msg='row %d alone' % r)


# ---- 4. the step kernel -----------------------------------------------------------------------------------------------------------------
STEP = dict(lam=0.1, lr=0.3)


@functools.lru_cache(maxsize=None)
def _step_case(k):
    out = O.step_inputs(k)
    for a in (out[0], out[1], out[2], out[4]):
        a.flags.writeable = False
    return out


@pytest.mark.parametrize('heavy_from', [300, NO_HEAVY])
@pytest.mark.parametrize('k', [1, 30, 128])
def test_step_rows_against_the_oracle(k, heavy_from):
    import tkr_hip
    X0, H0, Y, rows, D = _step_case(k)
    assert {0, 1, 700} <= {len(r) for r in rows}
    ptr, cols = O.to_csr(rows)
    Yd, Dd, pd, cd = _dev(Y), _dev(D), _dev(ptr), _dev(cols)
    for fixed in (k, -1):
        for scale in (True, False):
            hyper = dict(fixed=fixed, scale_by_likes=scale, **STEP)
            x64, h64, l64 = O.step_rows(X0, H0, Y, D, rows, **hyper)
            x32, h32, l32 = O.step_rows(X0, H0, Y, D, rows, dtype=np.float32, heavy_from=heavy_from, **hyper)
            X, H = _dev(X0), _dev(H0)
            loss = tkr_hip.smf_step_rows(Yd, Dd, pd, cd, X, H, heavy_from=heavy_from, want_loss=True, **hyper)
            X, H, loss = X.cpu().numpy(), H.cpu().numpy(), loss.cpu().numpy()
            tag = 'k=%d fixed=%d scale=%d heavy_from=%s' % (k, fixed, scale, 'none' if heavy_from == NO_HEAVY else heavy_from)
            _held('step x ' + tag, X, x64, x32)
            _held('step h ' + tag, H, h64, h32)
            _held('step row loss ' + tag, loss, l64, l32)
            if fixed >= 0:
                np.testing.assert_array_equal(_bits(X[:, fixed]), _bits(X0[:, fixed]))
                np.testing.assert_array_equal(_bits(H[:, fixed]), _bits(H0[:, fixed]))
            else:
                assert (X[:, k] != X0[:, k]).all() and (H[:, k] > H0[:, k]).all()
            assert (X[:, :k] != X0[:, :k]).any(axis=1).all()          # a row without likes steps too: D and the regulariser


# ---- 5. refusals ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('heavy_from', [300, NO_HEAVY])
def test_like_columns_outside_the_table_are_skipped(heavy_from):
    import tkr_hip
    k = 33
    X0, H0, Y, rows, D = _step_case(k)
    n_y = len(Y)
    dirty = [np.asarray(x, dtype=np.int64) for x in rows]
    dirty[3] = np.concatenate([dirty[3][:3], [-1], dirty[3][3:], [n_y]])       # 7 likes and two refused
    dirty[2] = np.concatenate([[n_y], dirty[2]])
    dirty[6] = np.concatenate([dirty[6][:270], [-1, -1], dirty[6][270:]])      # in the second slab of a heavy row
    dirty[8] = np.asarray([-1, n_y])                                            # nothing left: as a row without likes
    ptr, cols = O.to_csr(dirty)
    hyper = dict(fixed=k, scale_by_likes=False, **STEP)                         # (with scale_by_likes the weight is what the row STORES)
    X, H = _dev(X0), _dev(H0)
    loss, status = tkr_hip.smf_step_rows(_dev(Y), _dev(D), _dev(ptr), _dev(cols), X, H, heavy_from=heavy_from, want_loss=True, check=False, **hyper)
    assert int(status.item()) == 4 * 2 + 1
    x64, h64, l64 = O.step_rows(X0, H0, Y, D, rows, **hyper)
    x32, h32, l32 = O.step_rows(X0, H0, Y, D, rows, dtype=np.float32, heavy_from=heavy_from, **hyper)
    _held('step x with refused columns', X.cpu().numpy(), x64, x32)
    _held('step row loss with refused columns', loss.cpu().numpy(), l64, l32)
    with pytest.raises(tkr_hip.SmfRefused) as info:
        tkr_hip.smf_step_rows(_dev(Y), _dev(D), _dev(ptr), _dev(cols), _dev(X0), _dev(H0), heavy_from=heavy_from, **hyper)
    assert (info.value.row, info.value.kind) == (2, 1)


@pytest.mark.parametrize('heavy_from', [300, NO_HEAVY])
def test_descending_like_ptr_leaves_the_row(heavy_from):
    import tkr_hip
    k = 16
    X0, H0, Y, rows, D = _step_case(k)
    ptr, cols = O.to_csr(rows)
    good = ptr.copy()
    ptr[6] = ptr[5] - 1                                                         # row 5 descends; row 6 is a row again, longer by what row 5 had
    Yd, Dd = _dev(Y), _dev(D)
    hyper = dict(fixed=-1, scale_by_likes=True, heavy_from=heavy_from, **STEP)
    X, H = _dev(X0), _dev(H0)
    loss, status = tkr_hip.smf_step_rows(Yd, Dd, _dev(ptr), _dev(cols), X, H, want_loss=True, check=False, **hyper)
    assert int(status.item()) == 4 * 5 + 3
    X, H = X.cpu().numpy(), H.cpu().numpy()
    np.testing.assert_array_equal(_bits(X[5]), _bits(X0[5]))
    np.testing.assert_array_equal(_bits(H[5]), _bits(H0[5]))
    assert loss[5].item() == 0.0 and np.isfinite(X).all()
    assert all((X[r] != X0[r]).any() for r in range(len(rows)) if r != 5)
    for at, value, word in ((1, 3, 4 * 1 + 3), (len(good) - 1, len(cols) + 1, 4 * (len(rows) - 1) + 3)):      # row 1 ends past row 2's end; past the end
        bad_ptr = good.copy()
        bad_ptr[at] = value
        _, status = tkr_hip.smf_step_rows(Yd, Dd, _dev(bad_ptr), _dev(cols), _dev(X0), _dev(H0), check=False, **hyper)
        assert int(status.item()) == word
    bad_ptr = good.copy()
    bad_ptr[0] = 1                                                              # does not start at 0
    with pytest.raises(tkr_hip.SmfRefused) as info:
        tkr_hip.smf_step_rows(Yd, Dd, _dev(bad_ptr), _dev(cols), _dev(X0), _dev(H0), **hyper)
    assert (info.value.row, info.value.kind) == (0, 3)


def _raw():
    lib = C.CDLL(os.path.join(ROOT, 'top-k-rec_amd', 'libtkr_hip.so'))
    lse, dense, step, size = lib.tkr_smf_lse_rows, lib.tkr_smf_dense_rows, lib.tkr_smf_step_rows, lib.tkr_smf_workspace_bytes
    lse.restype = dense.restype = step.restype = C.c_int
    size.restype = C.c_int64
    size.argtypes = [C.c_int64, C.c_int32, C.c_int64]
    lse.argtypes = [C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_int32, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p]
    dense.argtypes = [C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p]
    step.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_int32, C.c_int32, C.c_double,
                     C.c_double, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p]
    return lse, dense, step, size


def test_raw_abi_through_ctypes():
    """the symbols as a maintainer of the reference would bind them: no helper module in between; and the argument
    checks: k = 129 is TKR_E_UNSUPPORTED, nothing is launched and nothing written"""
    lse_f, dense, step, size = _raw()
    k = 12
    K = k + 1
    X0, H0, _, rows, _ = _step_case(k)
    n_x, n_y = len(X0), SLAB + 5                                                # two slabs: the dense calls need the workspace
    Y = (np.random.Generator(np.random.PCG64(6)).standard_normal((n_y, K)) * 0.5).astype(np.float32)
    rows = [np.asarray(x) % n_y for x in rows]
    ptr, cols = O.to_csr(rows)
    Xd, Hd, Yd, pd, cd = _dev(X0), _dev(H0), _dev(Y), _dev(ptr), _dev(cols)
    lse = torch.zeros(n_x, dtype=torch.float32, device='cuda')
    D = torch.zeros((n_x, K), dtype=torch.float32, device='cuda')
    loss = torch.zeros(n_x, dtype=torch.float64, device='cuda')
    status = torch.empty(1, dtype=torch.int64, device='cuda')
    need = size(n_x, k, n_y)
    assert need >= 2 * n_x * K * 4 and need % 16 == 0
    ws = torch.empty(need // 8 + 2, dtype=torch.int64, device='cuda')
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    p = lambda t: C.c_void_p(t.data_ptr())
    l_args = [p(Xd), n_x, p(Yd), n_y, k, p(lse), p(ws), need, stream]
    assert lse_f(*l_args) == 0
    _held('raw lse', lse.cpu().numpy(), O.lse_rows(X0, Y), O.lse_rows(X0, Y, dtype=np.float32))
    d_args = [p(Xd), n_x, p(Yd), n_y, k, p(lse), None, p(D), p(ws), need, stream]
    assert dense(*d_args) == 0
    lse_h = lse.cpu().numpy()
    _held('raw dense', D.cpu().numpy(), O.dense_rows(X0, Y, row_off=lse_h), O.dense_rows(X0, Y, row_off=lse_h, dtype=np.float32))
    s_args = [p(Yd), n_y, k, p(D), p(pd), p(cd), len(cols), n_x, k, 1, STEP['lam'], STEP['lr'], 300, p(Xd), p(Hd), p(loss), p(ws), need, p(status), stream]
    Dh = D.cpu().numpy()
    assert step(*s_args) == 0
    assert int(status.item()) == -1
    hyper = dict(fixed=k, scale_by_likes=True, **STEP)
    x64, h64, l64 = O.step_rows(X0, H0, Y, Dh, rows, **hyper)
    x32, h32, l32 = O.step_rows(X0, H0, Y, Dh, rows, dtype=np.float32, heavy_from=300, **hyper)
    _held('raw step x', Xd.cpu().numpy(), x64, x32)
    _held('raw step row loss', loss.cpu().numpy(), l64, l32)
    before = [t.clone() for t in (Xd, Hd, D, lse, loss)]
    odd = C.c_void_p(ws.data_ptr() + 8)                                         # a workspace that is not 16-byte aligned
    for at, bad, rc in ((0, None, -1), (2, None, -1), (5, None, -1), (1, 0, -1), (3, 0, -1), (4, 0, -1), (4, 129, -2), (6, odd, -1), (6, None, -1),
                        (7, 16, -1), (7, -1, -1)):
        args = list(l_args)
        args[at] = bad
        assert lse_f(*args) == rc, at
    for at, bad, rc in ((0, None, -1), (2, None, -1), (7, None, -1), (1, 0, -1), (3, 0, -1), (4, 0, -1), (4, 129, -2), (8, odd, -1), (8, None, -1),
                        (9, need - 16 * n_x, -1), (9, -1, -1), (5, C.c_void_p(lse.data_ptr() + 2), -1)):
        args = list(d_args)
        args[at] = bad
        assert dense(*args) == rc, at
    for at, bad, rc in ((0, None, -1), (3, None, -1), (4, None, -1), (5, None, -1), (13, None, -1), (14, None, -1), (18, None, -1), (2, 0, -1),
                        (2, 129, -2), (6, -1, -1), (7, 0, -1), (1, 0, -1), (8, -2, -1), (8, K, -1), (9, 2, -1), (12, 0, -1), (10, -0.5, -1),
                        (10, float('nan'), -1), (11, float('inf'), -1), (16, None, -1), (16, odd, -1), (17, 8, -1)):
        args = list(s_args)
        args[at] = bad
        assert step(*args) == rc, at
    assert size(n_x, 129, n_y) == -2 and size(n_x, 0, n_y) == -1
    torch.cuda.synchronize()
    for was, now in zip(before, (Xd, Hd, D, lse, loss)):
        assert torch.equal(was, now)


# ---- 6. smf.SMF end to end --------------------------------------------------------------------------------------------------------------
def _g2(golden_dir):
    return os.path.join(golden_dir, 'g2')


def _model(golden_dir):
    import smf
    d = _g2(golden_dir)
    m = smf.SMF(k=O.E2E['k'], lam=O.E2E['lam'], lr=O.E2E['lr'])
    m.load_training_data(os.path.join(d, 'uid'), os.path.join(d, 'vid'), os.path.join(d, 'f0tr.txt'), seed=O.E2E['seed'])
    return m


@functools.lru_cache(maxsize=None)
def _trained(golden_dir):
    m = _model(golden_dir)
    X0, Y0 = m._tables()
    up, uc, ip, ic = m._csr
    likes = (O.csr_rows(up, uc), O.csr_rows(ip, ic))
    hyper = dict(lam=m.lam, lr=m.lr, max_iter=O.E2E['iters'])
    m.train(max_iter=O.E2E['iters'], verbose=False)
    return m, X0, Y0, likes, O.train(X0, Y0, *likes, **hyper), O.train(X0, Y0, *likes, dtype=np.float32, **hyper)


def test_smf_trains_as_the_oracle(golden_dir):
    m, X0, Y0, likes, t64, t32 = _trained(golden_dir)
    k = m.k
    assert len(m.losses) == O.E2E['iters'] == m.iters_done and (len(likes[0]), len(likes[1])) == (40, 30)
    assert m.fue.dtype == np.float32 and m.fue.shape == (40, k) and m.fie.shape == (30, k) and m.fib.shape == (30, 1)
    for name, got, at in (('fue', m.fue, lambda t: t[0][:, :k]), ('fie', m.fie, lambda t: t[1][:, :k]), ('item biases', m.fib[:, 0], lambda t: t[1][:, k]),
                          ('user slots', m.hu, lambda t: t[2]), ('item slots', m.hi, lambda t: t[3])):
        _held('SMF %s after %d iterations' % (name, O.E2E['iters']), got, at(t64), at(t32))
    rel = np.abs(np.asarray(m.losses) - np.asarray(t64[4])) / np.asarray(t64[4])
    print('K27 SMF losses on g2: %s, against the oracle %s' % (m.losses, rel))
    assert rel.max() <= 1e-5
    assert abs(m.losses[0] - m.n_likes * np.log(m.n_items)) <= 1e-3 * m.losses[0] and m.losses[-1] < m.losses[0]
    assert sum(1 for x in likes[0] if len(x) == 0) == 3 and sum(1 for x in likes[1] if len(x) == 0) == 4
    assert (m.hu[:, k] == 1).all() and (m.hi[:, k] > 1).all()       # the users' ones are fixed, the items' biases move


def test_two_trainings_with_one_seed_give_the_same_bits(golden_dir):
    m = _trained(golden_dir)[0]
    again = _model(golden_dir)
    again.train(max_iter=O.E2E['iters'], verbose=False)
    for name in ('fue', 'fie', 'fib', 'hu', 'hi'):
        np.testing.assert_array_equal(_bits(getattr(again, name)), _bits(getattr(m, name)), err_msg=name)
    assert again.losses == m.losses


# ---- 7. the model directory -------------------------------------------------------------------------------------------------------------
def test_smf_model_directory_serves_evaluate_and_a_second_train(golden_dir, tmp_path):
    import evaluate as E
    from oracle import ref_np as R
    m = _trained(golden_dir)[0]
    out = str(tmp_path / 'smf')
    m.export_embeddings(out)
    assert sorted(os.listdir(out)) == ['final-B.dat', 'final-U.dat', 'final-V.dat', 'smf.npz']
    # g2 holds no out-of-matrix test line: with 'om' the command ends as the reference's does (evaluate.py:112 divides by the number of
    # test likes) and so does the oracle, before either prints a line (tests/test_gpu_als.py); the scenario that has lines is compared
    with pytest.raises(ZeroDivisionError):
        E.main(['-d', _g2(golden_dir), '-m', out, '-sl', 'im', 'om', '-M', 'acc', 'auc'])
    with pytest.raises(ZeroDivisionError):
        R.evaluate_cli(_g2(golden_dir), out, scenarios=('im', 'om'))
    got = E.main(['-d', _g2(golden_dir), '-m', out, '-sl', 'im', '-M', 'acc', 'auc'])
    exp = R.evaluate_cli(_g2(golden_dir), out, scenarios=('im',))
    assert got[0].startswith('im,') and sorted(g.split(',')[0] for g in got[1:]) == ['im.acc', 'im.auc'] and len(exp) == 1
    assert [float(x) for x in got[0].split(',')[1:]] == [float(x) for x in exp[0].split(',')[1:]]
    for g in got[1:]:
        assert all(0.0 <= float(x) <= 1.0 for x in g.split(',')[1:])
    fresh = _model(golden_dir)
    fresh.train(max_iter=0, model_path=out, verbose=False)                      # loads, runs no iteration
    np.testing.assert_array_equal(_bits(fresh.hu), _bits(m.hu))
    np.testing.assert_array_equal(_bits(fresh.hi), _bits(m.hi))
    assert fresh.iters_done == m.iters_done and (fresh.hu != 1).any()
    np.testing.assert_allclose(fresh.fue, m.fue, atol=1e-6)                     # the '%f ' text of the factors
    np.testing.assert_allclose(fresh.fib, m.fib, atol=1e-6)
    fresh.train(max_iter=1, verbose=False)
    assert fresh.iters_done == m.iters_done + 1 and (fresh.hu >= m.hu).all() and (fresh.hu[:, :m.k] > m.hu[:, :m.k]).any()


# ---- 8. fold-in -------------------------------------------------------------------------------------------------------------------------
def test_smf_fold_in_is_five_user_half_steps_from_zero(golden_dir):
    m, X0, Y0, likes = _trained(golden_dir)[:4]
    k = m.k
    users = [u for u, x in enumerate(likes[0]) if len(x)][:5]
    hist = [likes[0][u] for u in users]
    rows = m.fold_in(hist, steps=5)
    assert rows.shape == (5, k) and rows.dtype == np.float32
    Ya = m._tables()[1]
    ref = {dtype: O.fold_in(Ya, hist, steps=5, lam=m.lam, lr=m.lr, dtype=dtype) for dtype in (np.float64, np.float32)}
    _held('SMF fold_in rows', rows, ref[np.float64][:, :k], ref[np.float32][:, :k])
    none = m.fold_in([[]], steps=2)                                             # a user without likes has no gradient at zero
    assert none.shape == (1, k) and not none.any()
    assert m.fold_in([], steps=2).shape == (0, k)
