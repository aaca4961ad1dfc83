"""K20 on the GPU (csrc/als.hip, top-k-rec_amd/als.py) against tests/_als_oracle.py.

The yardstick of the solve is float32 LAPACK on the same systems: with x64 the float64 oracle on the same fp32 inputs and x32 the
float32 one, e32 = max|x32 - x64| / max|x64| per case, and the kernel has to stay within F * max(e32, 2^-23) -- Cholesky in place of
pivoted LU and another order of the Gram's sums are a small constant either way.  F is the next power of two above twice the worst
ratio err / max(e32, 2^-23) measured on an MI355X (7.84, the loss of the single row at k = 5; the rest lie between 0.1 and 1.5;
DESIGN.md section 4 K20 keeps the ratios per k); F <= 16 is a condition of the design, not a knob.  The backward error has a bound that can be derived and is asserted as derived."""
import ctypes as C
import functools
import os

import numpy as np
import pytest
import torch

import _als_oracle as O

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = 16.0
FLOOR = 2.0 ** -23


def _dev(a):
    return torch.from_numpy(np.array(a, order='C')).cuda()               # (a copy: the shared oracle arrays are read-only)


def _bits(a):
    return np.ascontiguousarray(a).view(np.int32 if a.dtype == np.float32 else np.int64)


def _ratio(got, x64, x32):
    scale = np.abs(x64).max()
    err, e32 = np.abs(got - x64).max() / scale, np.abs(x32 - x64).max() / scale
    return err / max(e32, FLOOR), err, e32


# ---- 1. the Gram, exact ---------------------------------------------------------------------------------------------------------------
def _exact_table(rng, n, k):
    return (rng.integers(-3, 4, (n, k)) / 8).astype(np.float32)


def _gram_np(Y, rows, scale, ridge):
    Yr = Y[rows].astype(np.float64)                                   # every sum is exact: multiples of 1/64 far below 2^24 of them
    return (scale * (Yr.T @ Yr) + ridge * np.eye(Y.shape[1])).astype(np.float32)


def _check_gram(k, sizes, seed):
    import tkr_hip
    rng = np.random.Generator(np.random.PCG64([seed, k]))
    for n_listed in sizes:
        for scale, ridge in ((0.5, 0.25), (1.0, 0.0)):
            if n_listed > 0:                                          # rows = NULL: all n rows
                Y = _exact_table(rng, n_listed, k)
                G = tkr_hip.als_gram(_dev(Y), None, scale=scale, ridge=ridge).cpu().numpy()
                np.testing.assert_array_equal(_bits(G), _bits(_gram_np(Y, np.arange(n_listed), scale, ridge)), err_msg='all rows, n = %d' % n_listed)
            n = 57
            Y = _exact_table(rng, n, k)
            rows = rng.integers(0, n, n_listed).astype(np.int32)      # with repeats (57 rows, the lists are longer)
            if n_listed >= 2:
                rows[1] = rows[0]
            Yd, rd = _dev(Y), _dev(rows)
            G = tkr_hip.als_gram(Yd, rd, scale=scale, ridge=ridge).cpu().numpy()
            np.testing.assert_array_equal(_bits(G), _bits(_gram_np(Y, rows, scale, ridge)), err_msg='a list of %d' % n_listed)
            np.testing.assert_array_equal(_bits(G), _bits(tkr_hip.als_gram(Yd, rd, scale=scale, ridge=ridge).cpu().numpy()))


@pytest.mark.parametrize('k', [1, 3, 8, 31, 32, 33, 64, 65, 128])
def test_gram_is_exact_on_exact_inputs(k):
    _check_gram(k, (0, 1, 2), seed=1)


@pytest.mark.parametrize('k', [8, 33])
def test_gram_is_exact_across_slabs(k):
    import tkr_hip
    S = tkr_hip.ALS_GRAM_SLAB
    _check_gram(k, (S - 1, S, S + 1, 2 * S + 3), seed=2)


def test_gram_skips_and_reports_rows_outside_the_table():
    import tkr_hip
    rng = np.random.Generator(np.random.PCG64(3))
    n, k = 40, 33
    Y = _exact_table(rng, n, k)
    S = tkr_hip.ALS_GRAM_SLAB
    for n_listed, bad in ((50, {7: -1, 30: n}), (50, {30: -1, 7: n}), (S + 9, {S + 2: n, S + 5: -1}), (3, {2: 1 << 30})):
        rows = rng.integers(0, n, n_listed).astype(np.int32)
        for t, value in bad.items():
            rows[t] = value
        keep = np.asarray([t for t in range(n_listed) if t not in bad])
        G, status = tkr_hip.als_gram(_dev(Y), _dev(rows), scale=0.5, ridge=2.0, check=False)
        assert int(status.item()) == 4 * min(bad) + 1
        np.testing.assert_array_equal(_bits(G.cpu().numpy()), _bits(_gram_np(Y, rows[keep], 0.5, 2.0)))
        with pytest.raises(tkr_hip.AlsRefused) as info:
            tkr_hip.als_gram(_dev(Y), _dev(rows), scale=0.5, ridge=2.0)
        assert (info.value.row, info.value.kind) == (min(bad), 1)


# ---- 2. / 3. the solve against the oracle; the backward error ----------------------------------------------------------------------
NO_HEAVY = 1 << 30


@functools.lru_cache(maxsize=None)
def _oracle_case(k, ridge, n_x):
    Y, X0, rows, rated = O.solve_inputs(k, n_x=n_x)
    hyper = dict(a=O.SOLVE_A, b=O.SOLVE_B, ridge_in_G=0.0, ridge=ridge)
    x64, l64 = O.half_step(X0, Y, rows, rated, dtype=np.float64, **hyper)
    x32, l32 = O.half_step(X0, Y, rows, rated, dtype=np.float32, **hyper)
    for a in (Y, X0, x64, l64, x32, l32):
        a.setflags(write=False)
    return Y, X0, rows, rated, x64, l64, x32, l32


@functools.lru_cache(maxsize=None)
def _gpu_case(k, heavy_from, ridge, n_x):
    import tkr_hip
    Y, X0, rows, rated = _oracle_case(k, ridge, n_x)[:4]
    ptr, cols = O.to_csr(rows)
    Yd, pd, cd = _dev(Y), _dev(ptr), _dev(cols)
    G = tkr_hip.als_gram(Yd, _dev(np.asarray(rated, dtype=np.int32)), scale=O.SOLVE_B, ridge=0.0)
    out = []
    for _ in range(2):
        X = _dev(X0.copy())
        loss = tkr_hip.als_solve_rows(Yd, G, pd, cd, X, w_like=O.SOLVE_A - O.SOLVE_B, w_rhs=O.SOLVE_A, ridge=ridge, heavy_from=heavy_from,
                                      want_loss=True)
        out.append((X.cpu().numpy(), loss.cpu().numpy()))
    return out


SOLVE_K = [1, 5, 32, 33, 50, 64, 65, 128]


@pytest.mark.parametrize('ridge', [0.01, 0.1])
@pytest.mark.parametrize('heavy_from', [8, NO_HEAVY])
@pytest.mark.parametrize('k', SOLVE_K)
def test_solve_rows_against_the_oracle(k, heavy_from, ridge):
    _solve_against_oracle(k, heavy_from, ridge, 37)


@pytest.mark.parametrize('heavy_from', [8, NO_HEAVY])
@pytest.mark.parametrize('k', [5, 128])
def test_solve_one_row(k, heavy_from):
    _solve_against_oracle(k, heavy_from, 0.01, 1)


@pytest.mark.parametrize('heavy_from', [8, NO_HEAVY])
def test_solve_more_rows_than_the_plan_walks_at_once(heavy_from):
    """1,037 rows: the plan kernel hands out the heavy rows' slabs in chunks of 1,024 rows and carries the count across them"""
    _solve_against_oracle(5, heavy_from, 0.01, 1037)


@pytest.mark.parametrize('heavy_from', [8, NO_HEAVY])
def test_solve_rows_longer_than_a_slab(heavy_from):
    """rows of 2 slabs + 3 and of 1 slab + 6 likes (with repeats: the table has 45 rows): several workgroups share a heavy row, and the
    solve adds their partials; alone, the row walks 65 tiles"""
    import tkr_hip
    S, k, ridge = tkr_hip.ALS_GRAM_SLAB, 33, 0.01
    rng = np.random.Generator(np.random.PCG64(21))
    Y, X0 = rng.random((45, k), dtype=np.float32), rng.random((3, k), dtype=np.float32)
    rows = [rng.integers(0, 45, 2 * S + 3), np.zeros(0, np.int64), rng.integers(0, 45, S + 6)]
    rated = list(range(45))
    ptr, cols = O.to_csr(rows)
    Yd, X = _dev(Y), _dev(X0)
    G = tkr_hip.als_gram(Yd, None, scale=O.SOLVE_B, ridge=0.0)
    loss = tkr_hip.als_solve_rows(Yd, G, _dev(ptr), _dev(cols), X, w_like=O.SOLVE_A - O.SOLVE_B, w_rhs=O.SOLVE_A, ridge=ridge,
                                  heavy_from=heavy_from, want_loss=True).cpu().numpy()
    X = X.cpu().numpy()
    hyper = dict(a=O.SOLVE_A, b=O.SOLVE_B, ridge_in_G=0.0, ridge=ridge)
    x64, l64 = O.half_step(X0, Y, rows, rated, dtype=np.float64, **hyper)
    x32, l32 = O.half_step(X0, Y, rows, rated, dtype=np.float32, **hyper)
    rx, ex, e32x = _ratio(X.astype(np.float64), x64, x32.astype(np.float64))
    rl, el, e32l = _ratio(loss, l64, l32)
    print('K20 long rows heavy_from=%d: x err %.3g e32 %.3g ratio %.3g; loss err %.3g e32 %.3g ratio %.3g' % (heavy_from, ex, e32x, rx, el, e32l, rl))
    np.testing.assert_array_equal(_bits(X[1]), _bits(X0[1]))
    assert rx <= F and rl <= F


def _solve_against_oracle(k, heavy_from, ridge, n_x):
    Y, X0, rows, rated, x64, l64, x32, l32 = _oracle_case(k, ridge, n_x)
    (X, loss), (X2, loss2) = _gpu_case(k, heavy_from, ridge, n_x)
    np.testing.assert_array_equal(_bits(X), _bits(X2))                          # two calls, the same bits
    np.testing.assert_array_equal(_bits(loss), _bits(loss2))
    empty = [r for r, likes in enumerate(rows) if len(likes) == 0]
    np.testing.assert_array_equal(_bits(X[empty]), _bits(X0[empty]))            # rows without likes: bit for bit as they were
    assert not loss[empty].any() and np.isfinite(X).all()
    rx, ex, e32x = _ratio(X.astype(np.float64), x64, x32.astype(np.float64))
    rl, el, e32l = _ratio(loss, l64, l32)
    print('K20 solve k=%d heavy_from=%d ridge=%g n_x=%d: x err %.3g e32 %.3g ratio %.3g; loss err %.3g e32 %.3g ratio %.3g'
          % (k, heavy_from, ridge, n_x, ex, e32x, rx, el, e32l, rl))
    assert rx <= F, (ex, e32x)
    assert rl <= F, (el, e32l)


@pytest.mark.parametrize('ridge', [0.01, 0.1])
@pytest.mark.parametrize('heavy_from', [8, NO_HEAVY])
@pytest.mark.parametrize('k', SOLVE_K)
def test_solve_rows_backward_error(k, heavy_from, ridge):
    """|| (A64 + ridge I) x - rhs64 ||_inf <= (3 k^2 + m + n_rated + 8) 2^-24 (||A64 + ridge I||_inf ||x||_inf + ||rhs64||_inf): 3 k^2 is
    Higham's constant k gamma_{3k+1} of a Cholesky solve, m + n_rated + 8 the worst summation error of the two Grams in any order; all
    terms of the sums are non-negative on these inputs, so no cancellation hides in the norms"""
    Y, X0, rows, rated = _oracle_case(k, ridge, 37)[:4]
    X = _gpu_case(k, heavy_from, ridge, 37)[0][0].astype(np.float64)
    Y64 = Y.astype(np.float64)
    G = O.gram(Y64, rated, O.SOLVE_B, 0.0)
    worst = 0.0
    for r, likes in enumerate(rows):
        if len(likes) == 0:
            continue
        y = Y64[likes]
        A = G + (O.SOLVE_A - O.SOLVE_B) * (y.T @ y) + ridge * np.eye(k)
        rhs = O.SOLVE_A * y.sum(axis=0)
        bound = (3 * k * k + len(likes) + len(rated) + 8) * 2.0 ** -24 * (np.abs(A).sum(axis=1).max() * np.abs(X[r]).max() + np.abs(rhs).max())
        res = np.abs(A @ X[r] - rhs).max()
        worst = max(worst, res / bound)
        assert res <= bound, (r, len(likes), res, bound)
    print('K20 backward error k=%d heavy_from=%d ridge=%g: worst residual / bound %.3g' % (k, heavy_from, ridge, worst))


# ---- 4. refusals -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('heavy_from', [8, NO_HEAVY])
def test_like_columns_outside_the_table_are_skipped(heavy_from):
    import tkr_hip
    k, ridge = 33, 0.01
    Y, X0, rows, rated = O.solve_inputs(k)
    n_y = len(Y)
    dirty = [np.asarray(x, dtype=np.int64) for x in rows]
    dirty[4] = np.concatenate([dirty[4][:3], [-1], dirty[4][3:], [n_y]])       # 8 likes and two refused: heavy at heavy_from = 8
    dirty[2] = np.concatenate([[n_y], dirty[2]])
    dirty[9] = np.concatenate([dirty[9][:20], [-1, -1], dirty[9][20:]])
    dirty[11] = np.asarray([-1, n_y])                                           # nothing left: as a row without likes
    clean = list(rows)
    clean[11] = np.zeros(0, np.int64)
    ptr, cols = O.to_csr(dirty)
    Yd = _dev(Y)
    G = tkr_hip.als_gram(Yd, _dev(np.asarray(rated, dtype=np.int32)), scale=O.SOLVE_B, ridge=0.0)
    X = _dev(X0.copy())
    loss, status = tkr_hip.als_solve_rows(Yd, G, _dev(ptr), _dev(cols), X, w_like=O.SOLVE_A - O.SOLVE_B, w_rhs=O.SOLVE_A, ridge=ridge,
                                          heavy_from=heavy_from, want_loss=True, check=False)
    assert int(status.item()) == 4 * 2 + 1
    hyper = dict(a=O.SOLVE_A, b=O.SOLVE_B, ridge_in_G=0.0, ridge=ridge)
    x64, l64 = O.half_step(X0, Y, clean, rated, dtype=np.float64, **hyper)
    x32, l32 = O.half_step(X0, Y, clean, rated, dtype=np.float32, **hyper)
    X, loss = X.cpu().numpy(), loss.cpu().numpy()
    assert _ratio(X.astype(np.float64), x64, x32.astype(np.float64))[0] <= F and _ratio(loss, l64, l32)[0] <= F
    np.testing.assert_array_equal(_bits(X[11]), _bits(X0[11]))
    assert loss[11] == 0.0
    with pytest.raises(tkr_hip.AlsRefused) as info:
        tkr_hip.als_solve_rows(Yd, G, _dev(ptr), _dev(cols), _dev(X0.copy()), w_like=0.99, w_rhs=1.0, ridge=ridge, heavy_from=heavy_from)
    assert (info.value.row, info.value.kind) == (2, 1)


@pytest.mark.parametrize('heavy_from', [8, NO_HEAVY])
def test_descending_like_ptr_leaves_the_row(heavy_from):
    import tkr_hip
    k = 16
    Y, X0, rows, rated = O.solve_inputs(k)
    ptr, cols = O.to_csr(rows)
    ptr = ptr.copy()
    ptr[6] = ptr[5] - 1                                                         # row 5 descends; row 6 is a row again, longer by what row 5 had
    Yd = _dev(Y)
    G = tkr_hip.als_gram(Yd, None, scale=O.SOLVE_B, ridge=0.0)
    X = _dev(X0.copy())
    loss, status = tkr_hip.als_solve_rows(Yd, G, _dev(ptr), _dev(cols), X, w_like=0.99, w_rhs=1.0, ridge=0.01, heavy_from=heavy_from,
                                          want_loss=True, check=False)
    assert int(status.item()) == 4 * 5 + 3
    X = X.cpu().numpy()
    np.testing.assert_array_equal(_bits(X[5]), _bits(X0[5]))
    assert loss[5].item() == 0.0 and np.isfinite(X).all()
    changed = [r for r in range(len(rows)) if r != 5 and ptr[r + 1] > ptr[r]]
    assert all((X[r] != X0[r]).any() for r in changed)
    good = O.to_csr(rows)[0]
    for at, value, word in ((1, 3, 4 * 1 + 3), (len(good) - 1, len(cols) + 1, 4 * (len(rows) - 1) + 3)):      # row 1 ends past row 2's end; past the end
        bad_ptr = good.copy()
        bad_ptr[at] = value
        _, status = tkr_hip.als_solve_rows(Yd, G, _dev(bad_ptr), _dev(cols), _dev(X0.copy()), w_like=0.99, w_rhs=1.0, ridge=0.01,
                                           heavy_from=heavy_from, check=False)
        assert int(status.item()) == word
    bad_ptr = good.copy()
    bad_ptr[0] = 1                                                              # does not start at 0
    with pytest.raises(tkr_hip.AlsRefused) as info:
        tkr_hip.als_solve_rows(Yd, G, _dev(bad_ptr), _dev(cols), _dev(X0.copy()), w_like=0.99, w_rhs=1.0, ridge=0.01, heavy_from=heavy_from)
    assert (info.value.row, info.value.kind) == (0, 3)


def test_a_system_that_is_not_positive_definite_is_refused():
    import tkr_hip
    for k in (1, 7, 64):
        Y = torch.zeros((5, k), dtype=torch.float32, device='cuda')
        G = torch.zeros((k, k), dtype=torch.float32, device='cuda')
        X0 = np.random.Generator(np.random.PCG64(k)).random((3, k), dtype=np.float32)
        X = _dev(X0.copy())
        ptr, cols = _dev(np.asarray([0, 0, 1, 1], dtype=np.int64)), _dev(np.asarray([2], dtype=np.int32))
        loss, status = tkr_hip.als_solve_rows(Y, G, ptr, cols, X, w_like=0.99, w_rhs=1.0, ridge=0.0, heavy_from=NO_HEAVY, want_loss=True, check=False)
        assert int(status.item()) == 4 * 1 + 2
        np.testing.assert_array_equal(_bits(X.cpu().numpy()), _bits(X0))
        assert not loss.cpu().numpy().any()
        with pytest.raises(tkr_hip.AlsRefused) as info:
            tkr_hip.als_solve_rows(Y, G, ptr, cols, X, w_like=0.99, w_rhs=1.0, ridge=0.0)
        assert (info.value.row, info.value.kind) == (1, 2)


def _raw():
    lib = C.CDLL(os.path.join(ROOT, 'top-k-rec_amd', 'libtkr_hip.so'))
    gram, solve, size = lib.tkr_als_gram, lib.tkr_als_solve_rows, lib.tkr_als_workspace_bytes
    gram.restype = solve.restype = C.c_int
    size.restype = C.c_int64
    size.argtypes = [C.c_int64, C.c_int32, C.c_int64]
    gram.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_int64, C.c_double, C.c_double, C.c_void_p, C.c_void_p, C.c_int64,
                     C.c_void_p, C.c_void_p]
    solve.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_double, C.c_double,
                      C.c_double, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p]
    return gram, solve, size


# ---- 6. the raw ABI (and the argument checks of 4.) -------------------------------------------------------------------------------
def test_raw_abi_through_ctypes():
    """the symbols as a maintainer of the reference would bind them: no helper module in between"""
    gram, solve, size = _raw()
    k, ridge = 12, 0.01
    Y, X0, rows, rated = O.solve_inputs(k, n_x=9, n_y=20)
    ptr, cols = O.to_csr(rows)
    Yd, Xd, pd, cd, rd = _dev(Y), _dev(X0.copy()), _dev(ptr), _dev(cols), _dev(np.asarray(rated, dtype=np.int32))
    G = torch.empty((k, k), dtype=torch.float32, device='cuda')
    loss = torch.empty(9, dtype=torch.float64, device='cuda')
    status = torch.empty(1, dtype=torch.int64, device='cuda')
    n_heavy = sum(1 for x in rows if len(x) >= 8)
    ws = torch.empty(max(size(0, k, 1), size(9, k, n_heavy)) // 8, dtype=torch.int64, device='cuda')
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    p = lambda t: C.c_void_p(t.data_ptr())
    g_args = [p(Yd), 20, k, p(rd), len(rated), O.SOLVE_B, 0.0, p(G), p(ws), ws.numel() * 8, p(status), stream]
    assert gram(*g_args) == 0
    assert int(status.item()) == -1
    s_args = [p(Yd), 20, k, p(G), p(pd), p(cd), len(cols), 9, O.SOLVE_A - O.SOLVE_B, O.SOLVE_A, ridge, 8, p(Xd), p(loss), p(ws), ws.numel() * 8,
              p(status), stream]
    assert solve(*s_args) == 0
    assert int(status.item()) == -1
    hyper = dict(a=O.SOLVE_A, b=O.SOLVE_B, ridge_in_G=0.0, ridge=ridge)
    x64, l64 = O.half_step(X0, Y, rows, rated, dtype=np.float64, **hyper)
    x32, l32 = O.half_step(X0, Y, rows, rated, dtype=np.float32, **hyper)
    assert _ratio(Xd.cpu().numpy().astype(np.float64), x64, x32.astype(np.float64))[0] <= F
    assert _ratio(loss.cpu().numpy(), l64, l32)[0] <= F
    # null pointers, k = 0, negative sizes: TKR_E_INVAL; k = 129: TKR_E_UNSUPPORTED; nothing is launched, X stays as it is
    before = Xd.clone()
    for at, bad, rc in ((0, None, -1), (7, None, -1), (10, None, -1), (2, 0, -1), (2, 129, -2), (1, 0, -1), (4, -1, -1), (8, None, -1)):
        args = list(g_args)
        args[at] = bad
        assert gram(*args) == rc, at
    for at, bad, rc in ((0, None, -1), (3, None, -1), (4, None, -1), (5, None, -1), (12, None, -1), (16, None, -1), (2, 0, -1), (2, 129, -2),
                        (6, -1, -1), (7, 0, -1), (1, 0, -1), (11, 0, -1), (10, -0.5, -1), (8, float('nan'), -1), (14, None, -1), (15, 8, -1)):
        args = list(s_args)
        args[at] = bad
        assert solve(*args) == rc, at
    assert size(9, 129, 0) == -1 and size(9, 0, 0) == -1
    torch.cuda.synchronize()
    assert torch.equal(before, Xd)


# ---- 5. als.WMF end to end ------------------------------------------------------------------------------------------------------------
def _g2(golden_dir):
    return os.path.join(golden_dir, 'g2')


def _model(golden_dir):
    import als
    d = _g2(golden_dir)
    m = als.WMF(k=O.E2E['k'], lu=O.E2E['lu'], lv=O.E2E['lv'])
    m.load_training_data(os.path.join(d, 'uid'), os.path.join(d, 'vid'), os.path.join(d, 'f0tr.txt'), seed=O.E2E['seed'])
    return m


@functools.lru_cache(maxsize=None)
def _trained(golden_dir):
    m = _model(golden_dir)
    U0, V0 = m.fue.copy(), m.fie.copy()
    up, uc, ip, ic = m._csr
    likes = (O.csr_rows(up, uc), O.csr_rows(ip, ic))
    hyper = dict(a=m.a, b=m.b, lu=m.lu, lv=m.lv)
    m.train(max_iter=O.E2E['iters'], tol=0.0, verbose=False)
    t64 = O.train(U0, V0, *likes, max_iter=O.E2E['iters'], tol=0.0, dtype=np.float64, **hyper)
    t32 = O.train(U0, V0, *likes, max_iter=O.E2E['iters'], tol=0.0, dtype=np.float32, **hyper)
    return m, U0, V0, likes, hyper, t64, t32


def test_wmf_trains_as_the_oracle(golden_dir):
    m, U0, V0, likes, hyper, (U64, V64, l64), (U32, V32, l32) = _trained(golden_dir)
    assert len(m.losses) == O.E2E['iters'] == len(l64)
    assert all(later < earlier for earlier, later in zip([np.exp(50)] + m.losses, m.losses)), m.losses
    assert m.fue.dtype == np.float32 and m.fue.shape == U0.shape and m.fie.shape == V0.shape
    for name, got, x64, x32 in (('fue', m.fue, U64, U32), ('fie', m.fie, V64, V32), ('last loss', np.asarray(m.losses[-1:]), np.asarray(l64[-1:]), np.asarray(l32[-1:]))):
        ratio, err, e32 = _ratio(got.astype(np.float64), x64, x32.astype(np.float64))
        print('K20 WMF %s after %d iterations: err %.3g e32 %.3g ratio %.3g' % (name, O.E2E['iters'], err, e32, ratio))
        assert ratio <= F, (name, err, e32)
    no_u = [u for u, x in enumerate(likes[0]) if len(x) == 0]
    no_i = [i for i, x in enumerate(likes[1]) if len(x) == 0]
    assert no_u                                                                # g2 has users without a training like
    np.testing.assert_array_equal(_bits(m.fue[no_u]), _bits(U0[no_u]))
    np.testing.assert_array_equal(_bits(m.fie[no_i]), _bits(V0[no_i]))


def test_wmf_stops_where_the_oracle_stops(golden_dir):
    m, U0, V0, likes, hyper = _trained(golden_dir)[:5]
    fresh = _model(golden_dir)
    np.testing.assert_array_equal(fresh.fue, U0)
    fresh.train(max_iter=200, tol=1e-2, verbose=False)
    stop64 = len(O.train(U0, V0, *likes, max_iter=200, tol=1e-2, **hyper)[2])
    assert 1 < stop64 < 200 and abs(len(fresh.losses) - stop64) <= 1


def test_wmf_model_directory_serves_evaluate(golden_dir, tmp_path, capsys):
    import evaluate as E
    from oracle import ref_np as R
    m = _trained(golden_dir)[0]
    out = str(tmp_path / 'wmf')
    m.export_embeddings(out)
    assert sorted(os.listdir(out)) == ['final-U.dat', 'final-V.dat']
    # g2 holds no out-of-matrix test line: with 'om' the command ends as the reference's does (evaluate.py:112 divides by the number of
    # test likes) and so does the oracle, before either prints a line; the scenario that has lines is compared line by line
    with pytest.raises(ZeroDivisionError):
        E.main(['-d', _g2(golden_dir), '-m', out, '-sl', 'im', 'om'])
    with pytest.raises(ZeroDivisionError):
        R.evaluate_cli(_g2(golden_dir), out, scenarios=('im', 'om'))
    got = E.main(['-d', _g2(golden_dir), '-m', out, '-sl', 'im'])
    exp = R.evaluate_cli(_g2(golden_dir), out, scenarios=('im',))
    assert len(got) == len(exp) == 1 and got[0].startswith('im,')
    for g, e in zip(got, exp):
        assert g.split(',')[0] == e.split(',')[0]
        assert [float(x) for x in g.split(',')[1:]] == [float(x) for x in e.split(',')[1:]]


def test_wmf_fold_in_is_the_user_half_step(golden_dir):
    m, U0, V0, likes, hyper = _trained(golden_dir)[:5]
    users = [u for u, x in enumerate(likes[0]) if len(x)][:3]
    hist = [likes[0][u] for u in users]
    got = m.fold_in(hist)
    assert got.shape == (3, m.k) and got.dtype == np.float32
    step = dict(a=m.a, b=m.b, ridge_in_G=m.lu, ridge=0.0)
    x64, _ = O.half_step(np.zeros((3, m.k)), m.fie, hist, m.i_rated, dtype=np.float64, **step)
    x32, _ = O.half_step(np.zeros((3, m.k)), m.fie, hist, m.i_rated, dtype=np.float32, **step)
    ratio, err, e32 = _ratio(got.astype(np.float64), x64, x32.astype(np.float64))
    print('K20 WMF fold_in: err %.3g e32 %.3g ratio %.3g' % (err, e32, ratio))
    assert ratio <= F
    assert not m.fold_in([[], []]).any()
