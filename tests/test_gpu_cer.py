"""K21 on the GPU (csrc/als.hip tkr_als_solve_rows_prior, top-k-rec_amd/als.py CER) against tests/_cer_oracle.py.

The yardstick is K20's (tests/test_gpu_als.py): with x64 the float64 oracle on the same fp32 inputs and x32 the float32 one (float32
LAPACK on the same systems), e32 = max|x32 - x64| / max|x64| per case, and the kernel has to stay within F * max(e32, 2^-23).  F is set
by K20's rule, the next power of two above twice the worst ratio measured on an MI355X (7.69, the loss of the four cold rows at k = 64,
w_prior = ridge = 10, where e32 lies below the floor; rows with likes stay below 3.4, cold rows below 6.3 in x; DESIGN.md section 4 K21
keeps the ratios per k); F <= 16 is a condition of the design, not a knob.  Rows with likes and rows without are measured apart."""
import ctypes as C
import functools
import os
import pickle
import shutil

import numpy as np
import pytest
import torch

import _als_oracle as A
import _cer_oracle as O

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = 16.0
FLOOR = 2.0 ** -23
NO_HEAVY = 1 << 30


def _dev(a):
    return torch.from_numpy(np.array(a, order='C')).cuda()               # (a copy: the shared oracle arrays are read-only)


def _bits(a):
    return np.ascontiguousarray(a).view(np.int32 if a.dtype == np.float32 else np.int64)


def _ratio(got, x64, x32):
    scale = np.abs(x64).max()
    err, e32 = np.abs(got - x64).max() / scale, np.abs(x32 - x64).max() / scale
    return err / max(e32, FLOOR), err, e32


def _solve(Y, G, rows, X0, prior, *, w_prior, ridge, heavy_from=NO_HEAVY, check=True, want_loss=True):
    """-> (X, row_loss[, status]) as numpy; G: a device tensor, or None = tkr_als_gram over the columns somebody likes"""
    import tkr_hip
    ptr, cols = A.to_csr(rows)
    Yd = _dev(Y)
    if G is None:
        rated = sorted({int(c) for likes in rows for c in likes})
        G = tkr_hip.als_gram(Yd, _dev(np.asarray(rated, dtype=np.int32)), scale=A.SOLVE_B, ridge=0.0)
    X = _dev(X0)
    out = tkr_hip.als_solve_rows_prior(Yd, G, _dev(ptr), _dev(cols), X, _dev(prior), w_like=A.SOLVE_A - A.SOLVE_B, w_rhs=A.SOLVE_A,
                                       w_prior=w_prior, ridge=ridge, heavy_from=heavy_from, want_loss=want_loss, check=check)
    if check:
        return X.cpu().numpy(), out.cpu().numpy()
    return X.cpu().numpy(), out[0].cpu().numpy(), int(out[1].item())


# ---- a. K20's bits ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('heavy_from', [8, NO_HEAVY])
@pytest.mark.parametrize('k', [5, 50, 128])
def test_zero_prior_gives_the_bits_of_solve_rows(k, heavy_from):
    import tkr_hip
    Y, X0, rows, rated = A.solve_inputs(k)
    ptr, cols = A.to_csr(rows)
    Yd, pd, cd = _dev(Y), _dev(ptr), _dev(cols)
    G = tkr_hip.als_gram(Yd, _dev(np.asarray(rated, dtype=np.int32)), scale=A.SOLVE_B, ridge=0.0)
    hyper = dict(w_like=A.SOLVE_A - A.SOLVE_B, w_rhs=A.SOLVE_A, ridge=0.01, heavy_from=heavy_from, want_loss=True)
    X20 = _dev(X0)
    loss20 = tkr_hip.als_solve_rows(Yd, G, pd, cd, X20, **hyper).cpu().numpy()
    X21 = _dev(X0)
    loss21 = tkr_hip.als_solve_rows_prior(Yd, G, pd, cd, X21, torch.zeros_like(X21), w_prior=0.0, **hyper).cpu().numpy()
    X20, X21 = X20.cpu().numpy(), X21.cpu().numpy()
    warm = [r for r, likes in enumerate(rows) if len(likes)]
    cold = [r for r, likes in enumerate(rows) if len(likes) == 0]
    assert len(cold) >= 3 and (X20[warm] != X0[warm]).any()
    np.testing.assert_array_equal(_bits(X21[warm]), _bits(X20[warm]))
    np.testing.assert_array_equal(_bits(loss21[warm]), _bits(loss20[warm]))
    assert not X21[cold].any() and not loss21[cold].any()                       # (G + ridge I)^-1 0, exactly


# ---- b. cold rows, exact ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('k', [1, 17, 64, 65, 128])
def test_cold_rows_are_exact_on_exact_inputs(k):
    """G = 3 I, ridge = 1, w_prior = 2: the factor is 2 I, rhs = 2 p, every operation exact: x = p / 2 and the loss |p / 2|^2.  Any slip
    of a lane, a tail or a pitch moves a row or a column"""
    rng = np.random.Generator(np.random.PCG64([30, k]))
    G = _dev((3 * np.eye(k)).astype(np.float32))
    Y = rng.random((9, k), dtype=np.float32)
    for n_x in (1, 63, 64, 65, 200):
        P = (rng.integers(-24, 25, (n_x, k)) / 8).astype(np.float32)
        X0 = rng.random((n_x, k), dtype=np.float32)
        X, loss = _solve(Y, G, [[]] * n_x, X0, P, w_prior=2.0, ridge=1.0)
        np.testing.assert_array_equal(_bits(X), _bits(P / 2), err_msg='n_x = %d' % n_x)
        np.testing.assert_array_equal(_bits(loss), _bits(((P.astype(np.float64) / 2) ** 2).sum(axis=1)), err_msg='n_x = %d' % n_x)
        # every third row cold among rows with likes: the cold rows as before, the warm ones against the oracle
        _, _, rows, _ = A.solve_inputs(k, n_x=n_x, n_y=9) if n_x > 1 else (None, None, [np.asarray([4, 2, 7])], None)
        rows = [np.zeros(0, np.int64) if r % 3 == 0 or len(likes) == 0 else np.asarray(likes) % 9 for r, likes in enumerate(rows)]
        X, loss = _solve(Y, G, rows, X0, P, w_prior=2.0, ridge=1.0)
        cold = [r for r, likes in enumerate(rows) if len(likes) == 0]
        warm = [r for r, likes in enumerate(rows) if len(likes)]
        np.testing.assert_array_equal(_bits(X[cold]), _bits(P[cold] / 2), err_msg='mixed, n_x = %d' % n_x)
        np.testing.assert_array_equal(_bits(loss[cold]), _bits(((P[cold].astype(np.float64) / 2) ** 2).sum(axis=1)))
        if warm:
            hyper = dict(a=A.SOLVE_A, b=A.SOLVE_B, ridge_in_G=0.0, ridge=1.0, w_prior=2.0, G=3 * np.eye(k))
            x64, l64 = O.half_step_prior(X0, Y, rows, None, P, dtype=np.float64, **hyper)
            x32, l32 = O.half_step_prior(X0, Y, rows, None, P, dtype=np.float32, **hyper)
            rx, ex, e32x = _ratio(X[warm].astype(np.float64), x64[warm], x32[warm].astype(np.float64))
            rl, el, e32l = _ratio(loss[warm], l64[warm], l32[warm])
            print('K21 exact k=%d n_x=%d warm rows: x ratio %.3g loss ratio %.3g' % (k, n_x, rx, rl))
            assert rx <= F and rl <= F, (n_x, ex, e32x, el, e32l)


# ---- c. against the oracle ----------------------------------------------------------------------------------------------------------------
def _case_inputs(k, shape):
    if shape == 'cold':                                               # one row, without likes; the Gram over every row of Y
        Y, X0, _, _ = A.solve_inputs(k, n_x=1)
        rows, rated = [np.zeros(0, np.int64)], list(range(len(Y)))
    else:
        Y, X0, rows, rated = A.solve_inputs(k, n_x=shape)
    P = (2 * np.random.Generator(np.random.PCG64([31, k, len(rows)])).random((len(rows), k), dtype=np.float32) - 1).astype(np.float32)
    return Y, X0, rows, rated, P


@functools.lru_cache(maxsize=None)
def _oracle_case(k, w, shape):
    Y, X0, rows, rated, P = _case_inputs(k, shape)
    hyper = dict(a=A.SOLVE_A, b=A.SOLVE_B, ridge_in_G=0.0, ridge=w, w_prior=w)
    out = O.half_step_prior(X0, Y, rows, rated, P, dtype=np.float64, **hyper) + O.half_step_prior(X0, Y, rows, rated, P, dtype=np.float32, **hyper)
    for a in out:
        a.setflags(write=False)
    return out


@pytest.mark.parametrize('shape', [37, 1, 'cold'])
@pytest.mark.parametrize('w', [0.1, 10.0])
@pytest.mark.parametrize('heavy_from', [8, NO_HEAVY])
@pytest.mark.parametrize('k', [1, 5, 32, 33, 50, 64, 65, 128])
def test_solve_rows_prior_against_the_oracle(k, heavy_from, w, shape):
    import tkr_hip
    Y, X0, rows, rated, P = _case_inputs(k, shape)
    x64, l64, x32, l32 = _oracle_case(k, w, shape)
    G = tkr_hip.als_gram(_dev(Y), _dev(np.asarray(rated, dtype=np.int32)), scale=A.SOLVE_B, ridge=0.0)
    X, loss = _solve(Y, G, rows, X0, P, w_prior=w, ridge=w, heavy_from=heavy_from)
    X2, loss2 = _solve(Y, G, rows, X0, P, w_prior=w, ridge=w, heavy_from=heavy_from)
    np.testing.assert_array_equal(_bits(X), _bits(X2))                          # two calls, the same bits
    np.testing.assert_array_equal(_bits(loss), _bits(loss2))
    assert np.isfinite(X).all() and np.isfinite(loss).all()
    for name, which in (('warm', [r for r, likes in enumerate(rows) if len(likes)]), ('cold', [r for r, likes in enumerate(rows) if len(likes) == 0])):
        if not which:
            continue
        rx, ex, e32x = _ratio(X[which].astype(np.float64), x64[which], x32[which].astype(np.float64))
        rl, el, e32l = _ratio(loss[which], l64[which], l32[which])
        print('K21 solve k=%d heavy_from=%d w=%g n_x=%s %s rows: x err %.3g e32 %.3g ratio %.3g; loss err %.3g e32 %.3g ratio %.3g'
              % (k, heavy_from, w, shape, name, ex, e32x, rx, el, e32l, rl))
        assert rx <= F, (name, ex, e32x)
        assert rl <= F, (name, el, e32l)


# ---- d. independence ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('k', [33, 128])
def test_a_cold_row_does_not_depend_on_its_neighbours(k):
    import tkr_hip
    Y, X0, rows, rated = A.solve_inputs(k, n_x=200)
    rng = np.random.Generator(np.random.PCG64([32, k]))
    P = (2 * rng.random((200, k), dtype=np.float32) - 1).astype(np.float32)
    G = tkr_hip.als_gram(_dev(Y), _dev(np.asarray(rated, dtype=np.int32)), scale=A.SOLVE_B, ridge=0.0)
    X, loss = _solve(Y, G, rows, X0, P, w_prior=0.5, ridge=0.25)
    cold = [r for r, likes in enumerate(rows) if len(likes) == 0]
    assert len(cold) >= 5
    for r in (cold[0], cold[1], cold[len(cold) // 2], cold[-2], cold[-1]):       # lanes 0, 11, ..., in several waves and workgroups
        x1, l1 = _solve(Y, G, [[]], X0[r:r + 1], P[r:r + 1], w_prior=0.5, ridge=0.25)
        np.testing.assert_array_equal(_bits(x1[0]), _bits(X[r]))
        np.testing.assert_array_equal(_bits(l1), _bits(loss[r:r + 1]))


# ---- e. untrusted input -------------------------------------------------------------------------------------------------------------------
def test_a_factor_that_is_not_positive_definite_refuses_every_cold_row():
    k = 64                                                                      # (wider than the longest row: sum y y^T is rank deficient in every row)
    Y, X0, rows, rated = A.solve_inputs(k)
    P = np.ones((len(rows), k), np.float32)
    cold = [r for r, likes in enumerate(rows) if len(likes) == 0]
    # G = -I, ridge = 0.5: nothing is positive definite; the cold rows go with the factor, the warm rows one by one as K20 refuses them
    X, loss, status = _solve(Y, _dev(-np.eye(k, dtype=np.float32)), rows, X0, P, w_prior=1.0, ridge=0.5, check=False)
    assert status == 4 * cold[0] + 2 and cold[0] == 0
    np.testing.assert_array_equal(_bits(X), _bits(X0))
    assert not loss.any() and np.isfinite(X).all()
    # G = -0.6 I at k = 2 with rows of many likes: their systems ARE positive definite, G + ridge I = -0.1 I is not
    k = 2
    Y = np.random.Generator(np.random.PCG64(33)).random((45, k), dtype=np.float32) + 1
    rows = [np.arange(45), np.arange(40), np.zeros(0, np.int64), np.arange(3, 45), np.zeros(0, np.int64)]
    X0, P = np.full((5, k), 7, np.float32), np.ones((5, k), np.float32)
    G = -0.6 * np.eye(k, dtype=np.float32)
    X, loss, status = _solve(Y, _dev(G), rows, X0, P, w_prior=1.0, ridge=0.5, check=False)
    assert status == 4 * 2 + 2
    np.testing.assert_array_equal(_bits(X[[2, 4]]), _bits(X0[[2, 4]]))
    assert not loss[[2, 4]].any() and np.isfinite(X).all()
    x64, l64 = O.half_step_prior(X0, Y, rows, None, P, a=A.SOLVE_A, b=A.SOLVE_B, ridge_in_G=0.0, ridge=0.5, w_prior=1.0, G=G.astype(np.float64))
    np.testing.assert_allclose(X[[0, 1, 3]], x64[[0, 1, 3]], rtol=1e-4)
    import tkr_hip
    with pytest.raises(tkr_hip.AlsRefused) as info:
        _solve(Y, _dev(G), rows, X0, P, w_prior=1.0, ridge=0.5)
    assert (info.value.row, info.value.kind) == (2, 2)


@pytest.mark.parametrize('bad', [np.inf, -np.inf, np.nan])
def test_a_prior_that_is_not_finite_refuses_its_row_alone(bad):
    k = 33
    Y, X0, rows, rated = A.solve_inputs(k)
    P0 = (2 * np.random.Generator(np.random.PCG64(34)).random((len(rows), k), dtype=np.float32) - 1).astype(np.float32)
    good_X, good_loss = _solve(Y, None, rows, X0, P0, w_prior=0.5, ridge=0.5)
    for r, col in ((11, 0), (11, k - 1), (5, 0), (5, k - 1), (36, 17)):         # row 11 has no likes; rows 5 and 36 have
        P = P0.copy()
        P[r, col] = bad
        X, loss, status = _solve(Y, None, rows, X0, P, w_prior=0.5, ridge=0.5, check=False)
        assert status == 4 * r + 2, (r, col)
        assert np.isfinite(X).all() and np.isfinite(loss).all()
        np.testing.assert_array_equal(_bits(X[r]), _bits(X0[r]))
        assert loss[r] == 0.0
        others = [q for q in range(len(rows)) if q != r]
        np.testing.assert_array_equal(_bits(X[others]), _bits(good_X[others]))
        np.testing.assert_array_equal(_bits(loss[others]), _bits(good_loss[others]))


def test_descending_like_ptr_leaves_the_row():
    import tkr_hip
    k = 16
    Y, X0, rows, rated = A.solve_inputs(k)
    ptr, cols = A.to_csr(rows)
    ptr = ptr.copy()
    ptr[6] = ptr[5] - 1                                                         # row 5 descends; row 6 is a row again
    Yd = _dev(Y)
    G = tkr_hip.als_gram(Yd, None, scale=A.SOLVE_B, ridge=0.0)
    X = _dev(X0)
    P = torch.ones_like(X)
    for heavy_from in (8, NO_HEAVY):
        loss, status = tkr_hip.als_solve_rows_prior(Yd, G, _dev(ptr), _dev(cols), X, P, w_like=0.99, w_rhs=1.0, w_prior=0.3, ridge=0.3,
                                                    heavy_from=heavy_from, want_loss=True, check=False)
        assert int(status.item()) == 4 * 5 + 3
        got = X.cpu().numpy()
        np.testing.assert_array_equal(_bits(got[5]), _bits(X0[5]))
        assert loss[5].item() == 0.0 and np.isfinite(got).all()
        assert all((got[r] != X0[r]).any() for r in range(len(rows)) if r != 5)  # every other row is solved, the cold ones too


def test_raw_abi_argument_checks():
    lib = C.CDLL(os.path.join(ROOT, 'top-k-rec_amd', 'libtkr_hip.so'))
    solve, size = lib.tkr_als_solve_rows_prior, lib.tkr_als_prior_workspace_bytes
    solve.restype, size.restype = C.c_int, C.c_int64
    size.argtypes = [C.c_int64, C.c_int32, C.c_int64]
    solve.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_double, C.c_double,
                      C.c_double, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_double, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p]
    k, w = 12, 0.25
    Y, X0, rows, rated = A.solve_inputs(k, n_x=9, n_y=20)
    rows[3] = np.zeros(0, np.int64)
    Pn = (np.arange(9 * k, dtype=np.float32).reshape(9, k) % 5 - 2) / 4
    ptr, cols = A.to_csr(rows)
    Yd, Xd, pd, cd, Pd = _dev(Y), _dev(X0), _dev(ptr), _dev(cols), _dev(Pn)
    G = _dev(A.gram(Y, rated, A.SOLVE_B, 0.0, dtype=np.float32))
    loss = torch.empty(9, dtype=torch.float64, device='cuda')
    status = torch.empty(1, dtype=torch.int64, device='cuda')
    ws = torch.empty(size(9, k, sum(1 for x in rows if len(x) >= 8)) // 8, dtype=torch.int64, device='cuda')
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    p = lambda t: C.c_void_p(t.data_ptr())
    args = [p(Yd), 20, k, p(G), p(pd), p(cd), len(cols), 9, A.SOLVE_A - A.SOLVE_B, A.SOLVE_A, w, 8, p(Xd), p(loss), p(Pd), w, p(ws), ws.numel() * 8,
            p(status), stream]
    before = Xd.clone()
    # prior NULL or misaligned, w_prior negative or not finite, no workspace (the factor lives there), and what K20 refuses
    for at, bad, rc in ((14, None, -1), (14, C.c_void_p(Pd.data_ptr() + 2), -1), (15, -0.5, -1), (15, float('nan'), -1), (15, float('inf'), -1),
                        (16, None, -1), (17, 8, -1), (0, None, -1), (3, None, -1), (4, None, -1), (5, None, -1), (12, None, -1), (18, None, -1),
                        (2, 0, -1), (2, 129, -2), (6, -1, -1), (7, 0, -1), (1, 0, -1), (11, 0, -1), (10, -0.5, -1), (8, float('nan'), -1)):
        bad_args = list(args)
        bad_args[at] = bad
        assert solve(*bad_args) == rc, at
    torch.cuda.synchronize()
    assert torch.equal(before, Xd)
    assert size(9, 129, 0) == -1 and size(9, 0, 0) == -1
    assert solve(*args) == 0 and int(status.item()) == -1
    hyper = dict(a=A.SOLVE_A, b=A.SOLVE_B, ridge_in_G=0.0, ridge=w, w_prior=w)
    x64, l64 = O.half_step_prior(X0, Y, rows, rated, Pn, dtype=np.float64, **hyper)
    x32, l32 = O.half_step_prior(X0, Y, rows, rated, Pn, dtype=np.float32, **hyper)
    assert _ratio(Xd.cpu().numpy().astype(np.float64), x64, x32.astype(np.float64))[0] <= F
    assert _ratio(loss.cpu().numpy(), l64, l32)[0] <= F


# ---- f. - h. als.CER end to end -----------------------------------------------------------------------------------------------------------
def _g2(golden_dir):
    return os.path.join(golden_dir, 'g2')


def _model(golden_dir):
    import als
    d = _g2(golden_dir)
    m = als.CER(k=O.E2E['k'], d=O.E2E['d'], lu=O.E2E['lu'], lv=O.E2E['lv'], le=O.E2E['le'], a=O.E2E['a'], b=O.E2E['b'])
    m.load_training_data(os.path.join(d, 'uid'), os.path.join(d, 'vid'), os.path.join(d, 'f0tr.txt'), seed=O.E2E['seed'])
    m.feat = O.e2e_features(m.n_items)                                          # what load_content_data leaves (test h goes through a pickle)
    return m


def _likes(m):
    up, uc, ip, ic = m._csr
    return O.csr_rows(up, uc), O.csr_rows(ip, ic)


@functools.lru_cache(maxsize=None)
def _trained(golden_dir):
    m = _model(golden_dir)
    U0, V0, E0 = O.e2e_start(m.n_users, m.n_items)
    np.testing.assert_array_equal(U0, m.fue)
    likes = _likes(m)
    hyper = dict(a=m.a, b=m.b, lu=m.lu, lv=m.lv, le=m.le)
    m.train(max_iter=O.E2E['iters'], tol=0.0, verbose=False)
    t64 = O.cer_train(U0, V0, E0, m.feat, *likes, max_iter=O.E2E['iters'], tol=0.0, dtype=np.float64, **hyper)
    t32 = O.cer_train(U0, V0, E0, m.feat, *likes, max_iter=O.E2E['iters'], tol=0.0, dtype=np.float32, **hyper)
    return m, (U0, V0, E0), likes, hyper, t64, t32


def _compare_run(tag, m, t64, t32):
    U64, V64, E64, l64 = t64
    U32, V32, E32, l32 = t32
    assert len(m.losses) == len(l64)
    for name, got, x64, x32 in (('fue', m.fue, U64, U32), ('fie', m.fie, V64, V32), ('E', m.E, E64, E32)) + tuple(
            ('loss %d' % i, np.asarray([m.losses[i]]), np.asarray([l64[i]]), np.asarray([l32[i]])) for i in range(len(l64))):
        ratio, err, e32 = _ratio(np.asarray(got, dtype=np.float64), np.asarray(x64), np.asarray(x32, dtype=np.float64))
        print('K21 CER %s %s: err %.3g e32 %.3g ratio %.3g' % (tag, name, err, e32, ratio))
        assert ratio <= F, (name, err, e32)


def test_cer_trains_as_the_oracle(golden_dir):
    m, start, likes, hyper, t64, t32 = _trained(golden_dir)
    assert len(m.losses) == O.E2E['iters'] == 6
    assert all(later < earlier for earlier, later in zip([np.exp(50)] + m.losses, m.losses)), m.losses
    assert m.fue.dtype == m.fie.dtype == m.E.dtype == np.float32 and m.E.shape == (O.E2E['d'], O.E2E['k'])
    _compare_run('after 6 iterations', m, t64, t32)
    # the four cold rows: fie and embed_items are both the fp64 product F E rounded once
    cold = [j for j, x in enumerate(likes[1]) if len(x) == 0]
    assert len(cold) == 4
    Fc = m.feat[cold]
    got = m.embed_items(Fc)
    assert got.dtype == np.float32 and got.shape == (4, m.k)
    mag = np.abs(Fc).astype(np.float64) @ np.abs(m.E).astype(np.float64)
    x64 = Fc.astype(np.float64) @ m.E.astype(np.float64)
    d = O.E2E['d']
    assert (np.abs(m.fie[cold].astype(np.float64) - got) <= (d + 2) * 2.0 ** -24 * mag).all()
    for x in (m.fie[cold], got):
        assert (np.abs(x.astype(np.float64) - x64) <= 2.0 ** -24 * np.abs(x64) + (d + 2) * 2.0 ** -53 * mag).all()


def test_cer_stops_where_the_oracle_stops(golden_dir):
    m, (U0, V0, E0), likes, hyper = _trained(golden_dir)[:4]
    fresh = _model(golden_dir)
    fresh.train(max_iter=200, tol=1e-2, verbose=False)
    stop64 = len(O.cer_train(U0, V0, E0, fresh.feat, *likes, max_iter=200, tol=1e-2, **hyper)[3])
    assert 1 < stop64 < 200 and abs(len(fresh.losses) - stop64) <= 1


def test_cer_model_directory(golden_dir, tmp_path):
    import evaluate as E
    import textio
    import train_als
    from oracle import ref_np as R
    m, start, likes, hyper = _trained(golden_dir)[:4]
    out = str(tmp_path / 'cer')
    m.export_embeddings(out)
    assert sorted(os.listdir(out)) == ['final-E.dat', 'final-U.dat', 'final-V.dat']
    fresh = _model(golden_dir)
    fresh.import_embeddings(out)
    np.testing.assert_array_equal(fresh.E, textio.read_matrix(os.path.join(out, 'final-E.dat')))
    assert np.abs(fresh.E - m.E).max() <= 5.1e-7 * max(1.0, np.abs(m.E).max())  # '%f' keeps 6 decimals
    U1, V1, E1 = fresh.fue.copy(), fresh.fie.copy(), fresh.E.copy()
    fresh.train(max_iter=2, tol=0.0, model_path=out, verbose=False)              # the warm start of train.py:29
    t64 = O.cer_train(U1, V1, E1, fresh.feat, *likes, max_iter=2, tol=0.0, dtype=np.float64, **hyper)
    t32 = O.cer_train(U1, V1, E1, fresh.feat, *likes, max_iter=2, tol=0.0, dtype=np.float32, **hyper)
    _compare_run('warm start', fresh, t64, t32)

    # evaluate.py -sl im om: g2's own om files are empty, so the four items without a training like become the out-of-matrix scenario
    data = str(tmp_path / 'data')
    shutil.copytree(_g2(golden_dir), data)
    vids = [line.strip() for line in open(os.path.join(data, 'vid'))]
    uids = [line.strip() for line in open(os.path.join(data, 'uid'))]
    cold = [vids[j] for j, x in enumerate(likes[1]) if len(x) == 0]
    with open(os.path.join(data, 'f0te.om.idl'), 'w') as fh:
        fh.write(''.join(v + '\n' for v in cold))
    with open(os.path.join(data, 'f0te.om.txt'), 'w') as fh:
        for t, u in enumerate(uids[:12]):
            fh.write('%s,%s:1,%s:0,%s:%d\n' % (u, cold[t % 4], cold[(t + 1) % 4], cold[(t + 2) % 4], t % 2))
    got = E.main(['-d', data, '-m', out, '-sl', 'im', 'om'])
    exp = R.evaluate_cli(data, out, scenarios=('im', 'om'))
    assert len(got) == len(exp) == 2 and got[0].startswith('im,') and got[1].startswith('om,')
    for g, e in zip(got, exp):
        assert g.split(',')[0] == e.split(',')[0]
        assert [float(x) for x in g.split(',')[1:]] == [float(x) for x in e.split(',')[1:]]

    # fold_in is WMF's: the user half-step against the trained item table
    users = [u for u, x in enumerate(likes[0]) if len(x)][:3]
    hist = [likes[0][u] for u in users]
    rows = m.fold_in(hist)
    assert rows.shape == (3, m.k) and rows.dtype == np.float32
    step = dict(a=m.a, b=m.b, ridge_in_G=m.lu, ridge=0.0)
    x64, _ = A.half_step(np.zeros((3, m.k)), m.fie, hist, m.i_rated, dtype=np.float64, **step)
    x32, _ = A.half_step(np.zeros((3, m.k)), m.fie, hist, m.i_rated, dtype=np.float32, **step)
    ratio, err, e32 = _ratio(rows.astype(np.float64), x64, x32.astype(np.float64))
    print('K21 CER fold_in: err %.3g e32 %.3g ratio %.3g' % (err, e32, ratio))
    assert ratio <= F

    # the driver, the content through a pickle as load_content_data reads it
    pkl = str(tmp_path / 'meta.pkl')
    with open(pkl, 'wb') as fh:
        pickle.dump(m.feat, fh)
    out2 = str(tmp_path / 'cer2')
    hy = ['--lu', str(m.lu), '--lv', str(m.lv), '--le', str(m.le), '-k', str(m.k), '--seed', str(O.E2E['seed'])]
    model = train_als.main(['-d', _g2(golden_dir), '-o', out2, '--model', 'cer', '--content', pkl, '--dim', '24', '--iters', '6', '--tol', '0'] + hy)
    assert type(model).__name__ == 'CER' and sorted(os.listdir(out2)) == ['final-E.dat', 'final-U.dat', 'final-V.dat']
    np.testing.assert_array_equal(model.feat, m.feat)
    np.testing.assert_allclose(model.fie, m.fie, rtol=1e-4, atol=1e-6)           # the same seed, the same run
    np.testing.assert_allclose(model.E, m.E, rtol=1e-4, atol=1e-6)
    np.testing.assert_allclose(model.losses, m.losses, rtol=1e-6)
