"""K24 on the GPU (csrc/als_cg.hip, als.py solver='cg') against tests/_cg_oracle.py.

The yardstick of the solve is K20's: with x64 the float64 oracle on the same fp32 inputs and x32 the float32 one (the kernel's stated
order, operation by operation), e32 = max|x32 - x64| / max|x64| per case, and the kernel has to stay within F * max(e32, 2^-23).  An
unconverged conjugate-gradient iterate is sensitive to rounding (e32 reaches 0.5 at k = 512 after 8 steps), so what this holds the
kernel to is the float32 recurrence itself, which is the point: the kernel is that recurrence.  F is the next power of two at or above
twice the worst ratio measured on an MI355X; F <= 16 is a condition of the design.  Worst ratios per quantity:

    solve, X                                          3.99    (k = 64, 8 steps, n_x = 1, with a prior; nearly every other case 0.9 - 1.3)
    solve, row_loss                                   4.26    (the same case)
    the row of 2,100 likes, X / row_loss              1.00 / 1.00
    WMF on g2: fue / fie / losses                     0.89 / 0.97 / 0.77
    CER on g2: fue / fie / E / losses / cold items    1.00 / 0.99 / 1.01 / 0.80 / 0.97
    WMF.fold_in                                       1.08

Twice the worst is 8.5: F = 16.

The cases of test 3: every k of SOLVE_K with every step count of STEPS, with and without a prior, at one n_x each, dealt so that every
n_x of SOLVE_NX meets every step count (the width picks the kernel instantiation and the pitch, n_x the tile's tail: they do not
interact); and every n_x with every step count, with and without a prior, at k = 33."""
import ctypes as C
import functools
import os

import numpy as np
import pytest
import torch

import _als_oracle as O
import _cg_oracle as CG

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = 16.0
FLOOR = 2.0 ** -23
A, B = O.SOLVE_A, O.SOLVE_B


def _dev(a):
    return torch.from_numpy(np.array(a, order='C')).cuda()               # (a copy: the shared oracle arrays are read-only)


def _bits(a):
    return np.ascontiguousarray(a).view(np.int32 if a.dtype == np.float32 else np.int64)


def _ratio(got, x64, x32):
    scale = np.abs(x64).max()
    err, e32 = np.abs(got - x64).max() / scale, np.abs(x32 - x64).max() / scale
    return err / max(e32, FLOOR), err, e32


# ---- 1. the Gram, wide -----------------------------------------------------------------------------------------------------------------
def _exact_table(rng, n, k):
    return (rng.integers(-3, 4, (n, k)) / 8).astype(np.float32)


def _gram_np(Y, rows, scale, ridge):
    Yr = Y[rows].astype(np.float64)                                   # every sum is exact: multiples of 1/64 far below 2^24 of them
    return (scale * (Yr.T @ Yr) + ridge * np.eye(Y.shape[1])).astype(np.float32)


@pytest.mark.parametrize('k', [1, 33, 128, 129, 160, 256, 257, 512])
def test_gram_wide_is_exact_on_exact_inputs(k):
    """rows listed 1, 31, 33, 1025 and 2049 times (the last two cross a slab), with repeats and one row outside the table"""
    import tkr_hip
    rng = np.random.Generator(np.random.PCG64([24, k]))
    n = 57
    Y = _exact_table(rng, n, k)
    Yd = _dev(Y)
    for n_listed in (1, 31, 33, 1025, 2049):
        rows = rng.integers(0, n, n_listed).astype(np.int32)
        if n_listed >= 2:
            rows[1] = rows[0]
        for scale, ridge in ((0.5, 0.25), (1.0, 0.0)):
            G = tkr_hip.als_gram_wide(Yd, _dev(rows), scale=scale, ridge=ridge).cpu().numpy()
            np.testing.assert_array_equal(_bits(G), _bits(_gram_np(Y, rows, scale, ridge)), err_msg='a list of %d' % n_listed)
        bad = rows.copy()
        at = n_listed // 2
        bad[at] = n                                                   # outside: skipped and reported
        G, status = tkr_hip.als_gram_wide(Yd, _dev(bad), scale=0.5, ridge=2.0, check=False)
        assert int(status.item()) == 4 * at + 1
        np.testing.assert_array_equal(_bits(G.cpu().numpy()), _bits(_gram_np(Y, np.delete(rows, at), 0.5, 2.0)))
    G = tkr_hip.als_gram_wide(Yd, None, scale=0.5, ridge=0.25).cpu().numpy()      # rows = NULL: all n rows
    np.testing.assert_array_equal(_bits(G), _bits(_gram_np(Y, np.arange(n), 0.5, 0.25)))


@pytest.mark.parametrize('k', [5, 64, 128])
def test_gram_wide_has_the_bits_of_gram(k):
    import tkr_hip
    rng = np.random.Generator(np.random.PCG64([25, k]))
    Y = _dev(rng.standard_normal((1500, k), dtype=np.float32))
    rows = _dev(rng.integers(0, 1500, 2300).astype(np.int32))
    for r in (None, rows):
        want = tkr_hip.als_gram(Y, r, scale=0.01, ridge=0.1).cpu().numpy()
        got = tkr_hip.als_gram_wide(Y, r, scale=0.01, ridge=0.1).cpu().numpy()
        np.testing.assert_array_equal(_bits(got), _bits(want))


# ---- shared inputs ---------------------------------------------------------------------------------------------------------------------
W_PRIOR = 0.5


@functools.lru_cache(maxsize=None)
def _inputs(k, n_x, with_prior):
    """solve_inputs(k); with a prior a third of the rows lose their likes (every row is solved then) -> Y, X0, rows, rated, prior, ridge"""
    Y, X0, rows, rated = O.solve_inputs(k, n_x=n_x)
    prior, ridge = None, 0.01
    if with_prior:
        rows = [np.zeros(0, np.int64) if r % 3 == 1 else x for r, x in enumerate(rows)]
        prior = np.random.Generator(np.random.PCG64([26, k, n_x])).standard_normal((n_x, k), dtype=np.float32)
        prior.setflags(write=False)
        ridge = W_PRIOR
    for a in (Y, X0):
        a.setflags(write=False)
    return Y, X0, rows, rated, prior, ridge


def _hyper(prior, ridge):
    return dict(a=A, b=B, ridge_in_G=0.0, ridge=ridge, prior=prior, w_prior=W_PRIOR if prior is not None else 0.0)


@functools.lru_cache(maxsize=None)
def _oracle_case(k, steps, n_x, with_prior):
    Y, X0, rows, rated, prior, ridge = _inputs(k, n_x, with_prior)
    x64, l64 = CG.cg_half_step(X0, Y, rows, rated, steps=steps, dtype=np.float64, **_hyper(prior, ridge))
    x32, l32 = CG.cg_half_step(X0, Y, rows, rated, steps=steps, dtype=np.float32, **_hyper(prior, ridge))
    return x64, l64, x32, l32


def _gpu_solve(Y, X0, rows, rated, prior, ridge, steps, G=None, check=True, ptr=None):
    import tkr_hip
    p, cols = O.to_csr(rows)
    Yd = _dev(Y)
    if G is None:
        G = tkr_hip.als_gram_wide(Yd, _dev(np.asarray(rated, dtype=np.int32)), scale=B, ridge=0.0)
    X = _dev(X0)
    out = tkr_hip.als_cg_rows(Yd, G, _dev(p if ptr is None else ptr), _dev(cols), X, w_like=A - B, w_rhs=A, ridge=ridge, steps=steps,
                              prior=None if prior is None else _dev(prior), w_prior=W_PRIOR if prior is not None else 0.0, want_loss=True,
                              check=check)
    if check:
        return X.cpu().numpy(), out.cpu().numpy()
    return X.cpu().numpy(), out[0].cpu().numpy(), int(out[1].item())


# ---- 2. exact cases ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('with_prior', [False, True])
@pytest.mark.parametrize('k', [33, 129])
def test_no_steps_leave_x_and_give_the_loss(k, with_prior):
    """steps = 0 on exact inputs (multiples of 1/8, weights 1/2 and 1): every product and sum of the loss is exact in fp32 and fp64, so
    the kernel's loss IS the float64 oracle's"""
    import tkr_hip
    rng = np.random.Generator(np.random.PCG64([27, k]))
    n_y, n_x = 45, 37
    Y, X0 = _exact_table(rng, n_y, k), _exact_table(rng, n_x, k)
    rows = O.solve_inputs(k)[2]
    prior = _exact_table(rng, n_x, k) if with_prior else None
    if with_prior:
        rows = [np.zeros(0, np.int64) if r % 3 == 1 else x for r, x in enumerate(rows)]
    p, cols = O.to_csr(rows)
    Yd, X = _dev(Y), _dev(X0)
    G = tkr_hip.als_gram_wide(Yd, None, scale=0.5, ridge=0.0)
    loss = tkr_hip.als_cg_rows(Yd, G, _dev(p), _dev(cols), X, w_like=0.5, w_rhs=1.0, ridge=0.25, steps=0, prior=None if prior is None else _dev(prior),
                               w_prior=0.5 if with_prior else 0.0, want_loss=True).cpu().numpy()
    np.testing.assert_array_equal(_bits(X.cpu().numpy()), _bits(X0))
    _, want = CG.cg_half_step(X0, Y, rows, list(range(n_y)), a=1.0, b=0.5, ridge_in_G=0.0, ridge=0.25, steps=0, prior=prior,
                              w_prior=0.5 if with_prior else 0.0)
    assert want.any()
    np.testing.assert_array_equal(_bits(loss), _bits(want))


@pytest.mark.parametrize('k', [5, 129, 512])
def test_one_step_solves_a_multiple_of_the_identity(k):
    """a prior-mode call without likes, G = 3 I and ridge = 1: A = 4 I.  From x0 = 0 one step gives x = b / 4 bit for bit (p . q = 4 rho
    exactly: a power of two commutes with every rounding), a second step changes nothing (rho = 0 freezes the row), and a call that
    starts at the solution stores its bits"""
    import tkr_hip
    rng = np.random.Generator(np.random.PCG64([28, k]))
    n_x = 37
    prior = _exact_table(rng, n_x, k)
    prior[3] = 0                                                       # b = 0: rho = 0 from the start
    Y = _dev(np.zeros((4, k), np.float32))
    G = _dev(3 * np.eye(k, dtype=np.float32))
    ptr, cols = _dev(np.zeros(n_x + 1, np.int64)), torch.zeros(0, dtype=torch.int32, device='cuda')
    want = (0.5 * prior / 4).astype(np.float32)
    for steps, start in ((1, np.zeros_like(prior)), (2, np.zeros_like(prior)), (3, want)):
        X = _dev(start)
        loss = tkr_hip.als_cg_rows(Y, G, ptr, cols, X, w_like=0.99, w_rhs=1.0, ridge=1.0, steps=steps, prior=_dev(prior), w_prior=0.5, want_loss=True)
        np.testing.assert_array_equal(_bits(X.cpu().numpy()), _bits(want), err_msg='steps = %d' % steps)
        np.testing.assert_array_equal(loss.cpu().numpy(), 0.25 * ((want.astype(np.float64) - prior) ** 2).sum(axis=1))


# ---- 3. against the float64 oracle -------------------------------------------------------------------------------------------------------
SOLVE_K = [1, 5, 32, 33, 64, 65, 128, 129, 200, 256, 257, 512]
STEPS = [1, 3, 8]
SOLVE_NX = [1, 31, 32, 33, 37, 65]


def _against_oracle(k, steps, n_x, with_prior):
    Y, X0, rows, rated, prior, ridge = _inputs(k, n_x, with_prior)
    x64, l64, x32, l32 = _oracle_case(k, steps, n_x, with_prior)
    X, loss = _gpu_solve(Y, X0, rows, rated, prior, ridge, steps)
    assert np.isfinite(X).all()
    if prior is None:
        empty = [r for r, likes in enumerate(rows) if len(likes) == 0]
        np.testing.assert_array_equal(_bits(X[empty]), _bits(X0[empty]))            # rows without likes: bit for bit as they were
        assert not loss[empty].any()
    rx, ex, e32x = _ratio(X.astype(np.float64), x64, x32.astype(np.float64))
    rl, el, e32l = _ratio(loss, l64, l32)
    print('K24 cg k=%d steps=%d n_x=%d prior=%d: x err %.3g e32 %.3g ratio %.3g; loss err %.3g e32 %.3g ratio %.3g'
          % (k, steps, n_x, with_prior, ex, e32x, rx, el, e32l, rl))
    assert rx <= F, (ex, e32x)
    assert rl <= F, (el, e32l)


@pytest.mark.parametrize('with_prior', [False, True])
@pytest.mark.parametrize('steps', STEPS)
@pytest.mark.parametrize('k', SOLVE_K)
def test_cg_rows_against_the_oracle(k, steps, with_prior):
    _against_oracle(k, steps, SOLVE_NX[(SOLVE_K.index(k) + STEPS.index(steps)) % len(SOLVE_NX)], with_prior)


@pytest.mark.parametrize('with_prior', [False, True])
@pytest.mark.parametrize('steps', STEPS)
@pytest.mark.parametrize('n_x', SOLVE_NX)
def test_cg_rows_around_the_tile(n_x, steps, with_prior):
    _against_oracle(33, steps, n_x, with_prior)


def test_a_row_longer_than_the_like_loop_walks_at_once():
    """2,100 likes over 45 columns (repeats): the like loop takes 64 columns at a time"""
    k, ridge, steps = 33, 0.01, 3
    rng = np.random.Generator(np.random.PCG64(29))
    Y, X0 = rng.random((45, k), dtype=np.float32), rng.random((3, k), dtype=np.float32)
    rows = [rng.integers(0, 45, 2100), np.zeros(0, np.int64), rng.integers(0, 45, 70)]
    rated = list(range(45))
    X, loss = _gpu_solve(Y, X0, rows, rated, None, ridge, steps)
    x64, l64 = CG.cg_half_step(X0, Y, rows, rated, steps=steps, **_hyper(None, ridge))
    x32, l32 = CG.cg_half_step(X0, Y, rows, rated, steps=steps, dtype=np.float32, **_hyper(None, ridge))
    rx, ex, e32x = _ratio(X.astype(np.float64), x64, x32.astype(np.float64))
    rl, el, e32l = _ratio(loss, l64, l32)
    print('K24 cg long row: x err %.3g e32 %.3g ratio %.3g; loss err %.3g e32 %.3g ratio %.3g' % (ex, e32x, rx, el, e32l, rl))
    np.testing.assert_array_equal(_bits(X[1]), _bits(X0[1]))
    assert rx <= F and rl <= F


# ---- 4. a row's bits are its own ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('with_prior', [False, True])
@pytest.mark.parametrize('k', [33, 200])
def test_the_bits_of_a_row_do_not_depend_on_the_call(k, with_prior):
    import tkr_hip
    Y, X0, rows, rated, prior, ridge = _inputs(k, 65, with_prior)
    G = tkr_hip.als_gram_wide(_dev(Y), _dev(np.asarray(rated, dtype=np.int32)), scale=B, ridge=0.0)
    X, loss = _gpu_solve(Y, X0, rows, rated, prior, ridge, 3, G=G)
    X2, loss2 = _gpu_solve(Y, X0, rows, rated, prior, ridge, 3, G=G)
    np.testing.assert_array_equal(_bits(X), _bits(X2))                              # two calls, the same bits
    np.testing.assert_array_equal(_bits(loss), _bits(loss2))
    assert (X != X0).any()
    for pick in ([0], [31, 32], [64]):
        Xs, ls = _gpu_solve(Y, X0[pick], [rows[r] for r in pick], rated, None if prior is None else prior[pick], ridge, 3, G=G)
        np.testing.assert_array_equal(_bits(Xs), _bits(X[pick]), err_msg=str(pick))
        np.testing.assert_array_equal(_bits(ls), _bits(loss[pick]), err_msg=str(pick))


# ---- 5. converged CG is the solve --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('k', [5, 50, 128, 200])
def test_converged_cg_meets_the_backward_error_of_the_solve(k):
    """2 k steps from x0 = 0: || (A64 + ridge I) x - rhs64 ||_inf <= (3 k^2 + m + n_rated + 8) 2^-24 (||A64 + ridge I||_inf ||x||_inf +
    ||rhs64||_inf), the bound of test_solve_rows_backward_error (tests/test_gpu_als.py).  The float32 ORACLE meets it on these inputs at
    2 k steps (worst residual / bound 0.013, 6.1e-4, 3.3e-5, 1.1e-5 at k = 5, 50, 128, 200; at k steps it does not yet at k = 5), so
    2 k steps is what the kernel is held to."""
    ridge = 0.01
    Y, X0, rows, rated = O.solve_inputs(k)
    X, _ = _gpu_solve(Y, np.zeros_like(X0), rows, rated, None, ridge, 2 * k)
    X = X.astype(np.float64)
    Y64 = Y.astype(np.float64)
    G = O.gram(Y64, rated, B, 0.0)
    worst = 0.0
    for r, likes in enumerate(rows):
        if len(likes) == 0:
            assert not X[r].any()
            continue
        y = Y64[likes]
        Am = G + (A - B) * (y.T @ y) + ridge * np.eye(k)
        rhs = A * y.sum(axis=0)
        bound = (3 * k * k + len(likes) + len(rated) + 8) * 2.0 ** -24 * (np.abs(Am).sum(axis=1).max() * np.abs(X[r]).max() + np.abs(rhs).max())
        res = np.abs(Am @ X[r] - rhs).max()
        worst = max(worst, res / bound)
        assert res <= bound, (r, len(likes), res, bound)
    print('K24 backward error k=%d after %d steps: worst residual / bound %.3g' % (k, 2 * k, worst))


# ---- 6. untrusted input ------------------------------------------------------------------------------------------------------------------
def test_like_columns_outside_the_table_are_skipped():
    """kind 1: the row is solved with the likes that are left, in their order -- the bits of the call on the cleaned list"""
    k = 33
    Y, X0, rows, rated, prior, ridge = _inputs(k, 37, False)
    n_y = len(Y)
    dirty = [np.asarray(x, dtype=np.int64) for x in rows]
    dirty[4] = np.concatenate([dirty[4][:3], [-1], dirty[4][3:], [n_y]])
    dirty[2] = np.concatenate([[n_y], dirty[2]])
    dirty[11] = np.asarray([-1, n_y])                                           # nothing left: as a row without likes
    clean = list(rows)
    clean[11] = np.zeros(0, np.int64)
    X, loss, status = _gpu_solve(Y, X0, dirty, rated, None, ridge, 3, check=False)
    assert status == 4 * 2 + 1
    Xc, lc = _gpu_solve(Y, X0, clean, rated, None, ridge, 3)
    np.testing.assert_array_equal(_bits(X), _bits(Xc))
    np.testing.assert_array_equal(_bits(loss), _bits(lc))
    np.testing.assert_array_equal(_bits(X[11]), _bits(X0[11]))
    assert loss[11] == 0.0


def test_descending_like_ptr_leaves_the_row_and_the_smallest_word_is_reported():
    import tkr_hip
    k = 16
    Y, X0, rows, rated, prior, ridge = _inputs(k, 37, False)
    ptr, cols = O.to_csr(rows)
    ptr = ptr.copy()
    ptr[6] = ptr[5] - 1                                                         # row 5 descends; row 6 is a row again, longer by what row 5 had
    X, loss, status = _gpu_solve(Y, X0, rows, rated, None, ridge, 3, check=False, ptr=ptr)
    assert status == 4 * 5 + 3
    np.testing.assert_array_equal(_bits(X[5]), _bits(X0[5]))
    assert loss[5] == 0.0 and np.isfinite(X).all()
    changed = [r for r in range(len(rows)) if r != 5 and ptr[r + 1] > ptr[r]]
    assert all((X[r] != X0[r]).any() for r in changed)
    dirty = [np.asarray(x, dtype=np.int64) for x in rows]
    dirty[2] = np.concatenate([[len(Y)], dirty[2]])                             # kind 1 at row 2 and kind 3 at row 5: the smaller word
    p2, c2 = O.to_csr(dirty)
    p2 = p2.copy()
    p2[6] = p2[5] - 1
    Yd = _dev(Y)
    G = tkr_hip.als_gram_wide(Yd, None, scale=B, ridge=0.0)
    _, st = tkr_hip.als_cg_rows(Yd, G, _dev(p2), _dev(c2), _dev(X0), w_like=A - B, w_rhs=A, ridge=ridge, steps=3, check=False)
    assert int(st.item()) == 4 * 2 + 1
    with pytest.raises(tkr_hip.AlsCgRefused) as info:
        tkr_hip.als_cg_rows(Yd, G, _dev(ptr), _dev(cols), _dev(X0), w_like=A - B, w_rhs=A, ridge=ridge, steps=3)
    assert (info.value.row, info.value.kind) == (5, 3)


def test_a_direction_of_no_positive_curvature_is_refused():
    """G = -I: p . q <= 0 at the first step of every row with likes (kind 2): the rows stay as they came in, no NaN anywhere"""
    import tkr_hip
    for k in (7, 129):
        Y, X0, rows, rated, prior, ridge = _inputs(k, 37, False)
        G = _dev(-np.eye(k, dtype=np.float32))
        X, loss, status = _gpu_solve(Y * 0, X0, rows, rated, None, 0.0, 3, G=G, check=False)
        first = min(r for r, x in enumerate(rows) if len(x))
        assert status == 4 * first + 2
        np.testing.assert_array_equal(_bits(X), _bits(X0))
        assert not loss.any()


def test_a_prior_that_is_not_finite_refuses_its_row_only():
    k = 33
    Y, X0, rows, rated, prior, ridge = _inputs(k, 37, True)
    bad = prior.copy()
    bad[9, 4] = np.inf
    bad[20, 0] = np.nan
    X, loss, status = _gpu_solve(Y, X0, rows, rated, bad, ridge, 3, check=False)
    assert status == 4 * 9 + 2
    Xg, lg = _gpu_solve(Y, X0, rows, rated, prior, ridge, 3)
    others = [r for r in range(37) if r not in (9, 20)]
    np.testing.assert_array_equal(_bits(X[others]), _bits(Xg[others]))
    np.testing.assert_array_equal(_bits(loss[others]), _bits(lg[others]))
    np.testing.assert_array_equal(_bits(X[[9, 20]]), _bits(X0[[9, 20]]))
    assert not loss[[9, 20]].any() and np.isfinite(X).all()


# ---- 7. end to end on tests/golden/g2 -----------------------------------------------------------------------------------------------------
def _g2(golden_dir):
    return os.path.join(golden_dir, 'g2')


def _wmf(golden_dir, k=O.E2E['k']):
    import als
    d = _g2(golden_dir)
    m = als.WMF(k=k, lu=O.E2E['lu'], lv=O.E2E['lv'], solver='cg')
    m.load_training_data(os.path.join(d, 'uid'), os.path.join(d, 'vid'), os.path.join(d, 'f0tr.txt'), seed=O.E2E['seed'])
    return m


def _likes(m):
    up, uc, ip, ic = m._csr
    return O.csr_rows(up, uc), O.csr_rows(ip, ic)


@functools.lru_cache(maxsize=None)
def _trained(golden_dir):
    m = _wmf(golden_dir)
    U0, V0 = m.fue.copy(), m.fie.copy()
    likes = _likes(m)
    hyper = dict(a=m.a, b=m.b, lu=m.lu, lv=m.lv)
    m.train(max_iter=O.E2E['iters'], tol=0.0, verbose=False)
    t64 = CG.train_cg(U0, V0, *likes, max_iter=O.E2E['iters'], tol=0.0, steps=3, dtype=np.float64, **hyper)
    t32 = CG.train_cg(U0, V0, *likes, max_iter=O.E2E['iters'], tol=0.0, steps=3, dtype=np.float32, **hyper)
    return m, U0, V0, likes, hyper, t64, t32


def test_wmf_cg_trains_as_the_oracle(golden_dir):
    m, U0, V0, likes, hyper, (U64, V64, l64), (U32, V32, l32) = _trained(golden_dir)
    assert len(m.losses) == O.E2E['iters'] == len(l64)
    assert all(later < earlier for earlier, later in zip([np.exp(50)] + m.losses, m.losses)), m.losses
    assert m.fue.dtype == np.float32 and m.fue.shape == U0.shape and m.fie.shape == V0.shape
    for name, got, x64, x32 in (('fue', m.fue, U64, U32), ('fie', m.fie, V64, V32), ('losses', np.asarray(m.losses), np.asarray(l64), np.asarray(l32))):
        ratio, err, e32 = _ratio(got.astype(np.float64), x64, x32.astype(np.float64))
        print('K24 WMF cg %s after %d iterations: err %.3g e32 %.3g ratio %.3g' % (name, O.E2E['iters'], err, e32, ratio))
        assert ratio <= F, (name, err, e32)
    for i, (got, x64, x32) in enumerate(zip(m.losses, l64, l32)):                    # every loss, each on its own scale
        assert abs(got - x64) <= F * max(abs(x32 - x64), FLOOR * abs(x64)), (i, got, x64, x32)
    no_u = [u for u, x in enumerate(likes[0]) if len(x) == 0]
    assert no_u                                                                # g2 has users without a training like
    np.testing.assert_array_equal(_bits(m.fue[no_u]), _bits(U0[no_u]))


def test_wmf_cg_stops_where_the_oracle_stops(golden_dir):
    m, U0, V0, likes, hyper = _trained(golden_dir)[:5]
    fresh = _wmf(golden_dir)
    np.testing.assert_array_equal(fresh.fue, U0)
    fresh.train(max_iter=200, tol=1e-2, verbose=False)
    stop64 = len(CG.train_cg(U0, V0, *likes, max_iter=200, tol=1e-2, steps=3, **hyper)[2])
    assert 1 < stop64 < 200 and len(fresh.losses) == stop64


def test_cer_cg_trains_as_the_oracle(golden_dir):
    import als
    import _cer_oracle as CO
    d = _g2(golden_dir)
    e = CO.E2E
    m = als.CER(k=e['k'], d=e['d'], lu=e['lu'], lv=e['lv'], le=e['le'], a=e['a'], b=e['b'], solver='cg')
    m.load_training_data(os.path.join(d, 'uid'), os.path.join(d, 'vid'), os.path.join(d, 'f0tr.txt'), seed=e['seed'])
    m.feat = CO.e2e_features(m.n_items)
    U0, V0, E0 = CO.e2e_start(m.n_users, m.n_items)
    likes = _likes(m)
    hyper = dict(a=m.a, b=m.b, lu=m.lu, lv=m.lv, le=m.le)
    m.train(max_iter=e['iters'], tol=0.0, verbose=False)
    U64, V64, E64, l64 = CG.cer_train_cg(U0, V0, E0, m.feat, *likes, max_iter=e['iters'], tol=0.0, dtype=np.float64, **hyper)
    U32, V32, E32, l32 = CG.cer_train_cg(U0, V0, E0, m.feat, *likes, max_iter=e['iters'], tol=0.0, dtype=np.float32, **hyper)
    assert len(m.losses) == e['iters'] == len(l64)
    for name, got, x64, x32 in (('fue', m.fue, U64, U32), ('fie', m.fie, V64, V32), ('E', m.E, E64, E32),
                                ('losses', np.asarray(m.losses), np.asarray(l64), np.asarray(l32))):
        ratio, err, e32 = _ratio(got.astype(np.float64), x64, x32.astype(np.float64))
        print('K24 CER cg %s after %d iterations: err %.3g e32 %.3g ratio %.3g' % (name, e['iters'], err, e32, ratio))
        assert ratio <= F, (name, err, e32)
    cold = [j for j, x in enumerate(likes[1]) if len(x) == 0]
    assert len(cold) == 4
    ratio, err, e32 = _ratio(m.fie[cold].astype(np.float64), V64[cold], V32[cold].astype(np.float64))
    print('K24 CER cg cold items: err %.3g e32 %.3g ratio %.3g' % (err, e32, ratio))
    assert ratio <= F
    np.testing.assert_array_equal(m.fie[cold], m.embed_items(m.feat[cold]))        # E^T f, the fp64 product rounded once
    fresh = als.CER(k=e['k'], d=e['d'], lu=e['lu'], lv=e['lv'], le=e['le'], a=e['a'], b=e['b'], solver='cg')
    fresh.load_training_data(os.path.join(d, 'uid'), os.path.join(d, 'vid'), os.path.join(d, 'f0tr.txt'), seed=e['seed'])
    fresh.feat = m.feat
    fresh.train(max_iter=200, tol=1e-2, verbose=False)
    stop64 = len(CG.cer_train_cg(U0, V0, E0, m.feat, *likes, max_iter=200, tol=1e-2, **hyper)[3])
    assert 1 < stop64 < 200 and len(fresh.losses) == stop64


def test_wmf_cg_at_width_160_serves_evaluate(golden_dir, tmp_path):
    """a width the Cholesky path refuses: 3 iterations, the export, and evaluate.py -m on the directory (K4's width path)"""
    import evaluate as E
    from oracle import ref_np as R
    m = _wmf(golden_dir, k=160)
    m.train(max_iter=3, tol=0.0, verbose=False)
    assert len(m.losses) == 3 and all(later < earlier for earlier, later in zip(m.losses, m.losses[1:])), m.losses
    assert m.fue.shape == (m.n_users, 160) and np.isfinite(m.fue).all() and np.isfinite(m.fie).all()
    out = str(tmp_path / 'wmf160')
    m.export_embeddings(out)
    assert sorted(os.listdir(out)) == ['final-U.dat', 'final-V.dat']
    got = E.main(['-d', _g2(golden_dir), '-m', out, '-sl', 'im'])
    exp = R.evaluate_cli(_g2(golden_dir), out, scenarios=('im',))
    assert len(got) == len(exp) == 1 and got[0].startswith('im,')
    assert [float(x) for x in got[0].split(',')[1:]] == [float(x) for x in exp[0].split(',')[1:]]


def test_wmf_cg_fold_in_is_the_user_half_step_from_zero(golden_dir):
    m, U0, V0, likes, hyper = _trained(golden_dir)[:5]
    users = [u for u, x in enumerate(likes[0]) if len(x)][:3]
    hist = [likes[0][u] for u in users]
    got = m.fold_in(hist)
    assert got.shape == (3, m.k) and got.dtype == np.float32
    step = dict(a=m.a, b=m.b, ridge_in_G=m.lu, ridge=0.0, steps=m.k)
    x64, _ = CG.cg_half_step(np.zeros((3, m.k)), m.fie, hist, m.i_rated, dtype=np.float64, **step)
    x32, _ = CG.cg_half_step(np.zeros((3, m.k)), m.fie, hist, m.i_rated, dtype=np.float32, **step)
    ratio, err, e32 = _ratio(got.astype(np.float64), x64, x32.astype(np.float64))
    print('K24 WMF cg fold_in: err %.3g e32 %.3g ratio %.3g' % (err, e32, ratio))
    assert ratio <= F
    np.testing.assert_array_equal(_bits(m.fold_in(hist, steps=m.k)), _bits(got))


def test_train_als_with_the_cg_solver_writes_the_model(golden_dir, tmp_path):
    import train_als
    out = str(tmp_path / 'wmf_cg')
    model = train_als.main(['-d', _g2(golden_dir), '-o', out, '-k', '16', '--solver', 'cg', '--cg-steps', '2', '--iters', '3', '--tol', '0',
                            '--lu', '0.1', '--lv', '0.1', '--seed', '0'])
    assert type(model).__name__ == 'WMF' and (model.solver, model.cg_steps) == ('cg', 2) and len(model.losses) == 3
    assert sorted(os.listdir(out)) == ['final-U.dat', 'final-V.dat']


# ---- the raw ABI ---------------------------------------------------------------------------------------------------------------------------
def test_raw_abi_through_ctypes():
    """the symbols as a maintainer of the reference would bind them: no helper module in between"""
    lib = C.CDLL(os.path.join(ROOT, 'top-k-rec_amd', 'libtkr_hip.so'))
    V = C.c_void_p
    gram, solve, size = lib.tkr_als_gram_wide, lib.tkr_als_cg_rows, lib.tkr_als_gram_wide_workspace_bytes
    gram.restype = solve.restype = C.c_int
    size.restype = C.c_int64
    size.argtypes = [C.c_int32, C.c_int64]
    gram.argtypes = [V, C.c_int32, C.c_int32, V, C.c_int64, C.c_double, C.c_double, V, V, C.c_int64, V, V]
    solve.argtypes = [V, C.c_int32, C.c_int32, V, V, V, C.c_int64, C.c_int64, C.c_double, C.c_double, C.c_double, C.c_int32, V, V, V, C.c_double, V,
                      C.c_int64, V, V]
    k, ridge = 140, 0.01
    Y, X0, rows, rated = O.solve_inputs(k, n_x=9, n_y=20)
    ptr, cols = O.to_csr(rows)
    Yd, Xd, pd, cd, rd = _dev(Y), _dev(X0.copy()), _dev(ptr), _dev(cols), _dev(np.asarray(rated, dtype=np.int32))
    G = torch.empty((k, k), dtype=torch.float32, device='cuda')
    loss = torch.empty(9, dtype=torch.float64, device='cuda')
    status = torch.empty(1, dtype=torch.int64, device='cuda')
    ws = torch.empty(size(k, 1) // 8, dtype=torch.int64, device='cuda')
    stream = V(torch.cuda.current_stream().cuda_stream)
    p = lambda t: V(t.data_ptr())
    assert gram(p(Yd), 20, k, p(rd), len(rated), B, 0.0, p(G), p(ws), ws.numel() * 8, p(status), stream) == 0
    assert int(status.item()) == -1
    s_args = [p(Yd), 20, k, p(G), p(pd), p(cd), len(cols), 9, A - B, A, ridge, 3, p(Xd), p(loss), None, 0.0, None, 0, p(status), stream]
    assert solve(*s_args) == 0
    assert int(status.item()) == -1
    x64, l64 = CG.cg_half_step(X0, Y, rows, rated, steps=3, **_hyper(None, ridge))
    x32, l32 = CG.cg_half_step(X0, Y, rows, rated, steps=3, dtype=np.float32, **_hyper(None, ridge))
    assert _ratio(Xd.cpu().numpy().astype(np.float64), x64, x32.astype(np.float64))[0] <= F
    assert _ratio(loss.cpu().numpy(), l64, l32)[0] <= F
    before = Xd.clone()
    for at, bad, rc in ((0, None, -1), (2, 513, -2), (11, -1, -1), (10, -0.5, -1), (7, 0, -1)):
        args = list(s_args)
        args[at] = bad
        assert solve(*args) == rc, at
    torch.cuda.synchronize()
    assert torch.equal(before, Xd)
