"""K24 (the ALS half-step by conjugate gradients) without a GPU: the oracle of tests/_cg_oracle.py against itself and against the direct
solve of tests/_als_oracle.py, the constructor rules of als.WMF / CER / DPM under solver='cg', and everything of the C ABI that is
checked before a device is touched."""
import ctypes
import os
import re

import numpy as np
import pytest

import _als_oracle as O
import _cg_oracle as CG

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HYPER = dict(a=O.SOLVE_A, b=O.SOLVE_B, ridge_in_G=0.0, ridge=0.01)


@pytest.mark.parametrize('k', [5, 33, 129])
def test_float64_cg_converges_to_the_direct_solve(k):
    """conjugate gradients end after at most k steps in exact arithmetic: in float64, 2 k steps from the start of solve_inputs(k)
    reproduce np.linalg.solve to 1e-10 of the largest entry, and 3 steps from the direct solution return it.

    The first statement is made with the recurrence's exit rho < 1e-20 switched off (done=0): that exit is an ABSOLUTE residual of
    1e-10, and on these systems (smallest eigenvalue near ridge = 0.01) it leaves an error of 1.7e-11 / 1.6e-9 / 3.1e-10 of the largest
    entry at k = 5 / 33 / 129 -- it would be the exit, not the recurrence, that the 1e-10 measures.  Without it: 9.5e-15 / 2.5e-12 /
    5.1e-11.  The figures with the exit are printed, and held to the bound the exit itself implies, sqrt(1e-20) / ridge."""
    Y, X0, rows, rated = O.solve_inputs(k)
    direct, loss_direct = O.half_step(X0, Y, rows, rated, **HYPER)
    scale = np.abs(direct).max()
    x, loss = CG.cg_half_step(X0, Y, rows, rated, steps=2 * k, done=0.0, **HYPER)
    with_exit, _ = CG.cg_half_step(X0, Y, rows, rated, steps=2 * k, **HYPER)
    err, err_exit = np.abs(x - direct).max() / scale, np.abs(with_exit - direct).max() / scale
    print('K24 float64 CG k=%d, 2k steps: %.3g of the largest entry (with the exit rho < 1e-20: %.3g)' % (k, err, err_exit))
    assert err <= 1e-10
    assert np.abs(loss - loss_direct).max() <= 1e-10 * np.abs(loss_direct).max()
    assert err_exit * scale <= 1e-10 / HYPER['ridge']
    again, loss_again = CG.cg_half_step(direct, Y, rows, rated, steps=3, **HYPER)
    assert np.abs(again - direct).max() <= 1e-10 * scale
    assert np.abs(loss_again - loss_direct).max() <= 1e-10 * np.abs(loss_direct).max()
    empty = [r for r, likes in enumerate(rows) if len(likes) == 0]
    np.testing.assert_array_equal(x[empty], X0[empty].astype(np.float64))
    assert not loss[empty].any()


def test_float32_cg_follows_float64_and_a_prior_solves_every_row():
    k = 33
    Y, X0, rows, rated = O.solve_inputs(k)
    x64, l64 = CG.cg_half_step(X0, Y, rows, rated, steps=3, **HYPER)
    x32, l32 = CG.cg_half_step(X0, Y, rows, rated, steps=3, dtype=np.float32, **HYPER)
    assert x32.dtype == np.float32 and np.abs(x32 - x64).max() <= 1e-2 * np.abs(x64).max() and np.abs(l32 - l64).max() <= 1e-2 * np.abs(l64).max()
    rng = np.random.Generator(np.random.PCG64(5))
    prior = rng.standard_normal((len(rows), k))
    x, loss = CG.cg_half_step(X0, Y, rows, rated, steps=2 * k, prior=prior, w_prior=0.7, done=0.0, **{**HYPER, 'ridge': 0.7})
    G = O.gram(Y.astype(np.float64), rated, O.SOLVE_B, 0.0)
    for r, likes in enumerate(rows):
        y = Y[likes].astype(np.float64)
        A = G + (O.SOLVE_A - O.SOLVE_B) * (y.T @ y)
        grad = (A + 0.7 * np.eye(k)) @ x[r] - O.SOLVE_A * y.sum(axis=0) - 0.7 * prior[r]
        assert np.abs(grad).max() <= 1e-9 * (1.0 + np.abs(prior[r]).max())
        fit = 0.5 * x[r] @ A @ x[r] - O.SOLVE_A * (y @ x[r]).sum() + 0.5 * O.SOLVE_A * len(likes) if len(likes) else 0.0
        assert abs(fit + 0.35 * ((x[r] - prior[r]) ** 2).sum() - loss[r]) <= 1e-9 * max(1.0, abs(loss[r]))


def test_dot32_is_the_stated_tree():
    rng = np.random.Generator(np.random.PCG64(9))
    for k in (1, 63, 64, 65, 200, 512):
        a, b = rng.standard_normal(k).astype(np.float32), rng.standard_normal(k).astype(np.float32)
        got = CG.dot32(a, b)
        assert got.dtype == np.float32 and abs(float(got) - float(a.astype(np.float64) @ b.astype(np.float64))) <= 2.0 ** -20 * float(np.abs(a * b).sum())
    e = (np.arange(70) % 5 - 2).astype(np.float32) / 4                          # exact: every order gives the same sum
    assert float(CG.dot32(e, e)) == float((e.astype(np.float64) ** 2).sum())


def test_constructor_rules():
    import als
    assert als.WMF(k=129, solver='cg').k == 129 and als.WMF(k=512, solver='cg').solver == 'cg'
    m = als.CER(k=200, d=8, solver='cg', cg_steps=5)
    assert (m.k, m.solver, m.cg_steps) == (200, 'cg', 5)
    assert (als.WMF(k=8).solver, als.WMF(k=8).cg_steps) == ('cholesky', 3)
    assert als.DPM(k=128, d=8, solver='cg').solver == 'cg'
    for make in (lambda: als.WMF(k=513, solver='cg'), lambda: als.CER(k=513, d=8, solver='cg'), lambda: als.DPM(k=129, d=8, solver='cg'),
                 lambda: als.WMF(k=8, solver='qr'), lambda: als.WMF(k=8, cg_steps=0), lambda: als.WMF(k=8, solver='cg', cg_steps=0),
                 lambda: als.WMF(k=8, solver='cg', cg_steps=2.5), lambda: als.WMF(k=129), lambda: als.CER(k=129, d=8), lambda: als.DPM(k=129, d=8),
                 lambda: als.MLP(k=129, d=8), lambda: als.WMF(k=0, solver='cg')):
        with pytest.raises(ValueError):
            make()
    with pytest.raises(ValueError, match='MLP'):
        als.DPM(k=129, d=8, solver='cg')
    with pytest.raises(ValueError, match="solver='cg'"):
        als.WMF(k=8).fold_in([[1]], steps=4)                                    # steps is conjugate gradients' argument


def test_train_als_takes_the_solver(tmp_path):
    import train_als
    for argv in (['--solver', 'qr'], ['--solver', 'cg', '-k', '513'], ['--solver', 'cg', '--cg-steps', '0'], ['-k', '129'],
                 ['--model', 'dpm', '--content', 'x.pkl', '--dim', '3', '--solver', 'cg', '-k', '129']):
        with pytest.raises(SystemExit):
            train_als.main(argv + ['-d', str(tmp_path)])


def test_library_declares_and_exports_the_new_symbols():
    import tkr_hip
    header = open(os.path.join(ROOT, 'include', 'tkr.h')).read()
    declared = set(re.findall(r'^int(?:32_t|64_t)? (tkr_\w+)\(', header, flags=re.M))
    for name in ('tkr_als_cg_rows', 'tkr_als_gram_wide'):
        assert name in declared and name in tkr_hip.EXPORTS
    for name in ('tkr_als_cg_workspace_bytes', 'tkr_als_gram_wide_workspace_bytes'):
        assert name in declared and name in tkr_hip.EXPORTS_I64
    assert re.search(r'#define TKR_ALS_CG_MAX_K 512\b', header) and re.search(r'#define TKR_ALS_MAX_K 128\b', header)
    assert (tkr_hip.ALS_CG_MAX_K, tkr_hip.ALS_CG_STEPS, tkr_hip.ALS_MAX_K) == (512, 3, 128)


def _lib():
    import tkr_hip
    return ctypes.CDLL(tkr_hip.LIB_PATH) if os.path.exists(tkr_hip.LIB_PATH) else None      # (as tests/test_cer_cpu.py: a tree not built yet)


def test_size_functions():
    lib = _lib()
    if lib is None:
        return
    cg, wide, k20 = lib.tkr_als_cg_workspace_bytes, lib.tkr_als_gram_wide_workspace_bytes, lib.tkr_als_workspace_bytes
    cg.restype = wide.restype = k20.restype = ctypes.c_int64
    cg.argtypes = [ctypes.c_int64, ctypes.c_int32]
    wide.argtypes = [ctypes.c_int32, ctypes.c_int64]
    k20.argtypes = [ctypes.c_int64, ctypes.c_int32, ctypes.c_int64]
    assert cg(10, 513) < 0 and cg(10, 0) < 0 and cg(-1, 8) < 0 and cg(10, 512) >= 0 and cg(10, 1) >= 0
    assert wide(513, 1) < 0 and wide(0, 1) < 0 and wide(8, -1) < 0
    for k, s in ((512, 3), (1, 1), (129, 70), (50, 0)):
        assert wide(k, s) % 16 == 0 and wide(k, s) >= s * k * k * 4
    assert k20(10, 129, 0) == -1                                                 # K20's bound has not moved


def test_raw_abi_refuses_before_any_device_access():
    """every refused argument returns TKR_E_INVAL (-1) or TKR_E_UNSUPPORTED (-2) before anything is launched: the pointers below are
    addresses nobody owns, and this machine may have no device"""
    lib = _lib()
    if lib is None:
        return
    V = ctypes.c_void_p
    solve, gram = lib.tkr_als_cg_rows, lib.tkr_als_gram_wide
    solve.restype = gram.restype = ctypes.c_int
    solve.argtypes = [V, ctypes.c_int32, ctypes.c_int32, V, V, V, ctypes.c_int64, ctypes.c_int64, ctypes.c_double, ctypes.c_double, ctypes.c_double,
                      ctypes.c_int32, V, V, V, ctypes.c_double, V, ctypes.c_int64, V, V]
    gram.argtypes = [V, ctypes.c_int32, ctypes.c_int32, V, ctypes.c_int64, ctypes.c_double, ctypes.c_double, V, V, ctypes.c_int64, V, V]
    P = 0x10000                                                                 # aligned, never followed
    #        Y  n_y k  G  ptr cols n_likes n_x w_like w_rhs ridge steps X  loss prior w_prior ws  bytes status stream
    good = [P, 5, 4, P, P, P, 7, 3, 0.99, 1.0, 0.1, 3, P, P, P, 1.0, None, 0, P, None]
    nan, inf = float('nan'), float('inf')
    walk = [(0, None, -1), (3, None, -1), (4, None, -1), (12, None, -1), (18, None, -1), (5, None, -1),          # null pointers (cols with n_likes > 0)
            (0, P + 2, -1), (3, P + 1, -1), (12, P + 2, -1), (14, P + 2, -1), (4, P + 4, -1), (5, P + 2, -1), (18, P + 4, -1), (13, P + 4, -1),
            (16, P + 8, -1),                                                                                       # misaligned
            (2, 0, -1), (2, -3, -1), (2, 513, -2), (1, 0, -1), (7, 0, -1), (7, 1 << 31, -1), (6, -1, -1), (11, -1, -1), (17, -1, -1),
            (8, nan, -1), (8, inf, -1), (9, nan, -1), (10, nan, -1), (10, -0.5, -1), (15, -1.0, -1), (15, inf, -1)]
    for at, bad, rc in walk:
        args = list(good)
        args[at] = bad
        assert solve(*args) == rc, (at, bad)
    #         Y  n  k  rows n_listed scale ridge G  ws bytes status stream
    good = [P, 5, 4, P, 3, 0.5, 0.25, P, P, 1 << 20, P, None]
    for at, bad, rc in ((0, None, -1), (7, None, -1), (10, None, -1), (10, P + 4, -1), (8, P + 4, -1), (2, 0, -1), (2, 513, -2), (1, 0, -1), (4, -1, -1),
                        (9, -1, -1), (8, None, -1), (9, 8, -1), (5, nan, -1), (6, inf, -1)):
        args = list(good)
        args[at] = bad
        assert gram(*args) == rc, (at, bad)


def _g2_model(golden_dir, **over):
    import als
    d = os.path.join(golden_dir, 'g2')
    m = als.WMF(k=O.E2E['k'], lu=O.E2E['lu'], lv=O.E2E['lv'], **over)
    m.load_training_data(os.path.join(d, 'uid'), os.path.join(d, 'vid'), os.path.join(d, 'f0tr.txt'), seed=O.E2E['seed'])
    return m


def test_model_quality_of_three_steps_on_g2(golden_dir):
    """a statement about the METHOD, oracle against oracle in float64, not about the kernel: on g2 with k = 16 and the
    hyper-parameters of _als_oracle.E2E, after E2E['iters'] = 6 iterations

        the direct half-step (_als_oracle.train)      loss 5.533607131196431
        3 steps of CG per half-step (train_cg)        loss 5.538321534456880      (+8.52e-4 relatively)

    and both stop at iteration 7 under tol = 1e-2 and at iteration 26 under tol = 1e-4.  Asserted: CG's final loss lies within twice the
    measured margin, 1.704e-3, above the direct one (an inexact half-step cannot end below the exact one's loss by more than noise),
    and every iteration's loss falls."""
    m = _g2_model(golden_dir, solver='cg')
    up, uc, ip, ic = m._csr
    likes = (O.csr_rows(up, uc), O.csr_rows(ip, ic))
    hyper = dict(a=m.a, b=m.b, lu=m.lu, lv=m.lv)
    direct = O.train(m.fue, m.fie, *likes, max_iter=O.E2E['iters'], tol=0.0, **hyper)[2]
    cg = CG.train_cg(m.fue, m.fie, *likes, max_iter=O.E2E['iters'], tol=0.0, steps=3, **hyper)[2]
    print('K24 g2 float64 losses: direct %r, cg %r' % (direct, cg))
    assert len(cg) == len(direct) == O.E2E['iters']
    assert all(later < earlier for earlier, later in zip([np.exp(50)] + cg, cg)), cg
    margin = (cg[-1] - direct[-1]) / direct[-1]
    assert -1e-9 <= margin <= 2 * 8.52e-4, margin
    stop = len(CG.train_cg(m.fue, m.fie, *likes, max_iter=200, tol=1e-2, steps=3, **hyper)[2])
    assert 1 < stop < 200
