"""K21 (CER) without a GPU: the oracle of tests/_cer_oracle.py against the objective it is said to minimise, the premise of the GPU
end-to-end test, and everything of als.CER and the C ABI that is checked before a device is touched."""
import ctypes
import os
import re

import numpy as np
import pytest

import _cer_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _problem(seed=7, n_x=19, n_y=23, k=6):
    rng = np.random.Generator(np.random.PCG64(seed))
    Y, X0, P = rng.random((n_y, k)), rng.random((n_x, k)), rng.standard_normal((n_x, k))
    rows = [rng.permutation(n_y)[:m] for m in rng.integers(0, 6, n_x)]
    rows[3] = rows[11] = np.zeros(0, np.int64)                                   # cold rows, whatever the draw gave
    rated = sorted({int(c) for likes in rows for c in likes})
    return Y, X0, P, rows, rated


def test_item_half_step_zeroes_the_gradient_of_its_rows_objective():
    """row r minimises 1/2 x^T (G + w sum y y^T) x - a sum y.x + 1/2 ridge |x|^2 ... with the prior: the gradient
    (A + ridge I) x - a sum y - w_prior p vanishes, for warm rows and, with no likes, for cold ones; the row loss is the stated one"""
    Y, X0, P, rows, rated = _problem()
    a, b, ridge, w_prior = 1.0, 0.01, 0.7, 0.7
    X1, loss = O.half_step_prior(X0, Y, rows, rated, P, a=a, b=b, ridge_in_G=0.0, ridge=ridge, w_prior=w_prior)
    G = O.gram(Y, rated, b, 0.0)
    n_cold = 0
    for r, likes in enumerate(rows):
        y = Y[likes]
        A = G + (a - b) * (y.T @ y)
        grad = (A + ridge * np.eye(Y.shape[1])) @ X1[r] - a * y.sum(axis=0) - w_prior * P[r]
        assert np.abs(grad).max() <= 1e-12 * (1.0 + np.abs(P[r]).max())
        fit = 0.5 * X1[r] @ A @ X1[r] - a * (y @ X1[r]).sum() + 0.5 * a * len(likes) if len(likes) else 0.0      # cer.py:61-63
        assert abs(fit + 0.5 * w_prior * ((X1[r] - P[r]) ** 2).sum() - loss[r]) <= 1e-12 * max(1.0, abs(loss[r]))
        n_cold += len(likes) == 0
    assert n_cold >= 2
    # w_prior = 0 and a prior of zeros: the warm rows of K20's oracle, the cold rows zero
    X2, loss2 = O.half_step_prior(X0, Y, rows, rated, np.zeros_like(P), a=a, b=b, ridge_in_G=0.0, ridge=ridge, w_prior=0.0)
    X3, loss3 = O.half_step(X0, Y, rows, rated, a=a, b=b, ridge_in_G=0.0, ridge=ridge)
    warm = [r for r, likes in enumerate(rows) if len(likes)]
    np.testing.assert_array_equal(X2[warm], X3[warm])
    np.testing.assert_array_equal(loss2[warm], loss3[warm])
    assert not X2[[3, 11]].any() and not loss2[[3, 11]].any()


def test_e_step_zeroes_the_gradient_of_the_regression():
    """E minimises 1/2 lv |V - F E|^2 + 1/2 le |E|^2: lv F^T (F E - V) + le E = 0"""
    rng = np.random.Generator(np.random.PCG64(8))
    F, V = rng.random((30, 40)) * (rng.random((30, 40)) < 0.2), rng.standard_normal((30, 6))         # d > n: le alone keeps FF definite
    for lv, le in ((0.1, 1.0), (10.0, 1e4)):
        E = O.e_step(F, V, lv=lv, le=le)
        grad = lv * F.T @ (F @ E - V) + le * E
        assert np.abs(grad).max() <= 1e-11 * lv * np.abs(F.T @ V).max()


def _g2_model(golden_dir, **over):
    import als
    d = os.path.join(golden_dir, 'g2')
    hyper = dict(k=O.E2E['k'], d=O.E2E['d'], lu=O.E2E['lu'], lv=O.E2E['lv'], le=O.E2E['le'], a=O.E2E['a'], b=O.E2E['b'])
    hyper.update(over)
    m = als.CER(**hyper)
    m.load_training_data(os.path.join(d, 'uid'), os.path.join(d, 'vid'), os.path.join(d, 'f0tr.txt'), seed=O.E2E['seed'])
    return m


def test_float64_losses_fall_on_the_inputs_of_the_gpu_tests(golden_dir):
    """the premise of the GPU end-to-end test: the printed loss mixes the old Fe with the new E and is not monotone by construction; on
    g2 with E2E it does fall at every iteration in float64.  g2: 30 items, 26 with a training like, 4 cold"""
    m = _g2_model(golden_dir)
    assert (m.n_items, len(m.i_rated)) == (30, 26) and O.E2E['d'] == 24 < m.n_items
    F = O.e2e_features(m.n_items)
    assert F.dtype == np.float32 and F.shape == (30, 24) and 0.1 < (F != 0).mean() < 0.3
    U0, V0, E0 = O.e2e_start(m.n_users, m.n_items)
    np.testing.assert_array_equal(U0, m.fue)                                     # the start the model draws from the same seed
    np.testing.assert_array_equal(V0, m.fie)
    np.testing.assert_array_equal(E0, m._rng.standard_normal((m.d, m.k), dtype=np.float32))
    up, uc, ip, ic = m._csr
    likes = (O.csr_rows(up, uc), O.csr_rows(ip, ic))
    hyper = dict(a=m.a, b=m.b, lu=m.lu, lv=m.lv, le=m.le)
    U, V, E, losses = O.cer_train(U0, V0, E0, F, *likes, max_iter=O.E2E['iters'], tol=0.0, **hyper)
    assert len(losses) == O.E2E['iters']
    assert all(later < earlier for earlier, later in zip([np.exp(50)] + losses, losses)), losses
    cold = [j for j in range(m.n_items) if j not in m.i_rated]
    assert len(cold) == 4
    np.testing.assert_array_equal(V[cold], F[cold].astype(np.float64) @ E)      # cer.py:70-73
    stop = len(O.cer_train(U0, V0, E0, F, *likes, max_iter=200, tol=1e-2, **hyper)[3])
    assert 1 < stop < 200                                                        # ... and the stopping test has something to stop at


def test_cer_argument_checks_need_no_gpu(golden_dir, tmp_path):
    import als
    from utils import export_embed_to_file
    for bad in (dict(d=0), dict(d=2.5), dict(lv=0.0), dict(lv=-1.0), dict(le=0.0), dict(le=-3.0), dict(k=129), dict(a=0.01, b=0.01), dict(b=0.0)):
        with pytest.raises(ValueError):
            als.CER(**{**dict(k=4, d=3), **bad})
    m = als.CER(k=4, d=3)
    assert (m.k, m.d, m.lu, m.lv, m.le, m.a, m.b) == (4, 3, 0.01, 10.0, 10e3, 1.0, 0.01) and m.E is None
    with pytest.raises(ValueError, match='load_training_data'):
        m.train()
    with pytest.raises(ValueError, match='train'):
        m.embed_items(np.zeros((2, 3), np.float32))
    m = _g2_model(golden_dir)
    with pytest.raises(ValueError, match='load_content_data'):
        m.train()
    # a final-E.dat of another shape
    out = str(tmp_path / 'model')
    os.mkdir(out)
    export_embed_to_file(os.path.join(out, 'final-E.dat'), np.ones((O.E2E['d'] + 1, O.E2E['k']), np.float32))
    with pytest.raises(ValueError, match=r'\(d, k\)'):
        m.import_model(out)
    assert m.E is None
    good = np.arange(O.E2E['d'] * O.E2E['k'], dtype=np.float32).reshape(O.E2E['d'], O.E2E['k']) / 8
    export_embed_to_file(os.path.join(out, 'final-E.dat'), good)
    m.import_model(out)
    np.testing.assert_array_equal(m.E, good)
    feat = np.eye(O.E2E['d'], dtype=np.float32)[:5] * 2
    np.testing.assert_array_equal(m.embed_items(feat), 2 * good[:5])
    with pytest.raises(ValueError, match='feat'):
        m.embed_items(np.zeros((2, O.E2E['d'] + 1), np.float32))
    # the memory arithmetic: 8 (d^2 + n_items d) for the fp64 features and FF; U, V, Fe and E in fp32
    assert als.cer_train_bytes(7, 5, 3, 2) == (8 * (4 + 10), 4 * 3 * (7 + 10 + 2))
    dense, tables = als.cer_train_bytes(69878, 10677, 50, 20000)
    assert dense == 8 * (20000 ** 2 + 10677 * 20000) and tables == 4 * 50 * (69878 + 2 * 10677 + 20000)


def test_single_cer_still_raises():
    import single
    with pytest.raises(NotImplementedError):
        single.CER(k=4)


def test_train_als_takes_content_with_cer_only(tmp_path):
    import train_als
    for argv in (['--content', 'x.pkl'], ['--model', 'cer'], ['--model', 'cer', '--content', 'x.pkl'], ['--model', 'wmf', '--content', 'x.pkl', '--dim', '3']):
        with pytest.raises(SystemExit):
            train_als.main(argv + ['-d', str(tmp_path)])


def test_library_exports_the_prior_entry_points():
    import tkr_hip
    header = open(os.path.join(ROOT, 'include', 'tkr.h')).read()
    declared = set(re.findall(r'^int(?:32_t|64_t)? (tkr_\w+)\(', header, flags=re.M))
    assert 'tkr_als_solve_rows_prior' in declared and 'tkr_als_solve_rows_prior' in tkr_hip.EXPORTS
    assert 'tkr_als_prior_workspace_bytes' in declared and 'tkr_als_prior_workspace_bytes' in tkr_hip.EXPORTS_I64
    if not os.path.exists(tkr_hip.LIB_PATH):
        return
    lib = ctypes.CDLL(tkr_hip.LIB_PATH)
    size, k20 = lib.tkr_als_prior_workspace_bytes, lib.tkr_als_workspace_bytes
    size.restype = k20.restype = ctypes.c_int64
    size.argtypes = k20.argtypes = [ctypes.c_int64, ctypes.c_int32, ctypes.c_int64]
    assert size(10, 129, 0) == -1 and size(10, 0, 0) == -1 and size(-1, 8, 0) == -1
    for n_x, k, s in ((10, 8, 3), (0, 128, 0), (1000, 50, 7)):
        assert size(n_x, k, s) % 16 == 0 and size(n_x, k, s) - k20(n_x, k, s) >= k * k * 4      # room for one factor
    # refused before any launch: no device is touched (this machine may have none)
    solve = lib.tkr_als_solve_rows_prior
    solve.restype = ctypes.c_int
    solve.argtypes = [ctypes.c_void_p, ctypes.c_int32, ctypes.c_int32, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64, ctypes.c_int64,
                      ctypes.c_double, ctypes.c_double, ctypes.c_double, ctypes.c_int64, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                      ctypes.c_double, ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p, ctypes.c_void_p]
    assert solve(None, 5, 4, None, None, None, 0, 3, 0.99, 1.0, 0.1, 8, None, None, None, 1.0, None, 0, None, None) == -1
