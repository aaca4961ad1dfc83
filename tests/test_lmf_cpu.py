"""K25 without a GPU: the oracle of tests/test_gpu_lmf.py against its own definitions (tests/_lmf_oracle.py), the symbols of
include/tkr.h, and what lmf.LMF checks and stores before any kernel runs."""
import ctypes
import os
import re

import numpy as np
import pytest

import _lmf_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _small(k=3, n_users=7, n_items=5, seed=3):
    rng = np.random.Generator(np.random.PCG64(seed))
    Xa = rng.standard_normal((n_users, k + 2)) * 0.7
    Ya = rng.standard_normal((n_items, k + 2)) * 0.7
    Xa[:, k + 1] = 1
    Ya[:, k] = 1
    user_likes = [rng.permutation(n_items)[:m] for m in (0, 1, 2, 3, 5, 1, 2)]
    item_likes = [np.asarray([u for u, l in enumerate(user_likes) if i in l], dtype=np.int64) for i in range(n_items)]
    return Xa, Ya, user_likes, item_likes


def test_gradient_is_the_derivative_of_the_dense_objective():
    """central finite differences of the oracle's own float64 loss, both sides; the fixed column has no gradient"""
    k, alpha, lam, eps = 3, 2.5, 0.6, 1e-6
    Xa, Ya, user_likes, item_likes = _small(k)
    R = O.dense_counts(user_likes, len(Ya))
    gx = O.gradient(Xa, Ya, user_likes, fixed=k + 1, alpha=alpha, lam=lam)
    gy = O.gradient(Ya, Xa, item_likes, fixed=k, alpha=alpha, lam=lam)
    assert not gx[:, k + 1].any() and not gy[:, k].any()
    for table, g, fixed, f in ((Xa, gx, k + 1, lambda t: O.loss(t, Ya, R, alpha=alpha, lam=lam)), (Ya, gy, k, lambda t: O.loss(Xa, t, R, alpha=alpha, lam=lam))):
        for r in range(table.shape[0]):
            for j in range(k + 2):
                if j == fixed:
                    continue
                hi, lo = table.copy(), table.copy()
                hi[r, j] += eps
                lo[r, j] -= eps
                fd = (f(hi) - f(lo)) / (2 * eps)
                assert abs(-fd - g[r, j]) <= 1e-6 * max(1.0, abs(g[r, j])), (r, j, fd, g[r, j])


def test_step_rows_is_adagrad_on_that_gradient():
    k, alpha, lam, lr = 3, 2.5, 0.6, 0.5
    Xa, Ya, user_likes, _ = _small(k)
    H = 1 + np.random.Generator(np.random.PCG64(1)).random(Xa.shape)
    g = O.gradient(Xa, Ya, user_likes, fixed=k + 1, alpha=alpha, lam=lam)
    D, _ = O.dense_rows(Xa, Ya)
    Xn, Hn, _ = O.step_rows(Xa, H, Ya, D, user_likes, fixed=k + 1, alpha=alpha, lam=lam, lr=lr)
    free = np.arange(k + 2) != k + 1
    np.testing.assert_allclose(Hn[:, free], (H + g * g)[:, free], rtol=1e-12)
    np.testing.assert_allclose(Xn[:, free], (Xa + lr * g / np.sqrt(H + g * g))[:, free], rtol=1e-12)
    np.testing.assert_array_equal(Xn[:, k + 1], Xa[:, k + 1])
    np.testing.assert_array_equal(Hn[:, k + 1], H[:, k + 1])


def test_logged_loss_is_the_dense_formula():
    """what train() logs for an iteration is `loss` at the new users and the old items, from the row terms and sp"""
    k, alpha, lam = 3, 2.5, 0.6
    Xa, Ya, user_likes, item_likes = _small(k)
    R = O.dense_counts(user_likes, len(Ya))
    X1, Y1, Hx, Hy, losses = O.train(Xa, Ya, user_likes, item_likes, alpha=alpha, lam=lam, lr=0.5, max_iter=1)
    assert abs(losses[0] - O.loss(X1, Ya, R, alpha=alpha, lam=lam)) <= 1e-10 * abs(losses[0])
    S = Xa @ Ya.T                                                 # ... and `loss` is the formula written out, pair by pair
    by_pair = sum((1 + alpha * R[u, i]) * np.logaddexp(0, S[u, i]) - alpha * R[u, i] * S[u, i] for u in range(len(Xa)) for i in range(len(Ya)))
    regs = 0.5 * lam * ((Xa[:, :k + 1] ** 2).sum() + (Ya[:, :k] ** 2).sum() + (Ya[:, k + 1] ** 2).sum())
    assert abs(O.loss(Xa, Ya, R, alpha=alpha, lam=lam) - (by_pair + regs)) <= 1e-10 * abs(by_pair)
    # the float32 restatement, in the kernels' order, stays close to the float64 one on the same inputs
    X32 = O.train(Xa, Ya, user_likes, item_likes, alpha=alpha, lam=lam, lr=0.5, max_iter=2, dtype=np.float32)[0]
    X64 = O.train(Xa.astype(np.float32), Ya.astype(np.float32), user_likes, item_likes, alpha=alpha, lam=lam, lr=0.5, max_iter=2)[0]
    assert np.abs(X32 - X64).max() <= 1e-5 * np.abs(X64).max()


def test_float32_oracle_cuts_slabs_and_heavy_rows_like_the_kernels():
    rng = np.random.Generator(np.random.PCG64(5))
    X = (rng.standard_normal((3, 5)) * 0.5).astype(np.float32)
    Y = (rng.standard_normal((70, 5)) * 0.5).astype(np.float32)
    D64, sp64 = O.dense_rows(X, Y)
    for slab in (16, 32, O.SLAB):
        D32, sp32 = O.dense_rows(X, Y, dtype=np.float32, slab=slab)
        assert D32.dtype == np.float32 and np.abs(D32 - D64).max() <= 1e-5 * np.abs(D64).max() and np.abs(sp32 - sp64).max() <= 1e-5 * sp64.max()
    Xs, H, Ys, rows, fixed = O.step_inputs(5, 'user')
    Ds, _ = O.dense_rows(Xs, Ys)
    hyper = dict(fixed=fixed, alpha=3.0, lam=0.6, lr=1.0)
    x64 = O.step_rows(Xs, H, Ys, Ds, rows, **hyper)[0]
    for heavy_from in (8, O.NO_HEAVY):
        x32 = O.step_rows(Xs, H, Ys, Ds, rows, dtype=np.float32, heavy_from=heavy_from, **hyper)[0]
        assert np.abs(x32 - x64).max() <= 1e-5 * np.abs(x64).max()
    assert max(len(r) for r in rows) > O.LIKE_SLAB and min(len(r) for r in rows) == 0


def test_library_declares_and_exports_the_lmf_entry_points():
    import tkr_hip
    header = open(os.path.join(ROOT, 'include', 'tkr.h')).read()
    declared = set(re.findall(r'^int(?:32_t|64_t)? (tkr_\w+)\(', header, flags=re.M))
    for name in ('tkr_lmf_dense_rows', 'tkr_lmf_step_rows', 'tkr_lmf_workspace_bytes'):
        assert name in declared and name in tkr_hip.EXPORTS + tkr_hip.EXPORTS_I64
    for macro, value in (('MAX_K', tkr_hip.LMF_MAX_K), ('SLAB', tkr_hip.LMF_SLAB), ('LIKE_SLAB', tkr_hip.LMF_LIKE_SLAB), ('HEAVY_WAVES', tkr_hip.LMF_HEAVY_WAVES)):
        assert re.search(r'#define TKR_LMF_%s %d\b' % (macro, value), header), macro
    assert (O.SLAB, O.LIKE_SLAB, O.HEAVY_WAVES) == (tkr_hip.LMF_SLAB, tkr_hip.LMF_LIKE_SLAB, tkr_hip.LMF_HEAVY_WAVES)
    if not os.path.exists(tkr_hip.LIB_PATH):
        return
    lib = ctypes.CDLL(tkr_hip.LIB_PATH)
    lib.tkr_lmf_workspace_bytes.restype = ctypes.c_int64
    size = lambda n_x, k, n_y: lib.tkr_lmf_workspace_bytes(ctypes.c_int64(n_x), ctypes.c_int32(k), ctypes.c_int64(n_y))
    assert size(10, 8, tkr_hip.LMF_SLAB) == 16 + 48 and size(10, 8, tkr_hip.LMF_SLAB + 1) >= 2 * 10 * (10 * 4 + 8) and size(33, 128, 9000) % 16 == 0
    assert size(10, 129, 5) == -2 and size(10, 0, 5) == -1 and size(0, 8, 5) == -1 and size(5, 8, 0) == -1
    # refused before any launch: no device is touched (this machine may have none)
    i64, i32, f64 = ctypes.c_int64, ctypes.c_int32, ctypes.c_double
    assert lib.tkr_lmf_dense_rows(None, i64(1), None, i64(1), i32(4), None, None, None, i64(0), None) == -1
    assert lib.tkr_lmf_step_rows(None, i32(1), i32(4), None, None, None, i64(0), i64(1), i32(0), f64(1), f64(0), f64(1), i64(1), None, None, None, None,
                                 i64(0), None, None) == -1


def test_lmf_argument_checks_need_no_gpu():
    import lmf
    with pytest.raises(ValueError, match='128'):
        lmf.LMF(k=129)
    with pytest.raises(ValueError):
        lmf.LMF(k=0)
    with pytest.raises(ValueError, match='lam'):
        lmf.LMF(lam=-0.1)
    with pytest.raises(ValueError, match='alpha'):
        lmf.LMF(alpha=0.0)
    with pytest.raises(ValueError, match='alpha'):
        lmf.LMF(alpha=float('inf'))
    with pytest.raises(ValueError, match='lr'):
        lmf.LMF(lr=0.0)
    with pytest.raises(ValueError, match='load_training_data'):
        lmf.LMF().train()
    with pytest.raises(ValueError, match='load_training_data'):
        lmf.LMF().fold_in([[1]])
    m = lmf.LMF()
    assert (m.k, m.lam, m.alpha, m.lr) == (30, 0.6, None, 1.0)


def _g2_model(golden_dir, **hyper):
    import lmf
    d = os.path.join(golden_dir, 'g2')
    m = lmf.LMF(**hyper)
    m.load_training_data(os.path.join(d, 'uid'), os.path.join(d, 'vid'), os.path.join(d, 'f0tr.txt'), seed=O.E2E['seed'])
    return m


def test_alpha_none_balances_the_classes_and_the_seed_fixes_the_start(golden_dir):
    m = _g2_model(golden_dir, k=O.E2E['k'])
    assert (m.n_users, m.n_items, m.n_likes) == (40, 30, 103)
    assert m.alpha is None and m.alpha_ == (40 * 30 - 103) / 103 == O.balance_alpha(40, 30, 103)
    assert _g2_model(golden_dir, k=4, alpha=10).alpha_ == 10.0
    Xa, Ya = m._tables()
    X0, Y0 = O.init(40, 30, O.E2E['k'], O.E2E['seed'])
    np.testing.assert_array_equal(Xa, X0)
    np.testing.assert_array_equal(Ya, Y0)
    assert not m.fib.any() and m.fib.shape == (30, 1) and (m.hu == 1).all() and (m.hi == 1).all()
    up, uc, ip, ic = m._csr
    assert sum(1 for x in O.csr_rows(up, uc) if len(x) == 0) == 3 and sum(1 for x in O.csr_rows(ip, ic) if len(x) == 0) == 4


def test_float64_loss_halves_on_g2(golden_dir):
    """the premise of the GPU test: 30 iterations at the end-to-end hyper-parameters take the loss below half its first value"""
    m = _g2_model(golden_dir, k=O.E2E['k'])
    up, uc, ip, ic = m._csr
    hyper = {name: O.E2E[name] for name in ('alpha', 'lam', 'lr')}
    losses = O.train(*m._tables(), O.csr_rows(up, uc), O.csr_rows(ip, ic), max_iter=30, **hyper)[4]
    print('K25 g2 float64 losses: first %.1f last %.1f' % (losses[0], losses[-1]))
    assert losses[-1] < 0.5 * losses[0]


def test_lmf_npz_round_trip(golden_dir, tmp_path):
    m = _g2_model(golden_dir, k=5, alpha=7.0, lam=0.3, lr=0.5)
    rng = np.random.Generator(np.random.PCG64(9))
    m.fub = rng.standard_normal(40).astype(np.float32)
    m.hu = (1 + rng.random((40, 7))).astype(np.float32)
    m.hi = (1 + rng.random((30, 7))).astype(np.float32)
    m.iters_done = 12
    m.export_model(str(tmp_path))
    assert os.listdir(str(tmp_path)) == ['lmf.npz']
    with np.load(str(tmp_path / 'lmf.npz')) as z:
        assert sorted(z.files) == ['alpha', 'fub', 'hi', 'hu', 'iters', 'lam', 'lr', 'seed']
        assert (float(z['alpha']), float(z['lam']), float(z['lr']), int(z['seed']), int(z['iters'])) == (7.0, 0.3, 0.5, 0, 12)
    fresh = _g2_model(golden_dir, k=5, alpha=7.0)
    fresh.import_model(str(tmp_path))
    for name in ('fub', 'hu', 'hi'):
        np.testing.assert_array_equal(getattr(fresh, name), getattr(m, name))
    assert fresh.iters_done == 12
    with pytest.raises(ValueError, match='shapes'):
        _g2_model(golden_dir, k=6).import_model(str(tmp_path))
    fresh.import_model(str(tmp_path / 'nowhere'))                 # no lmf.npz: a fresh start
