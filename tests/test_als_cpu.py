"""K20 without a GPU: the float64 restatement (tests/_als_oracle.py) is what it claims to be -- each half-step the exact minimiser of
the dense objective, the row formula of the loss the dense objective itself, the loss falling on the inputs the GPU tests use -- and
the argument checks of als.WMF, which never need a device."""
import ctypes
import os
import re

import numpy as np
import pytest

import _als_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _problem(seed=5, n_users=23, n_items=17, k=6):
    rng = np.random.Generator(np.random.PCG64(seed))
    user_likes = [rng.integers(0, n_items, m) for m in rng.integers(0, 7, n_users)]      # repeats happen, empty rows too
    user_likes[3] = np.zeros(0, np.int64)
    item_likes = [[] for _ in range(n_items)]
    for u, likes in enumerate(user_likes):
        for i in likes:
            item_likes[int(i)].append(u)
    item_likes = [np.asarray(x, dtype=np.int64) for x in item_likes]
    U, V = rng.random((n_users, k)), rng.random((n_items, k))
    return U, V, user_likes, item_likes


def _gradients(U, V, R, u_rated, i_rated, a, b, lu, lv):
    """d loss_dense / dU, dV in the rated rows"""
    P = U[u_rated] @ V[i_rated].T
    Rr = R[np.ix_(u_rated, i_rated)]
    W = Rr * (a * (P - 1.0) - b * P) + b * P
    return W @ V[i_rated] + lu * U[u_rated], W.T @ U[u_rated] + lv * V[i_rated]


def test_half_step_zeroes_the_gradient_of_the_dense_objective():
    U, V, user_likes, item_likes = _problem()
    a, b, lu, lv = 1.0, 0.01, 0.03, 0.07
    u_rated = [u for u, l in enumerate(user_likes) if len(l)]
    i_rated = [i for i, l in enumerate(item_likes) if len(l)]
    R = O.dense_counts(user_likes, len(item_likes))
    U1, _ = O.half_step(U, V, user_likes, i_rated, a=a, b=b, ridge_in_G=lu, ridge=0.0)
    gU, _ = _gradients(U1, V, R, u_rated, i_rated, a, b, lu, lv)
    for row, u in zip(gU, u_rated):
        rhs = a * V[user_likes[u]].sum(axis=0)
        assert np.linalg.norm(row) <= 1e-9 * np.linalg.norm(rhs), u
    np.testing.assert_array_equal(U1[3], U[3])                                   # a row without likes is left as it is
    V1, _ = O.half_step(V, U1, item_likes, u_rated, a=a, b=b, ridge_in_G=0.0, ridge=lv)
    _, gV = _gradients(U1, V1, R, u_rated, i_rated, a, b, lu, lv)
    for row, i in zip(gV, i_rated):
        rhs = a * U1[item_likes[i]].sum(axis=0)
        assert np.linalg.norm(row) <= 1e-9 * np.linalg.norm(rhs), i


def test_row_formula_of_the_loss_is_the_dense_objective():
    U, V, user_likes, item_likes = _problem(seed=6)
    hyper = dict(a=1.0, b=0.01, lu=0.03, lv=0.07)
    u_rated = [u for u, l in enumerate(user_likes) if len(l)]
    i_rated = [i for i, l in enumerate(item_likes) if len(l)]
    R = O.dense_counts(user_likes, len(item_likes))
    for _ in range(3):
        U, V, loss = O.iteration(U, V, user_likes, item_likes, **hyper)
        dense = O.loss_dense(U, V, R, u_rated, i_rated, **hyper)
        assert abs(loss - dense) <= 1e-10 * abs(dense)


def _g2_model(golden_dir):
    import als
    d = os.path.join(golden_dir, 'g2')
    m = als.WMF(k=O.E2E['k'], lu=O.E2E['lu'], lv=O.E2E['lv'])
    m.load_training_data(os.path.join(d, 'uid'), os.path.join(d, 'vid'), os.path.join(d, 'f0tr.txt'), seed=O.E2E['seed'])
    return m


def test_float64_losses_fall_on_the_inputs_of_the_gpu_tests(golden_dir):
    """the premise of the GPU test of monotone losses: on its inputs the exact alternation does fall, at every iteration"""
    m = _g2_model(golden_dir)
    assert m.fue.dtype == np.float32 and m.fue.shape == (m.n_users, 16) and m.fie.shape == (m.n_items, 16)
    assert 0.0 <= m.fue.min() and m.fue.max() < 1.0 and m.n_ratings == m.n_users * m.n_items
    up, uc, ip, ic = m._csr
    assert m.u_rated == [u for u in range(m.n_users) if up[u + 1] > up[u]] and 0 < len(m.u_rated) < m.n_users
    assert m.i_rated == [i for i in range(m.n_items) if ip[i + 1] > ip[i]]
    _, _, losses = O.train(m.fue, m.fie, O.csr_rows(up, uc), O.csr_rows(ip, ic), a=m.a, b=m.b, lu=m.lu, lv=m.lv, max_iter=O.E2E['iters'], tol=0.0)
    assert len(losses) == O.E2E['iters']
    assert all(later < earlier for earlier, later in zip([np.exp(50)] + losses, losses)), losses
    m2 = _g2_model(golden_dir)                                                   # the seed fixes the start
    np.testing.assert_array_equal(m.fue, m2.fue)
    np.testing.assert_array_equal(m.fie, m2.fie)


def test_float64_losses_fall_on_the_solve_inputs():
    """... and a half-step on the inputs of the GPU solve test lowers the objective of its rows in float64 too (k = 5 .. 128)"""
    for k in (5, 50, 128):
        Y, X0, rows, rated = O.solve_inputs(k)
        X1, loss1 = O.half_step(X0, Y, rows, rated, a=O.SOLVE_A, b=O.SOLVE_B, ridge_in_G=0.0, ridge=0.01)
        G = O.gram(Y, rated, O.SOLVE_B, 0.0)
        for r, likes in enumerate(rows):
            if len(likes) == 0:
                np.testing.assert_array_equal(X1[r], X0[r].astype(np.float64))
                continue
            y = Y[likes].astype(np.float64)
            A = G + (O.SOLVE_A - O.SOLVE_B) * (y.T @ y)
            f = lambda x: 0.5 * x @ A @ x - O.SOLVE_A * (y @ x).sum() + 0.5 * O.SOLVE_A * len(likes) + 0.005 * x @ x
            assert f(X1[r]) <= f(X0[r].astype(np.float64))
            assert abs(f(X1[r]) - 0.005 * X1[r] @ X1[r] - loss1[r]) <= 1e-9 * max(1.0, abs(loss1[r]))


def test_wmf_argument_checks_need_no_gpu(golden_dir):
    import als
    with pytest.raises(ValueError, match='128'):
        als.WMF(k=129)
    with pytest.raises(ValueError):
        als.WMF(k=0)
    with pytest.raises(ValueError, match='exceed'):
        als.WMF(k=4, a=0.01, b=0.01)
    with pytest.raises(ValueError, match='exceed'):
        als.WMF(k=4, a=0.5, b=1.0)
    with pytest.raises(ValueError, match='positive'):
        als.WMF(k=4, b=0.0)
    with pytest.raises(ValueError, match='positive'):
        als.WMF(k=4, b=-1.0)
    with pytest.raises(ValueError, match='load_training_data'):
        als.WMF(k=4).train()
    m = als.WMF(k=128)
    assert (m.k, m.lu, m.lv, m.a, m.b) == (128, 0.01, 0.01, 1.0, 0.01) and m.fue is None and not hasattr(m, 'fib')
    m.export_model('nowhere')
    m.import_model('nowhere')


def test_single_wmf_still_raises():
    import single
    with pytest.raises(NotImplementedError, match='als.WMF'):
        single.WMF(k=4)
    for name in ('DPM', 'CER', 'ENCODER', 'MLP'):
        with pytest.raises(NotImplementedError):
            getattr(single, name)(k=4)


def test_library_exports_the_als_entry_points():
    import tkr_hip
    header = open(os.path.join(ROOT, 'include', 'tkr.h')).read()
    declared = set(re.findall(r'^int(?:32_t|64_t)? (tkr_\w+)\(', header, flags=re.M))
    for name in ('tkr_als_gram', 'tkr_als_solve_rows', 'tkr_als_workspace_bytes'):
        assert name in declared and name in tkr_hip.EXPORTS + tkr_hip.EXPORTS_I64
    assert re.search(r'#define TKR_ALS_MAX_K %d\b' % tkr_hip.ALS_MAX_K, header)
    assert re.search(r'#define TKR_ALS_GRAM_SLAB %d\b' % tkr_hip.ALS_GRAM_SLAB, header)
    if not os.path.exists(tkr_hip.LIB_PATH):
        return
    lib = ctypes.CDLL(tkr_hip.LIB_PATH)
    for name in ('tkr_als_gram', 'tkr_als_solve_rows', 'tkr_als_workspace_bytes'):
        assert hasattr(lib, name)
    lib.tkr_als_workspace_bytes.restype = ctypes.c_int64
    size = lambda n_x, k, s: lib.tkr_als_workspace_bytes(ctypes.c_int64(n_x), ctypes.c_int32(k), ctypes.c_int64(s))
    assert size(0, 8, 3) >= 3 * (64 + 8 + 1) * 4 and size(10, 8, 0) >= 40 and size(10, 8, 3) % 16 == 0
    assert size(10, 129, 0) == -1 and size(10, 0, 0) == -1 and size(-1, 8, 0) == -1
    # refused before any launch: no device is touched (this machine may have none)
    assert lib.tkr_als_gram(None, 1, 4, None, ctypes.c_int64(0), ctypes.c_double(1), ctypes.c_double(0), None, None, ctypes.c_int64(0), None, None) == -1
