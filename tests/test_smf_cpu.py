"""K27 without a GPU: the oracle of tests/test_gpu_smf.py against its own definitions (tests/_smf_oracle.py), the symbols of
include/tkr.h, and what smf.SMF checks and stores before any kernel runs."""
import ctypes
import os
import re

import numpy as np
import pytest

import _smf_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _toy(n_users=40, n_items=30, k=5, seed=27):
    """-> (Xa [n_users, k + 1], Ya [n_items, k + 1], user likes, item likes); one user and a few items without likes, one like twice"""
    rng = np.random.Generator(np.random.PCG64(seed))
    Xa = rng.standard_normal((n_users, k + 1)) * 0.7
    Ya = rng.standard_normal((n_items, k + 1)) * 0.7
    Xa[:, k] = 1
    user_likes = [rng.permutation(n_items - 3)[:rng.integers(1, 6)] for _ in range(n_users)]
    user_likes[3] = np.zeros(0, dtype=np.int64)
    user_likes[5] = np.concatenate([user_likes[5], user_likes[5][:1]])
    item_likes = [np.asarray([u for u, likes in enumerate(user_likes) for c in likes if c == i], dtype=np.int64) for i in range(n_items)]
    return Xa, Ya, user_likes, item_likes


def _gradients(Xa, Ya, user_likes, item_likes, lam):
    """the two gradients as the half-steps form them: the users' from lse as row offset, the items' from lse - log n as column offset"""
    k = Xa.shape[1] - 1
    lse = O.lse_rows(Xa, Ya)
    gx = O.gradient(Xa, Ya, user_likes, fixed=k, scale_by_likes=True, row_off=lse, lam=lam)
    gy = O.gradient(Ya, Xa, item_likes, fixed=-1, scale_by_likes=False, col_off=O.item_offsets(lse, O.counts(user_likes)), lam=lam)
    return gx, gy


@pytest.mark.parametrize('table,r,j', [('user', 7, 2), ('item', 11, 3), ('item', 4, 5)])
def test_minus_g_is_the_central_difference_of_f(table, r, j):
    """one user component, one item component and one item bias (column k = 5) on 40 x 30 with k = 5, to relative 1e-6"""
    lam, eps = 0.1, 1e-5
    Xa, Ya, user_likes, item_likes = _toy()
    g = _gradients(Xa, Ya, user_likes, item_likes, lam)[table == 'item'][r, j]
    hi, lo = [t.copy() for t in (Xa, Ya)], [t.copy() for t in (Xa, Ya)]
    hi[table == 'item'][r, j] += eps
    lo[table == 'item'][r, j] -= eps
    fd = (O.loss(*hi, user_likes, lam=lam) - O.loss(*lo, user_likes, lam=lam)) / (2 * eps)
    print('K27 %s[%d][%d]: -g %.9g, dF/eps %.9g' % (table, r, j, -g, fd))
    assert abs(g) > 1e-3 and abs(-g - fd) <= 1e-6 * abs(g)


def test_the_fixed_column_and_a_user_without_likes():
    Xa, Ya, user_likes, item_likes = _toy()
    gx, gy = _gradients(Xa, Ya, user_likes, item_likes, 0.1)
    assert not gx[:, 5].any() and gy[:, 5].any()
    np.testing.assert_allclose(gx[3], -0.1 * np.where(np.arange(6) == 5, 0, Xa[3]), rtol=1e-12)       # no likes: only the regulariser
    off = O.item_offsets(O.lse_rows(Xa, Ya), O.counts(user_likes))
    assert off[3] == np.inf and np.isfinite(np.delete(off, 3)).all()
    D = O.dense_rows(Ya, Xa, col_off=off)
    np.testing.assert_allclose(D, O.dense_rows(Ya, np.delete(Xa, 3, axis=0), col_off=np.delete(off, 3)), rtol=1e-12)


def test_first_loss_from_zero_tables_is_n_likes_log_n_items():
    _, _, user_likes, item_likes = _toy()
    Xa, Ya = np.zeros((40, 6)), np.zeros((30, 6))
    Xa[:, 5] = 1
    losses = O.train(Xa, Ya, user_likes, item_likes, lam=0.1, lr=0.3, max_iter=2)[4]
    n_likes = sum(len(x) for x in user_likes)
    assert abs(losses[0] - n_likes * np.log(30)) <= 1e-12 * losses[0] and losses[1] < losses[0]


def test_logged_loss_is_f_at_the_tables_entering_the_iteration():
    Xa, Ya, user_likes, item_likes = _toy()
    X1, Y1, _, _, losses = O.train(Xa, Ya, user_likes, item_likes, lam=0.1, lr=0.1, max_iter=2)
    X0, Y0 = O.train(Xa, Ya, user_likes, item_likes, lam=0.1, lr=0.1, max_iter=1)[:2]
    assert abs(losses[0] - O.loss(Xa, Ya, user_likes, lam=0.1)) <= 1e-12 * abs(losses[0])
    assert abs(losses[1] - O.loss(X0, Y0, user_likes, lam=0.1)) <= 1e-12 * abs(losses[1])


def test_step_rows_is_adagrad_on_that_gradient():
    lam, lr = 0.1, 0.5
    Xa, Ya, user_likes, item_likes = _toy()
    H = 1 + np.random.Generator(np.random.PCG64(1)).random(Xa.shape)
    gx = _gradients(Xa, Ya, user_likes, item_likes, lam)[0]
    Xn, Hn, part = O.half_step(Xa, H, Ya, user_likes, side='user', lam=lam, lr=lr)
    np.testing.assert_allclose(Hn[:, :5], (H + gx * gx)[:, :5], rtol=1e-12)
    np.testing.assert_allclose(Xn[:, :5], (Xa + lr * gx / np.sqrt(H + gx * gx))[:, :5], rtol=1e-12)
    np.testing.assert_array_equal(Xn[:, 5], Xa[:, 5])
    np.testing.assert_array_equal(Hn[:, 5], H[:, 5])


def test_float32_oracle_cuts_slabs_and_heavy_rows_like_the_kernels():
    rng = np.random.Generator(np.random.PCG64(5))
    X = (rng.standard_normal((3, 5)) * 0.5).astype(np.float32)
    Y = (rng.standard_normal((70, 5)) * 0.5).astype(np.float32)
    ro, co = rng.standard_normal(3).astype(np.float32), rng.standard_normal(70).astype(np.float32)
    lse64, D64 = O.lse_rows(X, Y), O.dense_rows(X, Y, ro, co)
    for slab in (32, 64, O.SLAB):
        lse32, D32 = O.lse_rows(X, Y, dtype=np.float32, slab=slab), O.dense_rows(X, Y, ro, co, dtype=np.float32, slab=slab)
        assert lse32.dtype == D32.dtype == np.float32
        assert np.abs(lse32 - lse64).max() <= 1e-6 * np.abs(lse64).max() and np.abs(D32 - D64).max() <= 1e-5 * np.abs(D64).max()
    big = O.lse_rows(X * 200, Y * 200, dtype=np.float32, slab=32)                # scores of magnitude 1e4
    assert np.isfinite(big).all() and np.abs(big - O.lse_rows(X * 200, Y * 200)).max() <= 1e-6 * np.abs(big).max()
    Xs, H, Ys, rows, Ds = O.step_inputs(5)
    hyper = dict(fixed=5, scale_by_likes=True, lam=0.1, lr=0.3)
    x64 = O.step_rows(Xs, H, Ys, Ds, rows, **hyper)[0]
    for heavy_from in (300, O.NO_HEAVY):
        x32 = O.step_rows(Xs, H, Ys, Ds, rows, dtype=np.float32, heavy_from=heavy_from, **hyper)[0]
        assert np.abs(x32 - x64).max() <= 1e-5 * np.abs(x64).max()
    assert max(len(r) for r in rows) == 700 and min(len(r) for r in rows) == 0


def test_library_declares_and_exports_the_smf_entry_points():
    """every name of the binding layer is declared and exported.  The header's rule for TKR_VERSION is that additions which change no
    existing entry point keep the number, and the tests of K9, K10 and K17 hold it at 120: K27 is such an addition"""
    import tkr_hip
    header = open(os.path.join(ROOT, 'include', 'tkr.h')).read()
    declared = set(re.findall(r'^int(?:32_t|64_t)? (tkr_\w+)\(', header, flags=re.M))
    for name in ('tkr_smf_lse_rows', 'tkr_smf_dense_rows', 'tkr_smf_step_rows', 'tkr_smf_workspace_bytes'):
        assert name in declared and name in tkr_hip.EXPORTS + tkr_hip.EXPORTS_I64
    for name in ('SMF_MAX_K', 'SMF_SLAB', 'SmfRefused', 'smf_workspace_bytes', 'smf_lse_rows', 'smf_dense_rows', 'smf_step_rows'):
        assert hasattr(tkr_hip, name), name
    assert issubclass(tkr_hip.SmfRefused, tkr_hip.AlsRefused)
    for macro, value in (('MAX_K', tkr_hip.SMF_MAX_K), ('SLAB', tkr_hip.SMF_SLAB)):
        assert re.search(r'#define TKR_SMF_%s %d\b' % (macro, value), header), macro
    assert (O.SLAB, O.LIKE_SLAB, O.HEAVY_WAVES) == (tkr_hip.SMF_SLAB, tkr_hip.LMF_LIKE_SLAB, tkr_hip.LMF_HEAVY_WAVES)
    assert int(re.search(r'#define TKR_VERSION (\d+)\b', header).group(1)) == tkr_hip.VERSION
    if not os.path.exists(tkr_hip.LIB_PATH):
        return
    lib = ctypes.CDLL(tkr_hip.LIB_PATH)
    assert lib.tkr_version() == tkr_hip.VERSION
    lib.tkr_smf_workspace_bytes.restype = ctypes.c_int64
    size = lambda n_x, k, n_y: lib.tkr_smf_workspace_bytes(ctypes.c_int64(n_x), ctypes.c_int32(k), ctypes.c_int64(n_y))
    assert size(10, 8, tkr_hip.SMF_SLAB) == 16 + 48 and size(10, 8, tkr_hip.SMF_SLAB + 1) >= 2 * 10 * 9 * 4 and size(33, 128, 9000) % 16 == 0
    assert size(10, 129, 5) == -2 and size(10, 0, 5) == -1 and size(0, 8, 5) == -1 and size(5, 8, 0) == -1
    # refused before any launch: no device is touched (this machine may have none)
    i64, i32, f64 = ctypes.c_int64, ctypes.c_int32, ctypes.c_double
    assert lib.tkr_smf_lse_rows(None, i64(1), None, i64(1), i32(4), None, None, i64(0), None) == -1
    assert lib.tkr_smf_dense_rows(None, i64(1), None, i64(1), i32(4), None, None, None, None, i64(0), None) == -1
    assert lib.tkr_smf_step_rows(None, i32(1), i32(4), None, None, None, i64(0), i64(1), i32(0), i32(0), f64(0), f64(1), i64(1), None, None, None,
                                 None, i64(0), None, None) == -1


def test_smf_argument_checks_need_no_gpu():
    import smf
    with pytest.raises(ValueError, match='128'):
        smf.SMF(k=129)
    with pytest.raises(ValueError):
        smf.SMF(k=0)
    with pytest.raises(ValueError, match='lam'):
        smf.SMF(lam=-0.1)
    with pytest.raises(ValueError, match='lr'):
        smf.SMF(lr=float('inf'))
    with pytest.raises(ValueError, match='lr'):
        smf.SMF(lr=float('nan'))
    with pytest.raises(ValueError, match='load_training_data'):
        smf.SMF().train()
    with pytest.raises(ValueError, match='load_training_data'):
        smf.SMF().fold_in([[1]])
    m = smf.SMF()
    assert (m.k, m.lam, m.lr) == (30, 0.01, 0.1)


def _g2_model(golden_dir, **hyper):
    import smf
    d = os.path.join(golden_dir, 'g2')
    m = smf.SMF(**hyper)
    m.load_training_data(os.path.join(d, 'uid'), os.path.join(d, 'vid'), os.path.join(d, 'f0tr.txt'), seed=O.E2E['seed'])
    return m


def test_the_seed_fixes_the_start(golden_dir):
    m = _g2_model(golden_dir, k=O.E2E['k'])
    assert (m.n_users, m.n_items, m.n_likes) == (40, 30, 103)
    Xa, Ya = m._tables()
    X0, Y0 = O.init(40, 30, O.E2E['k'], O.E2E['seed'])
    np.testing.assert_array_equal(Xa, X0)
    np.testing.assert_array_equal(Ya, Y0)
    assert not m.fib.any() and m.fib.shape == (30, 1) and (m.hu == 1).all() and (m.hi == 1).all() and m.hu.shape == (40, O.E2E['k'] + 1)


def test_float64_loss_falls_monotonically_on_g2_at_the_defaults(golden_dir):
    """the rule the defaults were chosen by; and the first loss is n_likes log n_items to 5 digits"""
    import smf
    m = _g2_model(golden_dir)
    assert (m.lam, m.lr) == (smf.SMF().lam, smf.SMF().lr)
    up, uc, ip, ic = m._csr
    losses = O.train(*m._tables(), O.csr_rows(up, uc), O.csr_rows(ip, ic), lam=m.lam, lr=m.lr, max_iter=30)[4]
    print('K27 g2 float64 losses: first %.3f last %.3f' % (losses[0], losses[-1]))
    assert all(b < a for a, b in zip(losses, losses[1:])) and losses[-1] < 0.5 * losses[0]
    assert abs(losses[0] - 103 * np.log(30)) <= 1e-4 * losses[0]


def test_embeddings_round_trip_on_the_host(golden_dir, tmp_path):
    """export_embeddings -> import_embeddings -> _tables(); smf.npz holds both slots, lam, lr, seed, iterations"""
    m = _g2_model(golden_dir, k=5, lam=0.3, lr=0.5)
    rng = np.random.Generator(np.random.PCG64(9))
    m.fue = (rng.integers(-250, 250, (40, 5)) / 64).astype(np.float32)      # values the '%f ' text holds exactly
    m.fie = (rng.integers(-250, 250, (30, 5)) / 64).astype(np.float32)
    m.fib = (rng.integers(-250, 250, (30, 1)) / 64).astype(np.float32)
    m.hu = (1 + rng.random((40, 6))).astype(np.float32)
    m.hi = (1 + rng.random((30, 6))).astype(np.float32)
    m.iters_done = 12
    out = str(tmp_path / 'smf')
    m.export_embeddings(out)
    assert sorted(os.listdir(out)) == ['final-B.dat', 'final-U.dat', 'final-V.dat', 'smf.npz']
    with np.load(os.path.join(out, 'smf.npz')) as z:
        assert sorted(z.files) == ['hi', 'hu', 'iters', 'lam', 'lr', 'seed']
        assert (float(z['lam']), float(z['lr']), int(z['seed']), int(z['iters'])) == (0.3, 0.5, 0, 12)
    fresh = _g2_model(golden_dir, k=5)
    fresh.import_embeddings(out)
    for a, b in zip(fresh._tables(), m._tables()):
        np.testing.assert_array_equal(a, b)
    for name in ('hu', 'hi'):
        np.testing.assert_array_equal(getattr(fresh, name), getattr(m, name))
    assert fresh.iters_done == 12 and (fresh._tables()[0][:, 5] == 1).all()
    with pytest.raises(ValueError, match='shapes'):
        _g2_model(golden_dir, k=6).import_model(out)
    fresh.import_model(str(tmp_path / 'nowhere'))                 # no smf.npz: a fresh start
