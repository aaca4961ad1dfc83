"""K25 on the GPU (csrc/lmf.hip, top-k-rec_amd/lmf.py) against tests/_lmf_oracle.py.

The yardstick is the project's own (tests/test_gpu_als.py): with x64 the float64 oracle on the same fp32 inputs and x32 the float32 one
in the kernels' order, e32 = max|x32 - x64| / max|x64| per case, and the kernel has to stay within F * max(e32, 2^-23); F = 16 is a
condition of the design, not a knob.  Every ratio is printed; DESIGN.md section 4 K25 keeps the worst.

The exact tests need no yardstick.  A remark on the saturated one: sigma(-64) is 1.6e-28 in fp32, not 0 (the kernel's sigma is +0 only
from s = -110 down), so a term that is "not selected" enters its chain as 1.6e-28 * y.  It changes no bit of a sum that holds one
selected row (|y| >= 1/8: 28 decimal orders above it), and the tables below give every row of X a selected row of Y and sums that
cannot cancel to zero: column 0 of the selected rows has one sign, the other columns are positive."""
import ctypes as C
import functools
import os

import numpy as np
import pytest
import torch

import _lmf_oracle as O

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = 16.0
FLOOR = 2.0 ** -23
SLAB = O.SLAB
KS = (3, 5, 32, 33, 64, 65, 128, 130)                            # widths of the tables, K = k + 2
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
    print('K25 %s: err %.3g e32 %.3g ratio %.3g' % (what, err, e32, ratio))
    assert ratio <= F, (what, err, e32)
    return ratio


# ---- 1. the dense kernel, exact -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('K', KS)
def test_dense_is_exact_where_sigma_is_one_half(K):
    """X = 0: every sigma is 0.5 exactly; Y multiples of 1/8: D = 0.5 * the column sums, bit for bit, in every row"""
    import tkr_hip
    rng = np.random.Generator(np.random.PCG64([1, K]))
    for n_y in (1, 31, 32, 33, 100, SLAB - 1, SLAB, SLAB + 1, 2 * SLAB + 5):
        Y = (rng.integers(-3, 4, (n_y, K)) / 8).astype(np.float32)
        want = (0.5 * Y.astype(np.float64).sum(axis=0)).astype(np.float32)
        Yd = _dev(Y)
        for n_x in (1, 31, 32, 33, 70):
            D, sp = tkr_hip.lmf_dense_rows(torch.zeros((n_x, K), dtype=torch.float32, device='cuda'), Yd, want_loss=True)
            D, sp = D.cpu().numpy(), sp.cpu().numpy()
            np.testing.assert_array_equal(D, np.broadcast_to(want, (n_x, K)), err_msg='n_x = %d, n_y = %d' % (n_x, n_y))
            assert np.abs(sp - n_y * np.log(2.0)).max() <= 1e-6 * n_y, (n_x, n_y)


def _saturated(rng, K, n_x, n_y, size):
    """-> (X, Y, selected [n_x, n_y] bool): every score is +size or -size exactly.  Column 0 of Y is a sign and the only column a row
    of X is not zero in; the others are positive"""
    Y = (rng.integers(1, 4, (n_y, K)) / 8).astype(np.float32)
    sign = rng.integers(0, 2, n_y) * 2 - 1
    sign[:2] = (1, -1)
    Y[:, 0] = sign
    X = np.zeros((n_x, K), dtype=np.float32)
    way = rng.integers(0, 2, n_x) * 2 - 1
    X[:, 0] = way * size
    return X, Y, sign[None, :] * way[:, None] > 0


@pytest.mark.parametrize('size', [64.0, 1e4])
@pytest.mark.parametrize('K', KS)
def test_dense_is_exact_where_sigma_is_saturated(K, size):
    """scores of +-64: sigma is 1 or too small to change a bit (the module's remark), D the exact sum of the selected rows and sp the
    exact sum of the positive scores; scores of +-1e4: sigma is exactly 1 or 0, D and sp are finite and the same sums"""
    import tkr_hip
    rng = np.random.Generator(np.random.PCG64([2, K]))
    for n_x, n_y in ((33, 100), (70, SLAB + 1), (5, 2 * SLAB + 5)):
        X, Y, selected = _saturated(rng, K, n_x, n_y, size)
        S = X.astype(np.float64) @ Y.astype(np.float64).T
        assert (np.abs(S) == size).all() and ((S > 0) == selected).all() and selected.any(axis=1).all()
        D, sp = tkr_hip.lmf_dense_rows(_dev(X), _dev(Y), want_loss=True)
        D, sp = D.cpu().numpy(), sp.cpu().numpy()
        assert np.isfinite(D).all() and np.isfinite(sp).all()
        np.testing.assert_array_equal(D, (selected.astype(np.float64) @ Y.astype(np.float64)).astype(np.float32), err_msg='%d x %d' % (n_x, n_y))
        np.testing.assert_array_equal(sp, size * selected.sum(axis=1))


# ---- 2. the dense kernel, generic -------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _generic(K, n_x, n_y):
    rng = np.random.Generator(np.random.PCG64([3, K, n_y]))
    X = (rng.standard_normal((n_x, K)) * 0.5).astype(np.float32)
    Y = (rng.standard_normal((n_y, K)) * 0.5).astype(np.float32)
    out = (X, Y, O.dense_rows(X, Y), O.dense_rows(X, Y, dtype=np.float32))
    for a in (X, Y) + out[2] + out[3]:
        a.flags.writeable = False
    return out


@pytest.mark.parametrize('n_y', [100, SLAB + 33])
@pytest.mark.parametrize('K', KS)
def test_dense_against_the_oracle(K, n_y):
    import tkr_hip
    X, Y, (D64, sp64), (D32, sp32) = _generic(K, 70, n_y)
    D, sp = tkr_hip.lmf_dense_rows(_dev(X), _dev(Y), want_loss=True)
    _held('dense D K=%d n_y=%d' % (K, n_y), D.cpu().numpy(), D64, D32)
    _held('dense sp K=%d n_y=%d' % (K, n_y), sp.cpu().numpy(), sp64, sp32)
    alone = tkr_hip.lmf_dense_rows(_dev(X), _dev(Y))              # without sp: the same D
    np.testing.assert_array_equal(_bits(alone.cpu().numpy()), _bits(D.cpu().numpy()))


# ---- 3. repeatability ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('K', [5, 33, 130])
def test_dense_bits_are_a_function_of_the_row(K):
    import tkr_hip
    X, Y = _generic(K, 70, SLAB + 33)[:2]
    Xd, Yd = _dev(X), _dev(Y)
    D, sp = (t.cpu().numpy() for t in tkr_hip.lmf_dense_rows(Xd, Yd, want_loss=True))
    D2, sp2 = (t.cpu().numpy() for t in tkr_hip.lmf_dense_rows(Xd, Yd, want_loss=True))
    np.testing.assert_array_equal(_bits(D), _bits(D2))
    np.testing.assert_array_equal(_bits(sp), _bits(sp2))
    for r in (0, 31, 32, 69):
        d1, s1 = (t.cpu().numpy() for t in tkr_hip.lmf_dense_rows(_dev(X[r:r + 1]), Yd, want_loss=True))
        np.testing.assert_array_equal(_bits(d1[0]), _bits(D[r]), err_msg='row %d alone' % r)
        np.testing.assert_array_equal(_bits(s1), _bits(sp[r:r + 1]))


# ---- 4. the step kernel ----------------------------------------------------------------------------------------------------------------
STEP = dict(alpha=3.0, lam=0.6, lr=1.0)


@functools.lru_cache(maxsize=None)
def _step_case(k, side):
    X, H, Y, rows, fixed = O.step_inputs(k, side)
    D = O.dense_rows(X, Y)[0].astype(np.float32)
    ref64 = O.step_rows(X, H, Y, D, rows, fixed=fixed, **STEP)
    return X, H, Y, rows, fixed, D, ref64


@pytest.mark.parametrize('heavy_from', [8, NO_HEAVY])
@pytest.mark.parametrize('k', [1, 5, 30, 64, 128])
def test_step_rows_against_the_oracle(k, heavy_from):
    import tkr_hip
    for side in ('user', 'item'):
        X0, H0, Y, rows, fixed, D, (x64, h64, l64) = _step_case(k, side)
        assert fixed == (k + 1 if side == 'user' else k) and {0, 1} <= {len(r) for r in rows} and max(len(r) for r in rows) > O.LIKE_SLAB
        x32, h32, l32 = O.step_rows(X0, H0, Y, D, rows, fixed=fixed, dtype=np.float32, heavy_from=heavy_from, **STEP)
        ptr, cols = O.to_csr(rows)
        X, H = _dev(X0), _dev(H0)
        loss = tkr_hip.lmf_step_rows(_dev(Y), _dev(D), _dev(ptr), _dev(cols), X, H, fixed=fixed, heavy_from=heavy_from, want_loss=True, **STEP)
        X, H, loss = X.cpu().numpy(), H.cpu().numpy(), loss.cpu().numpy()
        tag = 'k=%d %s heavy_from=%s' % (k, side, 'none' if heavy_from == NO_HEAVY else heavy_from)
        _held('step x ' + tag, X, x64, x32)
        _held('step h ' + tag, H, h64, h32)
        _held('step row loss ' + tag, loss, l64, l32)
        np.testing.assert_array_equal(_bits(X[:, fixed]), _bits(X0[:, fixed]))
        np.testing.assert_array_equal(_bits(H[:, fixed]), _bits(H0[:, fixed]))
        assert (X[:, np.arange(k + 2) != fixed] != X0[:, np.arange(k + 2) != fixed]).any(axis=1).all()      # a row without likes steps too


# ---- 5. refusals -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('heavy_from', [8, NO_HEAVY])
def test_like_columns_outside_the_table_are_skipped(heavy_from):
    import tkr_hip
    k = 33
    X0, H0, Y, rows, fixed, D, _ = _step_case(k, 'user')
    n_y = len(Y)
    dirty = [np.asarray(x, dtype=np.int64) for x in rows]
    dirty[4] = np.concatenate([dirty[4][:3], [-1], dirty[4][3:], [n_y]])       # 8 likes and two refused
    dirty[2] = np.concatenate([[n_y], dirty[2]])
    dirty[9] = np.concatenate([dirty[9][:270], [-1, -1], dirty[9][270:]])      # in the second slab of a heavy row
    dirty[11] = np.asarray([-1, n_y])                                           # nothing left: as a row without likes
    ptr, cols = O.to_csr(dirty)
    X, H = _dev(X0), _dev(H0)
    loss, status = tkr_hip.lmf_step_rows(_dev(Y), _dev(D), _dev(ptr), _dev(cols), X, H, fixed=fixed, heavy_from=heavy_from, want_loss=True,
                                         check=False, **STEP)
    assert int(status.item()) == 4 * 2 + 1
    x64, h64, l64 = O.step_rows(X0, H0, Y, D, rows, fixed=fixed, **STEP)
    x32, h32, l32 = O.step_rows(X0, H0, Y, D, rows, fixed=fixed, dtype=np.float32, heavy_from=heavy_from, **STEP)
    _held('step x with refused columns', X.cpu().numpy(), x64, x32)
    _held('step row loss with refused columns', loss.cpu().numpy(), l64, l32)
    with pytest.raises(tkr_hip.LmfRefused) as info:
        tkr_hip.lmf_step_rows(_dev(Y), _dev(D), _dev(ptr), _dev(cols), _dev(X0), _dev(H0), fixed=fixed, heavy_from=heavy_from, **STEP)
    assert (info.value.row, info.value.kind) == (2, 1)


@pytest.mark.parametrize('heavy_from', [8, NO_HEAVY])
def test_descending_like_ptr_leaves_the_row(heavy_from):
    import tkr_hip
    k = 16
    X0, H0, Y, rows, fixed, D, _ = _step_case(k, 'item')
    ptr, cols = O.to_csr(rows)
    good = ptr.copy()
    ptr[6] = ptr[5] - 1                                                         # row 5 descends; row 6 is a row again, longer by what row 5 had
    Yd, Dd = _dev(Y), _dev(D)
    X, H = _dev(X0), _dev(H0)
    loss, status = tkr_hip.lmf_step_rows(Yd, Dd, _dev(ptr), _dev(cols), X, H, fixed=fixed, heavy_from=heavy_from, want_loss=True, check=False, **STEP)
    assert int(status.item()) == 4 * 5 + 3
    X, H = X.cpu().numpy(), H.cpu().numpy()
    np.testing.assert_array_equal(_bits(X[5]), _bits(X0[5]))
    np.testing.assert_array_equal(_bits(H[5]), _bits(H0[5]))
    assert loss[5].item() == 0.0 and np.isfinite(X).all()
    assert all((X[r] != X0[r]).any() for r in range(len(rows)) if r != 5)
    for at, value, word in ((1, 3, 4 * 1 + 3), (len(good) - 1, len(cols) + 1, 4 * (len(rows) - 1) + 3)):      # row 1 ends past row 2's end; past the end
        bad_ptr = good.copy()
        bad_ptr[at] = value
        _, status = tkr_hip.lmf_step_rows(Yd, Dd, _dev(bad_ptr), _dev(cols), _dev(X0), _dev(H0), fixed=fixed, heavy_from=heavy_from, check=False, **STEP)
        assert int(status.item()) == word
    bad_ptr = good.copy()
    bad_ptr[0] = 1                                                              # does not start at 0
    with pytest.raises(tkr_hip.LmfRefused) as info:
        tkr_hip.lmf_step_rows(Yd, Dd, _dev(bad_ptr), _dev(cols), _dev(X0), _dev(H0), fixed=fixed, heavy_from=heavy_from, **STEP)
    assert (info.value.row, info.value.kind) == (0, 3)


def _raw():
    lib = C.CDLL(os.path.join(ROOT, 'top-k-rec_amd', 'libtkr_hip.so'))
    dense, step, size = lib.tkr_lmf_dense_rows, lib.tkr_lmf_step_rows, lib.tkr_lmf_workspace_bytes
    dense.restype = step.restype = C.c_int
    size.restype = C.c_int64
    size.argtypes = [C.c_int64, C.c_int32, C.c_int64]
    dense.argtypes = [C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p]
    step.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_int32, C.c_double, C.c_double,
                     C.c_double, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p]
    return dense, step, size


def test_raw_abi_through_ctypes():
    """the symbols as a maintainer of the reference would bind them: no helper module in between; and the argument
    checks: k = 129 is TKR_E_UNSUPPORTED, nothing is launched and nothing written"""
    dense, step, size = _raw()
    k = 12
    X0, H0, Y, rows, fixed, _, _ = _step_case(k, 'user')
    n_x, n_y = len(X0), len(Y)
    ptr, cols = O.to_csr(rows)
    Xd, Hd, Yd, pd, cd = _dev(X0), _dev(H0), _dev(Y), _dev(ptr), _dev(cols)
    D = torch.zeros((n_x, k + 2), dtype=torch.float32, device='cuda')
    sp = torch.zeros(n_x, dtype=torch.float64, device='cuda')
    loss = torch.zeros(n_x, dtype=torch.float64, device='cuda')
    status = torch.empty(1, dtype=torch.int64, device='cuda')
    ws = torch.empty(size(n_x, k, n_y) // 8, dtype=torch.int64, device='cuda')
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    p = lambda t: C.c_void_p(t.data_ptr())
    d_args = [p(Xd), n_x, p(Yd), n_y, k, p(D), p(sp), p(ws), ws.numel() * 8, stream]
    assert dense(*d_args) == 0
    D64, sp64 = O.dense_rows(X0, Y)
    D32, sp32 = O.dense_rows(X0, Y, dtype=np.float32)
    _held('raw dense D', D.cpu().numpy(), D64, D32)
    _held('raw dense sp', sp.cpu().numpy(), sp64, sp32)
    s_args = [p(Yd), n_y, k, p(D), p(pd), p(cd), len(cols), n_x, fixed, STEP['alpha'], STEP['lam'], STEP['lr'], 8, p(Xd), p(Hd), p(loss), p(ws),
              ws.numel() * 8, p(status), stream]
    Dh = D.cpu().numpy()
    assert step(*s_args) == 0
    assert int(status.item()) == -1
    x64, h64, l64 = O.step_rows(X0, H0, Y, Dh, rows, fixed=fixed, **STEP)
    x32, h32, l32 = O.step_rows(X0, H0, Y, Dh, rows, fixed=fixed, dtype=np.float32, heavy_from=8, **STEP)
    _held('raw step x', Xd.cpu().numpy(), x64, x32)
    _held('raw step row loss', loss.cpu().numpy(), l64, l32)
    before = [t.clone() for t in (Xd, Hd, D, sp, loss)]
    for at, bad, rc in ((0, None, -1), (2, None, -1), (5, None, -1), (1, 0, -1), (3, 0, -1), (4, 0, -1), (4, 129, -2), (8, -1, -1)):
        args = list(d_args)
        args[at] = bad
        assert dense(*args) == rc, at
    for at, bad, rc in ((0, None, -1), (3, None, -1), (4, None, -1), (5, None, -1), (13, None, -1), (14, None, -1), (18, None, -1), (2, 0, -1),
                        (2, 129, -2), (6, -1, -1), (7, 0, -1), (1, 0, -1), (8, -1, -1), (8, k + 2, -1), (12, 0, -1), (10, -0.5, -1),
                        (9, float('nan'), -1), (11, float('inf'), -1), (16, None, -1), (17, 8, -1)):
        args = list(s_args)
        args[at] = bad
        assert step(*args) == rc, at
    assert size(n_x, 129, n_y) == -2 and size(n_x, 0, n_y) == -1
    torch.cuda.synchronize()
    for was, now in zip(before, (Xd, Hd, D, sp, loss)):
        assert torch.equal(was, now)


# ---- 6. lmf.LMF end to end -------------------------------------------------------------------------------------------------------------
def _g2(golden_dir):
    return os.path.join(golden_dir, 'g2')


def _model(golden_dir):
    import lmf
    d = _g2(golden_dir)
    m = lmf.LMF(k=O.E2E['k'], lam=O.E2E['lam'], alpha=O.E2E['alpha'], lr=O.E2E['lr'])
    m.load_training_data(os.path.join(d, 'uid'), os.path.join(d, 'vid'), os.path.join(d, 'f0tr.txt'), seed=O.E2E['seed'])
    return m


@functools.lru_cache(maxsize=None)
def _trained(golden_dir):
    m = _model(golden_dir)
    X0, Y0 = m._tables()
    up, uc, ip, ic = m._csr
    likes = (O.csr_rows(up, uc), O.csr_rows(ip, ic))
    hyper = dict(alpha=m.alpha_, lam=m.lam, lr=m.lr, max_iter=O.E2E['iters'])
    m.train(max_iter=O.E2E['iters'], verbose=False)
    return m, X0, Y0, likes, O.train(X0, Y0, *likes, **hyper), O.train(X0, Y0, *likes, dtype=np.float32, **hyper)


def test_lmf_trains_as_the_oracle(golden_dir):
    m, X0, Y0, likes, t64, t32 = _trained(golden_dir)
    k = m.k
    assert len(m.losses) == O.E2E['iters'] == m.iters_done and (len(likes[0]), len(likes[1])) == (40, 30)
    assert m.fue.dtype == np.float32 and m.fue.shape == (40, k) and m.fie.shape == (30, k) and m.fib.shape == (30, 1) and m.fub.shape == (40,)
    for name, got, at in (('fue', m.fue, lambda t: t[0][:, :k]), ('fie', m.fie, lambda t: t[1][:, :k]), ('user biases', m.fub, lambda t: t[0][:, k]),
                          ('item biases', m.fib[:, 0], lambda t: t[1][:, k + 1]), ('user slots', m.hu, lambda t: t[2]), ('item slots', m.hi, lambda t: t[3]),
                          ('last loss', np.asarray(m.losses[-1:]), lambda t: np.asarray(t[4][-1:]))):
        _held('LMF %s after %d iterations' % (name, O.E2E['iters']), got, at(t64), at(t32))
    assert sum(1 for x in likes[0] if len(x) == 0) == 3 and sum(1 for x in likes[1] if len(x) == 0) == 4
    no_u = [u for u, x in enumerate(likes[0]) if len(x) == 0]
    assert (m.fue[no_u] != X0[no_u, :k]).any(axis=1).all()                        # a user without likes has a gradient


def test_lmf_loss_halves_in_thirty_iterations(golden_dir):
    m = _model(golden_dir)
    m.train(max_iter=30, verbose=False)
    print('K25 LMF on g2: loss %.1f -> %.1f' % (m.losses[0], m.losses[-1]))
    assert len(m.losses) == 30 and np.isfinite(m.losses).all() and m.losses[-1] < 0.5 * m.losses[0]
    stopped = _model(golden_dir)
    stopped.train(max_iter=30, tol=0.1, verbose=False)                          # the relative-change test of WMF
    assert 1 < len(stopped.losses) < 30 and stopped.losses == m.losses[:len(stopped.losses)]


# ---- 7. the model directory -----------------------------------------------------------------------------------------------------------
def test_lmf_model_directory_serves_evaluate_and_a_second_train(golden_dir, tmp_path):
    import evaluate as E
    from oracle import ref_np as R
    m = _trained(golden_dir)[0]
    out = str(tmp_path / 'lmf')
    m.export_embeddings(out)
    assert sorted(os.listdir(out)) == ['final-B.dat', 'final-U.dat', 'final-V.dat', 'lmf.npz']
    got = E.main(['-d', _g2(golden_dir), '-m', out, '-sl', 'im'])
    exp = R.evaluate_cli(_g2(golden_dir), out, scenarios=('im',))
    assert len(got) == len(exp) == 1 and got[0].startswith('im,')
    for g, e in zip(got, exp):
        assert g.split(',')[0] == e.split(',')[0]
        assert [float(x) for x in g.split(',')[1:]] == [float(x) for x in e.split(',')[1:]]
    fresh = _model(golden_dir)
    fresh.train(max_iter=0, model_path=out, verbose=False)                      # loads, runs no iteration
    np.testing.assert_array_equal(_bits(fresh.hu), _bits(m.hu))
    np.testing.assert_array_equal(_bits(fresh.hi), _bits(m.hi))
    np.testing.assert_array_equal(_bits(fresh.fub), _bits(m.fub))
    assert fresh.iters_done == m.iters_done and (fresh.hu != 1).any()
    np.testing.assert_allclose(fresh.fue, m.fue, atol=1e-6)                     # the '%f ' text of the factors
    np.testing.assert_allclose(fresh.fib, m.fib, atol=1e-6)
    fresh.train(max_iter=1, verbose=False)
    assert fresh.iters_done == m.iters_done + 1 and (fresh.hu >= m.hu).all() and (fresh.hu[:, :m.k + 1] > m.hu[:, :m.k + 1]).any()


# ---- 8. fold-in -----------------------------------------------------------------------------------------------------------------------
def test_lmf_fold_in_is_five_user_half_steps_from_zero(golden_dir):
    m, X0, Y0, likes = _trained(golden_dir)[:4]
    k = m.k
    users = [u for u, x in enumerate(likes[0]) if len(x)][:3]
    hist = [likes[0][u] for u in users]
    rows, biases = m.fold_in(hist, steps=5)
    assert rows.shape == (3, k) and rows.dtype == np.float32 and biases.shape == (3,) and biases.dtype == np.float32
    Ya = m._tables()[1]
    ref = {}
    for dtype in (np.float64, np.float32):
        X = np.zeros((3, k + 2), dtype=dtype)
        X[:, k + 1] = 1
        H = np.ones_like(X)
        for _ in range(5):
            X, H, _ = O.half_step(X, H, Ya, hist, fixed=k + 1, alpha=m.alpha_, lam=m.lam, lr=m.lr, dtype=dtype)
        ref[dtype] = X
    _held('LMF fold_in rows', rows, ref[np.float64][:, :k], ref[np.float32][:, :k])
    _held('LMF fold_in biases', biases, ref[np.float64][:, k], ref[np.float32][:, k])
    none, bias = m.fold_in([[]], steps=2)                                       # a user without likes still steps
    assert none.shape == (1, k) and (none != 0).any() and bias[0] < 0
