"""K26 (the sparse product and CER's E-step by conjugate gradients) without a GPU: the oracle of tests/_estep_oracle.py against itself and
against the direct solve of tests/_cer_oracle.py on the inputs the GPU tests use, the sparse loader of als.CER under estep='cg', the
constructor and command-line rules, and everything of the C ABI that is checked before a device is touched."""
import ctypes
import os
import pickle
import re

import numpy as np
import pytest
import scipy.sparse as ss

import _estep_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _column_errors(E, exact):
    return np.sqrt(((np.asarray(E, np.float64) - exact) ** 2).sum(axis=0))


@pytest.mark.parametrize('lv,le,steps', O.CONVERGE)
def test_float64_recurrence_converges_inside_the_cg_bound(lv, le, steps):
    """per column, in the 2-norm: |E_m - E*| <= 2 sqrt(kappa) ((sqrt(kappa) - 1) / (sqrt(kappa) + 1))^m |E_0 - E*|, E* the direct solve
    of _cer_oracle.e_step, kappa from eigvalsh of the dense system -- on the inputs of the GPU convergence test, and at every step count
    up to the one it uses.

    The bound is a statement about exact arithmetic.  At lv = 10, le = 1e4 (kappa = 1.028) and 8 steps it is 1.2e-17 of the start
    error, below what float64 can hold (2^-53 = 1.1e-16; the recurrence reaches 1.3e-16).  So the float64 run is held to the bound plus
    the resolution of the two computations compared: 64 * 2^-53 (|E_0c| + |E*_c|) -- E is built in place from E_0, so every update
    rounds at the size of E_0, and np.linalg.solve rounds at the size of E*; 64 ulps covers the eight steps and the solve generously.
    At every other step count here that floor is far below the bound and changes nothing."""
    F = O.features(O.CONVERGE_D)
    V, E0 = O.tables(O.CONVERGE_D, O.CONVERGE_K)
    exact = O.e_step(np.asarray(F.todense(), np.float64), V, lv=lv, le=le)
    start = _column_errors(E0, exact)
    floor = 64 * 2.0 ** -53 * (np.sqrt((exact ** 2).sum(axis=0)) + np.sqrt((E0.astype(np.float64) ** 2).sum(axis=0)))
    for m in sorted({1, 3, steps}):
        kappa, bound = O.cg_bound(F, lv, le, m)
        E, refused = O.estep_cg(F, V, E0, lv=lv, le=le, steps=m, heavy_from=O.TEST_HEAVY_FROM, done=0.0)
        err = _column_errors(E, exact)
        worst = (err / start).max()
        print('K26 float64 CG lv=%g le=%g kappa=%.4g steps=%d: worst column error %.3g of the start, bound %.3g' % (lv, le, kappa, m, worst, bound))
        assert not refused.any() and (err <= bound * start + floor).all()
    assert bound < 1e-3                                               # (the GPU test's step count says something)


def test_float32_oracle_follows_float64_on_the_gpu_tests_inputs():
    """e32 is finite and nonzero on every generic case the GPU test measures with it"""
    for d in O.GENERIC_D:
        for k in (1, 50):
            e64, e32, r64, r32 = O.estep_case(d, k, 3, O.GENERIC['lv'], O.GENERIC['le'])
            err = np.abs(e32 - e64).max() / np.abs(e64).max()
            print('K26 oracle d=%d k=%d steps=3: e32 %.3g' % (d, k, err))
            assert e32.dtype == np.float32 and np.isfinite(e32).all() and 0 < err < 1e-4
            assert not r64.any() and not r32.any()


def test_spmm_oracle_both_row_forms():
    """exact inputs (multiples of 1/8): every order gives the same sum, so the chain, the slab form and float64 agree bit for bit; on
    generic inputs the two float32 forms differ from float64 by rounding only"""
    rng = np.random.Generator(np.random.PCG64(41))
    A = ss.random(9, 400, density=0.5, random_state=np.random.RandomState(3), format='csr', dtype=np.float32)
    A.data = (rng.integers(-16, 17, len(A.data)) / 8).astype(np.float32)
    X = (rng.integers(-16, 17, (400, 5)) / 8).astype(np.float32)
    Z = (rng.integers(-16, 17, (9, 5)) / 8).astype(np.float32)
    ref = O.spmm(A, X, alpha=0.5, Z=Z, beta=2.0)
    assert max(np.diff(A.indptr)) > 64
    for heavy_from in (64, 1 << 30):
        got = O.spmm(A, X, alpha=0.5, Z=Z, beta=2.0, heavy_from=heavy_from, dtype=np.float32)
        assert got.dtype == np.float32
        np.testing.assert_array_equal(got.astype(np.float64), ref)
    A.data = rng.standard_normal(len(A.data)).astype(np.float32)
    X = rng.standard_normal((400, 5)).astype(np.float32)
    ref = O.spmm(A, X)
    mag = np.abs(A).astype(np.float64) @ np.abs(X).astype(np.float64)
    for heavy_from in (64, 1 << 30):
        got = O.spmm(A, X, heavy_from=heavy_from, dtype=np.float32)
        assert (np.abs(got - ref) <= 300 * 2.0 ** -24 * mag).all() and (got != ref.astype(np.float32)).any()


def test_dot_columns_is_the_stated_tree():
    rng = np.random.Generator(np.random.PCG64(42))
    for d in (1, 63, 64, 65, 1024, 1025, 2100):
        a, b = rng.standard_normal((d, 3)).astype(np.float32), rng.standard_normal((d, 3)).astype(np.float32)
        got, ref = O.dot_columns(a, b, np.float32), O.dot_columns(a, b)
        assert got.dtype == np.float32 and (np.abs(got - ref) <= 2.0 ** -18 * np.abs(a.astype(np.float64) * b).sum(axis=0)).all()
    e = ((np.arange(2100 * 2) % 5 - 2) / 4).astype(np.float32).reshape(2100, 2)     # exact: every order gives the same sum
    np.testing.assert_array_equal(O.dot_columns(e, e, np.float32).astype(np.float64), O.dot_columns(e, e))


def test_a_column_whose_pq_is_not_positive_is_refused_and_kept():
    F = O.features(63)
    V, E0 = O.tables(63, 16)
    for dtype in (np.float64, np.float32):
        E, refused = O.estep_cg(F, V, E0, lv=-1.0, le=1e-3, steps=3, dtype=dtype)     # lv < 0: the operator is indefinite
        assert refused.any()
        np.testing.assert_array_equal(E[:, refused], E0[:, refused].astype(dtype))


# ---- als.CER --------------------------------------------------------------------------------------------------------------------------
def _g2(golden_dir, **over):
    import als
    d = os.path.join(golden_dir, 'g2')
    m = als.CER(k=O.E2E['k'], d=over.pop('d', O.E2E['d']), lu=O.E2E['lu'], lv=O.E2E['lv'], le=O.E2E['le'], **over)
    m.load_training_data(os.path.join(d, 'uid'), os.path.join(d, 'vid'), os.path.join(d, 'f0tr.txt'), seed=O.E2E['seed'])
    return m, os.path.join(d, 'vid')


def test_load_content_data_keeps_the_features_sparse(golden_dir, tmp_path):
    dense_model, vid = _g2(golden_dir)
    feat = O.e2e_features(dense_model.n_items)
    order = np.random.Generator(np.random.PCG64(43)).permutation(dense_model.n_items)[:-3]      # the file's own row order; three items have no features
    ids = [line.strip() for line in open(vid)]
    fid = str(tmp_path / 'fid')
    with open(fid, 'w') as fh:
        fh.write(''.join(ids[j] + '\n' for j in order))
    for name, raw in (('sparse.pkl', ss.csr_matrix(feat[order])), ('coo.pkl', ss.coo_matrix(feat[order])), ('dense.pkl', feat[order])):
        path = str(tmp_path / name)
        with open(path, 'wb') as fh:
            pickle.dump(raw, fh)
        dense_model.load_content_data(path, fid)
        assert isinstance(dense_model.feat, np.ndarray) and dense_model.feat.dtype == np.float32
        m, _ = _g2(golden_dir, estep='cg')
        m.load_content_data(path, fid)
        assert ss.isspmatrix_csr(m.feat) and m.feat.dtype == np.float32 and m.feat.shape == (m.n_items, m.d)
        assert m.feat.has_canonical_format and (m.feat.data != 0).all()
        np.testing.assert_array_equal(m.feat.toarray(), dense_model.feat)
        assert not dense_model.feat[[j for j in range(m.n_items) if j not in set(order.tolist())]].any()
    m, _ = _g2(golden_dir, estep='cg', d=O.E2E['d'] + 1)
    with pytest.raises(ValueError, match='width'):
        m.load_content_data(str(tmp_path / 'sparse.pkl'), fid)


def test_canonical_csr_and_the_byte_model():
    import als
    dup = ss.coo_matrix((np.asarray([1.0, 2.0, 0.0, 4.0]), ([0, 0, 1, 1], [3, 3, 0, 2])), shape=(2, 5))
    c = als.canonical_csr(dup)
    assert c.has_canonical_format and c.dtype == np.float32 and c.nnz == 2
    np.testing.assert_array_equal(c.toarray(), np.asarray([[0, 0, 0, 3, 0], [0, 0, 4, 0, 0]], np.float32))
    np.testing.assert_array_equal(als.canonical_csr(dup.toarray()).toarray(), c.toarray())
    dense, _ = als.cer_train_bytes(1000, 10000, 50, 200000)
    assert dense >= 8 * 200000 ** 2                                   # 320 GB: what no device holds


def test_a_feat_of_the_wrong_shape_is_named_before_any_device_is_touched(golden_dir):
    """assigned directly, sparse or dense, under either E-step: train() raises a ValueError about feat (this machine may have no device)"""
    for estep in ('cg', 'cholesky'):
        m, _ = _g2(golden_dir, estep=estep)
        for feat in (ss.csr_matrix((m.n_items, m.d + 1), dtype=np.float32), ss.csr_matrix((m.n_items - 1, m.d), dtype=np.float32),
                     np.zeros((m.n_items, m.d - 1), np.float32)):
            m.feat = feat
            with pytest.raises(ValueError, match=r'feat has shape .* the model needs \(%d, %d\)' % (m.n_items, m.d)):
                m.train(max_iter=1, verbose=False)
        m.feat = None
        with pytest.raises(ValueError, match='load_content_data'):
            m.train(max_iter=1, verbose=False)


def test_constructor_rules():
    import als
    m = als.CER(k=8, d=4)
    assert (m.estep, m.e_steps) == ('cholesky', 8)
    m = als.CER(k=200, d=4, solver='cg', estep='cg', e_steps=3)
    assert (m.estep, m.e_steps, m.solver) == ('cg', 3, 'cg')
    for make in (lambda: als.CER(k=8, d=4, estep='qr'), lambda: als.CER(k=8, d=4, e_steps=0), lambda: als.CER(k=8, d=4, estep='cg', e_steps=0),
                 lambda: als.CER(k=8, d=4, estep='cg', e_steps=2.5), lambda: als.CER(k=8, d=4, estep='cg', e_steps=True)):
        with pytest.raises(ValueError):
            make()
    with pytest.raises(TypeError):
        als.WMF(k=8, estep='cg')                                      # the E-step is CER's


def test_train_als_takes_the_estep(tmp_path, capsys):
    """every refusal is the new rule's own message (an unknown flag would say 'unrecognized arguments'), and a valid --estep cg gets
    past the argument rules: it ends at the data directory, which is empty"""
    import train_als
    cer = ['--model', 'cer', '--content', 'x.pkl', '--dim', '3']
    dpm = ['--model', 'dpm', '--content', 'x.pkl', '--dim', '3']
    for argv, message in ((['--estep', 'cg'], 'go with --model cer'), (['--e-steps', '3'], 'go with --model cer'),
                          (dpm + ['--estep', 'cg'], 'go with --model cer'), (cer + ['--estep', 'qr'], "invalid choice: 'qr'"),
                          (cer + ['--estep', 'cg', '--e-steps', '0'], 'e_steps = 0 must be an integer, at least 1'),
                          (cer + ['--e-steps', '3'], 'goes with --estep cg'), (cer + ['--estep', 'cholesky', '--e-steps', '3'], 'goes with --estep cg')):
        with pytest.raises(SystemExit):
            train_als.main(argv + ['-d', str(tmp_path)])
        err = capsys.readouterr().err
        assert message in err and 'unrecognized arguments' not in err, (argv, err)
    for argv in (cer + ['--estep', 'cg'], cer + ['--estep', 'cg', '--e-steps', '3'], cer + ['--estep', 'cholesky'], cer):
        with pytest.raises(ValueError, match='list no users or no items'):
            train_als.main(argv + ['-d', str(tmp_path / 'empty')])
        assert 'error' not in capsys.readouterr().err


def test_library_declares_and_exports_the_new_symbols():
    import tkr_hip
    header = open(os.path.join(ROOT, 'include', 'tkr.h')).read()
    declared = set(re.findall(r'^int(?:32_t|64_t)? (tkr_\w+)\(', header, flags=re.M))
    for name in ('tkr_csr_spmm', 'tkr_estep_cg'):
        assert name in declared and name in tkr_hip.EXPORTS
    for name in ('tkr_csr_spmm_workspace_bytes', 'tkr_estep_cg_workspace_bytes'):
        assert name in declared and name in tkr_hip.EXPORTS_I64
    for name, value in (('TKR_SPMM_SLAB', tkr_hip.SPMM_SLAB), ('TKR_SPMM_HEAVY_FROM', tkr_hip.SPMM_HEAVY_FROM), ('TKR_ESTEP_SLAB', tkr_hip.ESTEP_SLAB)):
        assert re.search(r'#define %s %d\b' % (name, value), header)
    assert (tkr_hip.SPMM_SLAB, tkr_hip.SPMM_HEAVY_FROM, tkr_hip.ESTEP_SLAB, tkr_hip.ESTEP_STEPS) == (O.SPMM_SLAB, O.HEAVY_FROM, O.DOT_SLAB, 8)
    assert issubclass(tkr_hip.EstepRefused, tkr_hip.TkrError) and len(tkr_hip._ESTEP_REFUSED) == 4


def _lib():
    import tkr_hip
    if not os.path.exists(tkr_hip.LIB_PATH):
        pytest.skip('%s is not built (python __graft_entry__.py build): nothing to load' % tkr_hip.LIB_PATH)
    return ctypes.CDLL(tkr_hip.LIB_PATH)


def test_the_built_library_exports_the_new_symbols():
    lib = _lib()
    for name in ('tkr_csr_spmm', 'tkr_estep_cg', 'tkr_csr_spmm_workspace_bytes', 'tkr_estep_cg_workspace_bytes'):
        assert hasattr(lib, name), name


def test_size_functions():
    lib = _lib()
    import als
    one, room = lib.tkr_csr_spmm_workspace_bytes, lib.tkr_estep_cg_workspace_bytes
    one.restype = room.restype = ctypes.c_int64
    one.argtypes = [ctypes.c_int64]
    room.argtypes = [ctypes.c_int64, ctypes.c_int64, ctypes.c_int32]
    assert one(0) == -1 and one(1 << 31) == -1 and one(7) % 16 == 0 and one(7) >= 16 + 4 * 7
    assert room(0, 5, 4) == -1 and room(5, 0, 4) == -1 and room(5, 5, 0) == -1 and room(5, 5, 513) == -2 and room(1 << 31, 5, 4) == -1
    big = (1 << 31) - 1                                                          # rows the argument checks allow; at k = 512 a table of 2^40 floats
    assert room(big, 5, 512) == -2 and room(5, big, 512) == -2 and room(big, 5, 257) == -2 and room(big, 5, 256) > 0
    for n, d, k in ((300, 400, 16), (1, 1, 1), (10000, 200000, 50), (7, 2100, 512)):
        need = room(n, d, k)
        slabs = (d + 1023) // 1024
        assert need % 16 == 0 and need >= 4 * k * (n + 5 * d + 2 * slabs) + 4 * max(n, d)
        assert need <= 4 * k * (n + 5 * d + 2 * slabs) + 4 * max(n, d) + 16 * 16 + 5 * 4 * k
    sparse, tables, ws = als.cer_sparse_train_bytes(70000, 10000, 50, 200000, 10 ** 6)
    assert ws == room(10000, 200000, 50) and sparse == 16 * 10 ** 6 + 8 * 210002 and sparse + tables + ws < 1 << 30     # under 1 GB where FF needs 320


def test_raw_abi_refuses_before_any_device_access():
    """every refused argument returns TKR_E_INVAL (-1) or TKR_E_UNSUPPORTED (-2) before anything is launched: the pointers below are
    addresses nobody owns, and this machine may have no device"""
    lib = _lib()
    V, i32, i64, f64 = ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64, ctypes.c_double
    mm, es = lib.tkr_csr_spmm, lib.tkr_estep_cg
    mm.restype = es.restype = ctypes.c_int
    mm.argtypes = [V, V, V, i64, i64, i32, V, i32, f64, V, f64, V, i64, V, i64, V, V]
    es.argtypes = [V, V, V, V, V, V, i64, i64, i64, V, i32, V, f64, f64, i32, i64, V, i64, V, V]
    P = 0x10000                                                                 # aligned, never followed
    nan, inf = float('nan'), float('inf')
    #       ptr col val nnz n_rows n_cols X  k  alpha Z  beta out heavy_from ws bytes status stream
    good = [P, P, P, 7, 3, 5, P, 4, 1.0, P, 0.5, P, 2048, P, 1 << 20, P, None]
    walk = [(0, None, -1), (1, None, -1), (2, None, -1), (6, None, -1), (11, None, -1), (15, None, -1),
            (0, P + 4, -1), (1, P + 2, -1), (2, P + 2, -1), (6, P + 2, -1), (9, P + 2, -1), (11, P + 2, -1), (13, P + 8, -1), (15, P + 4, -1),
            (3, -1, -1), (4, 0, -1), (4, 1 << 31, -1), (5, 0, -1), (7, 0, -1), (7, 513, -2), (8, nan, -1), (10, inf, -1), (12, 0, -1), (14, -1, -1)]
    for at, bad, rc in walk:
        args = list(good)
        args[at] = bad
        assert mm(*args) == rc, (at, bad)
    args = list(good)
    args[12], args[13] = 3, None                                                # a row may be heavy and there is no room for the list
    assert mm(*args) == -1
    args[13], args[14] = P, 16
    assert mm(*args) == -1
    #       f_ptr f_col f_val t_ptr t_col t_val nnz n_items d V  k  E  lv  le  steps heavy_from ws bytes status stream
    good = [P, P, P, P, P, P, 7, 3, 5, P, 4, P, 10.0, 1e4, 8, 2048, P, 1 << 20, P, None]
    walk = [(at, None, -1) for at in (0, 1, 2, 3, 4, 5, 9, 11, 16, 18)] + \
           [(0, P + 4, -1), (3, P + 4, -1), (1, P + 2, -1), (5, P + 2, -1), (9, P + 2, -1), (11, P + 2, -1), (16, P + 8, -1), (18, P + 4, -1),
            (6, -1, -1), (7, 0, -1), (8, 0, -1), (7, 1 << 31, -1), (8, 1 << 31, -1), (10, 0, -1), (10, 513, -2), (12, 0.0, -1), (12, nan, -1),
            (13, -1.0, -1), (13, inf, -1), (14, 0, -1), (14, -2, -1), (15, 0, -1), (17, 64, -1), (17, -1, -1)]
    for at, bad, rc in walk:
        args = list(good)
        args[at] = bad
        assert es(*args) == rc, (at, bad)
    for at in (7, 8):                                                           # a table the flat launches cannot cover
        args = list(good)
        args[at], args[10], args[17] = (1 << 31) - 1, 512, 1 << 62
        assert es(*args) == -2, at
