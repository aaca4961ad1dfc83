"""K26 on the GPU (csrc/sparse.hip tkr_csr_spmm and tkr_estep_cg, top-k-rec_amd/als.py CER(estep='cg')) against tests/_estep_oracle.py.

The yardstick is K20's (tests/test_gpu_als.py): with x64 the float64 oracle on the same fp32 inputs and x32 the float32 one (the kernel's
stated order, operation by operation), e32 = max|x32 - x64| / max|x64| per case, and the kernel has to stay within F * max(e32, 2^-23).
F = 16 is a condition of the design, not a knob.  Worst ratios measured on an MI355X (DESIGN.md section 4 K26 keeps them; every test
prints its own): the product 0.90 (F^T, k = 16; every row has the float32 oracle's bits), the E-step 1.00 in all 60 cases (err = e32:
the kernel and the oracle run the same operations), CER on g2 fue / fie / cold fie / E 1.06 / 0.69 / 0.77 / 0.77, its losses 1.16."""
import ctypes as C
import functools
import os
import pickle

import numpy as np
import pytest
import scipy.sparse as ss
import torch

import _estep_oracle as O

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = 16.0
FLOOR = 2.0 ** -23
HEAVY = O.TEST_HEAVY_FROM


def _dev(a):
    return torch.from_numpy(np.array(a, order='C')).cuda()               # (a copy: the shared oracle arrays are read-only)


def _bits(a):
    return np.ascontiguousarray(a).view(np.int32)


def _ratio(got, x64, x32):
    scale = np.abs(x64).max()
    err, e32 = np.abs(got - x64).max() / scale, np.abs(x32 - x64).max() / scale
    return err / max(e32, FLOOR), err, e32


def _csr(m):
    import tkr_hip
    return tkr_hip.csr_upload(m, 'cuda')


def _eighths(rng, shape, low=-16, high=17):
    return (rng.integers(low, high, shape) / 8).astype(np.float32)


def _rows_matrix(rng, lengths, n_cols, values):
    """a CSR whose row r holds lengths[r] distinct ascending columns"""
    ptr = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)
    col = np.concatenate([np.sort(rng.choice(n_cols, size=m, replace=False)) for m in lengths] + [np.zeros(0, np.int64)]).astype(np.int32)
    return ss.csr_matrix((values(len(col)), col, ptr), shape=(len(lengths), n_cols))


# ---- a. the product, bit for bit on exact inputs ---------------------------------------------------------------------------------------
@pytest.mark.parametrize('with_z', [False, True])
@pytest.mark.parametrize('k', [1, 5, 50, 64, 65, 128, 200, 512])
def test_spmm_is_exact_on_exact_inputs(k, with_z):
    """values and X multiples of 1/8 below 2: every partial sum is exact in fp32, so any order gives float64 NumPy's bits.  Rows of 0,
    1, 300 (slabs of 256 with a tail of 44) and exactly heavy_from = 64 nonzeros among 66 others: 70 rows are 3 workgroups at k <= 8
    and 18 above k = 32"""
    import tkr_hip
    rng = np.random.Generator(np.random.PCG64([50, k]))
    lengths = [0, 1, 300, HEAVY] + list(rng.integers(0, 40, 66))
    A = _rows_matrix(rng, lengths, 400, lambda n: _eighths(rng, n))
    X, Z = _eighths(rng, (400, k)), _eighths(rng, (70, k))
    ref = 0.5 * (A.astype(np.float64) @ X.astype(np.float64)) + (2.0 * Z if with_z else 0.0)
    assert (ref.astype(np.float32) == ref).all()
    more = dict(Z=_dev(Z), beta=2.0) if with_z else {}
    for heavy_from in (HEAVY, None):                                  # the row of 300: slabs, and one chain
        got = tkr_hip.csr_spmm(_csr(A), _dev(X), alpha=0.5, heavy_from=heavy_from, **more).cpu().numpy()
        np.testing.assert_array_equal(_bits(got), _bits(ref.astype(np.float32)), err_msg='heavy_from = %r' % heavy_from)
    for r in (0, 1, 2, 3):                                            # n_rows = 1
        one = tkr_hip.csr_spmm(_csr(A[r]), _dev(X), alpha=0.5, heavy_from=HEAVY, **(dict(Z=_dev(Z[r:r + 1]), beta=2.0) if with_z else {}))
        np.testing.assert_array_equal(_bits(one.cpu().numpy()), _bits(ref[r:r + 1].astype(np.float32)), err_msg='row %d alone' % r)


# ---- b. a row's bits do not depend on the call -----------------------------------------------------------------------------------------
@pytest.mark.parametrize('k', [5, 50, 200])
def test_a_rows_bits_do_not_depend_on_the_call(k):
    import tkr_hip
    rng = np.random.Generator(np.random.PCG64([51, k]))
    lengths = list(rng.integers(0, 90, 700))
    lengths[0], lengths[333], lengths[699] = 300, 300, 41
    A = _rows_matrix(rng, lengths, 500, lambda n: rng.standard_normal(n).astype(np.float32))
    X = _dev(rng.standard_normal((500, k)).astype(np.float32))
    whole = tkr_hip.csr_spmm(_csr(A), X, alpha=1.5, heavy_from=HEAVY).cpu().numpy()
    again = tkr_hip.csr_spmm(_csr(A), X, alpha=1.5, heavy_from=HEAVY).cpu().numpy()
    np.testing.assert_array_equal(_bits(whole), _bits(again))
    for r in (0, 1, 7, 333, 350, 698, 699):
        alone = tkr_hip.csr_spmm(_csr(A[r]), X, alpha=1.5, heavy_from=HEAVY).cpu().numpy()
        np.testing.assert_array_equal(_bits(alone[0]), _bits(whole[r]), err_msg='row %d' % r)


# ---- c. generic inputs against the oracle ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize('k', O.GENERIC_K)
def test_spmm_against_the_oracle(k):
    """F of the E-step tests and its transpose (row 0 of it: 300 nonzeros, heavy at heavy_from = 64), X standard normal.
    Measured on an MI355X: see DESIGN.md section 4 K26"""
    import tkr_hip
    Fm = O.features(400)
    for name, A in (('F', Fm), ('Ft', O.canonical(Fm.T))):
        rng = np.random.Generator(np.random.PCG64([52, k, A.shape[0]]))
        X = rng.standard_normal((A.shape[1], k)).astype(np.float32)
        Z = rng.standard_normal((A.shape[0], k)).astype(np.float32)
        x64 = O.spmm(A, X, alpha=0.1, Z=Z, beta=1.0)
        x32 = O.spmm(A, X, alpha=0.1, Z=Z, beta=1.0, heavy_from=HEAVY, dtype=np.float32)
        got = tkr_hip.csr_spmm(_csr(A), _dev(X), alpha=0.1, Z=_dev(Z), beta=1.0, heavy_from=HEAVY).cpu().numpy()
        ratio, err, e32 = _ratio(got.astype(np.float64), x64, x32.astype(np.float64))
        print('K26 spmm %s k=%d: err %.3g e32 %.3g ratio %.3g; rows that differ from the float32 oracle: %d'
              % (name, k, err, e32, ratio, int((_bits(got) != _bits(x32)).any(axis=1).sum())))
        assert np.isfinite(got).all() and ratio <= F, (name, err, e32)


def _estep(Fm, V, E0, *, lv, le, steps, heavy_from=HEAVY, check=True):
    import tkr_hip
    E = _dev(E0)
    out = tkr_hip.estep_cg(_csr(Fm), _csr(O.canonical(Fm.T)), _dev(V), E, lv=lv, le=le, steps=steps, heavy_from=heavy_from, check=check)
    return (E.cpu().numpy(), int(out[1].item())) if not check else E.cpu().numpy()


@pytest.mark.parametrize('steps', O.GENERIC_STEPS)
@pytest.mark.parametrize('k', O.GENERIC_K)
@pytest.mark.parametrize('d', O.GENERIC_D)
def test_estep_against_the_oracle(d, k, steps):
    """n_items = 300, 12 nonzeros per row and column 0 in every item, lv = 0.1, le = 1, E0 standard normal.  d = 1, 63, 400: one
    dot-product slab with a tail; 1025, 2100: two and three.  Measured on an MI355X: see DESIGN.md section 4 K26"""
    e64, e32, r64, r32 = O.estep_case(d, k, steps, O.GENERIC['lv'], O.GENERIC['le'])
    V, E0 = O.tables(d, k)
    got = _estep(O.features(d), V, E0, steps=steps, **O.GENERIC)
    again = _estep(O.features(d), V, E0, steps=steps, **O.GENERIC)
    np.testing.assert_array_equal(_bits(got), _bits(again))                      # two calls, the same bits
    ratio, err, x32 = _ratio(got.astype(np.float64), e64, e32.astype(np.float64))
    print('K26 estep d=%d k=%d steps=%d: err %.3g e32 %.3g ratio %.3g' % (d, k, steps, err, x32, ratio))
    assert np.isfinite(got).all() and (got != E0).any() and ratio <= F, (err, x32)


# ---- d. convergence ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('lv,le,steps', O.CONVERGE)
def test_estep_converges_to_the_direct_solve(lv, le, steps):
    """per column, in the 2-norm: the kernel's E is within the bound of conjugate gradients of the float64 direct solve, or within
    F * e32 of it, whichever is larger (tests/test_estep_cpu.py holds the float64 recurrence to the same bound on the same inputs)"""
    d, k = O.CONVERGE_D, O.CONVERGE_K
    Fm = O.features(d)
    V, E0 = O.tables(d, k)
    exact = O.e_step(np.asarray(Fm.todense(), np.float64), V, lv=lv, le=le)
    e64, e32, _, _ = O.estep_case(d, k, steps, lv, le)
    kappa, bound = O.cg_bound(Fm, lv, le, steps)
    got = _estep(Fm, V, E0, lv=lv, le=le, steps=steps).astype(np.float64)
    norm = lambda a: np.sqrt((a ** 2).sum(axis=0))
    err, start, yard = norm(got - exact), norm(E0 - exact), norm(e32 - e64)
    allowed = np.maximum(bound * start, F * np.maximum(yard, FLOOR * norm(exact)))
    print('K26 converge lv=%g le=%g kappa=%.4g steps=%d: worst err %.3g of the start, bound %.3g, worst err / allowed %.3g'
          % (lv, le, kappa, steps, (err / start).max(), bound, (err / allowed).max()))
    assert (err <= allowed).all()
    assert (err / start).max() < 1e-4                                           # (and it did converge)


# ---- e. untrusted input -----------------------------------------------------------------------------------------------------------------
def _spoiled(what):
    """-> (F, Ft as device Csr, V tensor, expected word) with one thing wrong"""
    n, d, k = O.N_ITEMS, 63, 16
    Fm = O.features(d)
    A, At = _csr(Fm), _csr(O.canonical(Fm.T))
    V = _dev(O.tables(d, k)[0])
    if what == 'col d in F':
        A.col[int(A.ptr[7].item()) + 2] = d
        word = 4 * 7 + 0
    elif what == 'col -1 in Ft':
        At.col[int(At.ptr[5].item())] = -1
        word = 4 * (n + 5) + 0
    elif what == 'descending ptr in F':
        A.ptr[6] = A.ptr[5] - 1
        word = 4 * 5 + 3
    elif what == 'descending ptr in Ft':
        At.ptr[3] = At.ptr[2] - 1
        word = 4 * (n + 2) + 3
    elif what == 'nan in val of F':
        A.val[int(A.ptr[11].item())] = float('nan')
        word = 4 * 11 + 1
    elif what == 'inf in val of Ft':
        At.val[int(At.ptr[1].item()) - 1] = float('inf')                        # the last nonzero of row 0, the heavy one
        word = 4 * (n + 0) + 1
    else:
        V[9, k - 1] = float('-inf') if what == '-inf in V' else float('inf')
        word = 4 * 9 + 1
    return A, At, V, word


@pytest.mark.parametrize('what', ['col d in F', 'col -1 in Ft', 'descending ptr in F', 'descending ptr in Ft', 'nan in val of F',
                                  'inf in val of Ft', 'inf in V', '-inf in V'])
def test_a_refused_input_is_named_and_E_is_untouched(what):
    import tkr_hip
    A, At, V, word = _spoiled(what)
    E0 = O.tables(63, 16)[1]
    for heavy_from in (HEAVY, None):
        E = _dev(E0)
        _, status = tkr_hip.estep_cg(A, At, V, E, lv=0.1, le=1.0, steps=3, heavy_from=heavy_from, check=False)
        assert int(status.item()) == word, what
        np.testing.assert_array_equal(_bits(E.cpu().numpy()), _bits(E0))
    with pytest.raises(tkr_hip.EstepRefused) as info:
        tkr_hip.estep_cg(A, At, V, _dev(E0), lv=0.1, le=1.0, steps=3)
    assert (info.value.row, info.value.kind) == (word >> 2, word & 3)


def test_a_column_that_overflows_is_refused_alone():
    """V[:, 3] = 1e25: rho of column 3 is infinite in fp32, p . q is not finite -> 4 * 3 + 2; the column keeps its bits, the others
    are the bits of the clean call"""
    import tkr_hip
    d, k = 63, 16
    Fm = O.features(d)
    V, E0 = O.tables(d, k)
    clean = _estep(Fm, V, E0, lv=0.1, le=1.0, steps=3)
    Vb = V.copy()
    Vb[:, 3] = 1e25
    got, status = _estep(Fm, Vb, E0, lv=0.1, le=1.0, steps=3, check=False)
    assert status == 4 * 3 + 2
    others = [c for c in range(k) if c != 3]
    np.testing.assert_array_equal(_bits(got[:, 3]), _bits(E0[:, 3]))
    np.testing.assert_array_equal(_bits(got[:, others]), _bits(clean[:, others]))
    with pytest.raises(tkr_hip.EstepRefused, match='column 3'):
        _estep(Fm, Vb, E0, lv=0.1, le=1.0, steps=3)


def test_spmm_leaves_a_refused_row_unwritten():
    import tkr_hip
    rng = np.random.Generator(np.random.PCG64(53))
    A = _rows_matrix(rng, [5, 300, 9, 0, 12], 400, lambda n: rng.standard_normal(n).astype(np.float32))
    X = _dev(rng.standard_normal((400, 7)).astype(np.float32))
    good = tkr_hip.csr_spmm(_csr(A), X, heavy_from=HEAVY).cpu().numpy()
    for row, at, kind in ((1, 299, 0), (2, 0, 0), (1, 17, 1), (4, 11, 1)):
        B = _csr(A)
        e = int(B.ptr[row].item()) + at
        if kind == 0:
            B.col[e] = 400
        else:
            B.val[e] = float('nan')
        out = torch.full((5, 7), 77.0, device='cuda')
        _, status = tkr_hip.csr_spmm(B, X, heavy_from=HEAVY, out=out, check=False)
        assert int(status.item()) == 4 * row + kind
        out = out.cpu().numpy()
        assert (out[row] == 77.0).all()
        others = [r for r in range(5) if r != row]
        np.testing.assert_array_equal(_bits(out[others]), _bits(good[others]))
    B = _csr(A)
    B.ptr[3] = B.ptr[2] - 1                                                     # row 2 descends; row 3 is a row again
    _, status = tkr_hip.csr_spmm(B, X, heavy_from=HEAVY, check=False)
    assert int(status.item()) == 4 * 2 + 3
    with pytest.raises(tkr_hip.EstepRefused) as info:
        tkr_hip.csr_spmm(B, X, heavy_from=HEAVY)
    assert (info.value.row, info.value.kind) == (2, 3)


def test_raw_abi_argument_checks():
    """what tests/test_estep_cpu.py walks without a device, here with E on one: a refused call writes nothing, the good call runs"""
    lib = C.CDLL(os.path.join(ROOT, 'top-k-rec_amd', 'libtkr_hip.so'))
    es, size = lib.tkr_estep_cg, lib.tkr_estep_cg_workspace_bytes
    es.restype, size.restype = C.c_int, C.c_int64
    size.argtypes = [C.c_int64, C.c_int64, C.c_int32]
    V_, i32, i64, f64 = C.c_void_p, C.c_int32, C.c_int64, C.c_double
    es.argtypes = [V_, V_, V_, V_, V_, V_, i64, i64, i64, V_, i32, V_, f64, f64, i32, i64, V_, i64, V_, V_]
    d, k = 63, 16
    Fm = O.features(d)
    A, At = _csr(Fm), _csr(O.canonical(Fm.T))
    V, E0 = O.tables(d, k)
    Vd, Ed = _dev(V), _dev(E0)
    ws = torch.empty(size(O.N_ITEMS, d, k) // 8, dtype=torch.int64, device='cuda')
    status = torch.empty(1, dtype=torch.int64, device='cuda')
    p = lambda t: C.c_void_p(t.data_ptr())
    args = [p(A.ptr), p(A.col), p(A.val), p(At.ptr), p(At.col), p(At.val), A.nnz, O.N_ITEMS, d, p(Vd), k, p(Ed), 0.1, 1.0, 3, HEAVY, p(ws), ws.numel() * 8,
            p(status), C.c_void_p(torch.cuda.current_stream().cuda_stream)]
    for at, bad, rc in ((0, None, -1), (4, None, -1), (9, None, -1), (11, None, -1), (16, None, -1), (18, None, -1), (10, 0, -1), (10, 513, -2),
                        (14, 0, -1), (15, 0, -1), (17, ws.numel() * 8 - 16, -1), (12, 0.0, -1), (13, float('nan'), -1), (6, -1, -1), (7, 0, -1)):
        bad_args = list(args)
        bad_args[at] = bad
        assert es(*bad_args) == rc, at
    torch.cuda.synchronize()
    np.testing.assert_array_equal(_bits(Ed.cpu().numpy()), _bits(E0))
    assert es(*args) == 0 and int(status.item()) == -1
    e64, e32, _, _ = O.estep_case(d, k, 3, 0.1, 1.0)
    assert _ratio(Ed.cpu().numpy().astype(np.float64), e64, e32.astype(np.float64))[0] <= F


# ---- f. als.CER(estep='cg') end to end ----------------------------------------------------------------------------------------------------
E_STEPS = 8


def _g2(golden_dir):
    return os.path.join(golden_dir, 'g2')


def _model(golden_dir, **over):
    import als
    d = _g2(golden_dir)
    hyper = dict(k=O.E2E['k'], d=O.E2E['d'], lu=O.E2E['lu'], lv=O.E2E['lv'], le=O.E2E['le'], a=O.E2E['a'], b=O.E2E['b'], estep='cg', e_steps=E_STEPS)
    hyper.update(over)
    m = als.CER(**hyper)
    m.load_training_data(os.path.join(d, 'uid'), os.path.join(d, 'vid'), os.path.join(d, 'f0tr.txt'), seed=O.E2E['seed'])
    return m


@functools.lru_cache(maxsize=None)
def _trained(golden_dir):
    m = _model(golden_dir)
    m.feat = ss.csr_matrix(O.e2e_features(m.n_items))                           # assigned directly, as a CSR
    U0, V0, E0 = O.e2e_start(m.n_users, m.n_items)
    up, uc, ip, ic = m._csr
    likes = (O.csr_rows(up, uc), O.csr_rows(ip, ic))
    hyper = dict(a=m.a, b=m.b, lu=m.lu, lv=m.lv, le=m.le, e_steps=E_STEPS)
    m.train(max_iter=O.E2E['iters'], tol=0.0, verbose=False)
    t64 = O.cer_train_cg_estep(U0, V0, E0, m.feat, *likes, max_iter=O.E2E['iters'], tol=0.0, dtype=np.float64, **hyper)
    t32 = O.cer_train_cg_estep(U0, V0, E0, m.feat, *likes, max_iter=O.E2E['iters'], tol=0.0, dtype=np.float32, **hyper)
    return m, likes, t64, t32


def test_cer_with_the_cg_estep_trains_as_the_oracle(golden_dir):
    """fue, fie (its four cold rows among them), E and every iteration's loss within F of cer_train_cg_estep"""
    m, likes, (U64, V64, E64, l64), (U32, V32, E32, l32) = _trained(golden_dir)
    assert len(m.losses) == O.E2E['iters'] == len(l64)
    assert all(later < earlier for earlier, later in zip([np.exp(50)] + m.losses, m.losses)), m.losses
    assert m.fue.dtype == m.fie.dtype == m.E.dtype == np.float32 and m.E.shape == (O.E2E['d'], O.E2E['k'])
    cold = [j for j, x in enumerate(likes[1]) if len(x) == 0]
    assert len(cold) == 4
    for name, got, x64, x32 in (('fue', m.fue, U64, U32), ('fie', m.fie, V64, V32), ('cold fie', m.fie[cold], V64[cold], V32[cold]), ('E', m.E, E64, E32)) + \
            tuple(('loss %d' % i, np.asarray([m.losses[i]]), np.asarray([l64[i]]), np.asarray([l32[i]])) for i in range(len(l64))):
        ratio, err, e32 = _ratio(np.asarray(got, dtype=np.float64), np.asarray(x64), np.asarray(x32, dtype=np.float64))
        print('K26 CER estep=cg %s: err %.3g e32 %.3g ratio %.3g' % (name, err, e32, ratio))
        assert ratio <= F, (name, err, e32)
    # the method: 8 steps per iteration, warm-started, end where the direct E-step ends (float64 against float64)
    direct = O.cer_train(*O.e2e_start(m.n_users, m.n_items), np.asarray(m.feat.todense()), *likes, a=m.a, b=m.b, lu=m.lu, lv=m.lv, le=m.le,
                         max_iter=O.E2E['iters'], tol=0.0)[3]
    print('K26 CER float64 losses: direct E-step %r, %d steps of CG %r' % (direct[-1], E_STEPS, l64[-1]))
    assert abs(l64[-1] - direct[-1]) <= 1e-3 * direct[-1]
    # embed_items of a sparse matrix is the product's chain; of the same rows dense, the host path as before
    Fc = m.feat[cold]
    got = m.embed_items(Fc)
    assert got.dtype == np.float32 and got.shape == (4, m.k)
    np.testing.assert_array_equal(_bits(got), _bits(O.spmm(Fc, m.E, dtype=np.float32)))
    np.testing.assert_array_equal(_bits(got), _bits(m.fie[cold]))
    dense = m.embed_items(Fc.toarray())
    np.testing.assert_array_equal(_bits(dense), _bits((Fc.toarray().astype(np.float64) @ m.E.astype(np.float64)).astype(np.float32)))


def test_cer_with_the_cg_estep_model_directory(golden_dir, tmp_path):
    import evaluate as E
    import train_als
    from oracle import ref_np as R
    m = _trained(golden_dir)[0]
    out = str(tmp_path / 'cer')
    m.export_embeddings(out)
    assert sorted(os.listdir(out)) == ['final-E.dat', 'final-U.dat', 'final-V.dat']
    got = E.main(['-d', _g2(golden_dir), '-m', out, '-sl', 'im'])
    exp = R.evaluate_cli(_g2(golden_dir), out, scenarios=('im',))
    assert len(got) == len(exp) == 1 and got[0].startswith('im,')
    assert [float(x) for x in got[0].split(',')[1:]] == [float(x) for x in exp[0].split(',')[1:]]
    # the driver, the content through a sparse pickle as load_content_data reads it
    pkl = str(tmp_path / 'meta.pkl')
    with open(pkl, 'wb') as fh:
        pickle.dump(ss.coo_matrix(O.e2e_features(m.n_items)), fh)
    out2 = str(tmp_path / 'cer2')
    hy = ['--lu', str(m.lu), '--lv', str(m.lv), '--le', str(m.le), '-k', str(m.k), '--seed', str(O.E2E['seed'])]
    model = train_als.main(['-d', _g2(golden_dir), '-o', out2, '--model', 'cer', '--estep', 'cg', '--e-steps', str(E_STEPS), '--content', pkl, '--dim', '24',
                            '--iters', '6', '--tol', '0'] + hy)
    assert type(model).__name__ == 'CER' and model.estep == 'cg' and sorted(os.listdir(out2)) == ['final-E.dat', 'final-U.dat', 'final-V.dat']
    assert ss.isspmatrix_csr(model.feat)
    np.testing.assert_allclose(model.fie, m.fie, rtol=1e-4, atol=1e-6)           # the same seed, the same features, the same run
    np.testing.assert_allclose(model.E, m.E, rtol=1e-4, atol=1e-6)
    np.testing.assert_allclose(model.losses, m.losses, rtol=1e-6)
    # a warm start from the directory
    fresh = _model(golden_dir)
    fresh.feat = O.e2e_features(fresh.n_items)                                  # assigned directly, dense
    fresh.train(max_iter=2, tol=0.0, model_path=out, verbose=False)
    assert len(fresh.losses) == 2 and np.isfinite(fresh.losses).all() and fresh.losses[1] < fresh.losses[0]


# ---- g. the width the dense path cannot hold ------------------------------------------------------------------------------------------------
def test_a_width_of_200000_trains_under_cg_and_not_under_cholesky(golden_dir):
    wide = dict(k=O.WIDE['k'], d=O.WIDE['d'])
    dense = _model(golden_dir, estep='cholesky', **wide)
    dense.feat = O.wide_features(dense.n_items)
    with pytest.raises(ValueError, match=r'8 \(d\^2 \+ n_items d\)'):           # 320 GB of FF
        dense.train(max_iter=2, tol=0.0, verbose=False)
    m = _model(golden_dir, **wide)
    m.feat = O.wide_features(m.n_items)
    m.train(max_iter=2, tol=0.0, verbose=False)
    print('K26 CER d=200000 losses: %r' % (m.losses,))
    assert len(m.losses) == 2 and np.isfinite(m.losses).all() and m.losses[1] < m.losses[0]
    assert m.E.shape == (O.WIDE['d'], O.WIDE['k']) and np.isfinite(m.E).all() and np.isfinite(m.fie).all()
