"""K23 on the GPU (csrc/fusion_svm.hip; svmfusion.py, fuse.py --method s): the sums of a Newton pass bit for bit against the oracle on
inputs whose arithmetic is exact, bitwise repeatable and independent of the chunking, within the bound of the sum length on generic
inputs; learn_svm against the oracle's Newton on the oracle's own features; the command line on tests/golden/g4; the refusals."""
import functools
import json
import os
import shutil
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _fusion_oracle as FO
import _svm_oracle as O
from oracle import plan_np as P
from oracle import ref_np as R

pytestmark = pytest.mark.gpu

SLAB = 4096                                  # TKR_FUSION_SVM_SLAB (asserted below)
SIZES = (1, 2, 63, 64, 65, SLAB - 1, SLAB, SLAB + 1, 3 * SLAB + 5)
N_MAX = SIZES[-1]


def _dev(a, dtype=None):
    return torch.from_numpy(np.array(a, dtype=dtype, order='C')).to('cuda')              # a copy: the shared references stay read-only


def _pack(S, r, q, count):
    """the oracle's sums in the layout of the result: the upper triangle row by row | r | q | count as int64"""
    out = np.concatenate([S[np.triu_indices(len(S))], r, [q], [0.0]])
    out[-1:] = np.array([count], dtype=np.int64).view(np.float64)
    return out


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _run(D, W, first_row=0, **kw):
    import tkr_hip
    return tkr_hip.fusion_svm_sums(_dev(D, np.float32), _dev(W, np.float64), first_row, **kw).cpu().numpy()


@functools.lru_cache(maxsize=None)
def _exact_case(M, first_row):
    """D in eighths of small integers, W in eighths with W[0] = 1, and every fifth row moved exactly onto the hinge through its first
    entry (a multiple of 1 / 64): every product and every sum below is exact in fp64, in any order"""
    rng = np.random.Generator(np.random.PCG64(100 * M + first_row % 7))
    D = rng.integers(-12, 13, (N_MAX, M)).astype(np.float64) / 8
    W = rng.integers(-6, 7, M + 1).astype(np.float64) / 8
    W[0] = 1.0
    y = np.where((first_row + np.arange(N_MAX)) % 2 == 0, 1.0, -1.0)
    on = np.arange(N_MAX) % 5 == 0
    D[on, 0] = (1.0 - y * W[M] - D[:, 1:] @ W[1:M])[on]
    D32 = D.astype(np.float32)
    assert np.array_equal(D32.astype(np.float64), D)
    D32.setflags(write=False)
    W.setflags(write=False)
    return D32, W, on


@pytest.mark.parametrize('first_row', [0, 1, SLAB + 1])
@pytest.mark.parametrize('M', [1, 3, 4, 16])
def test_exact_sums_equal_the_oracle_bit_for_bit(M, first_row):
    import tkr_hip
    assert tkr_hip.FUSION_SVM_SLAB == SLAB
    D, W, on = _exact_case(M, first_row)
    z = O.margins(O.rows(D, first_row), W)
    assert np.all(z[on] == 1.0) and (z < 1.0).sum() > N_MAX // 4 and (z > 1.0).sum() > N_MAX // 20
    for N in SIZES:
        want = O.sums(D[:N], first_row, W)
        got = _run(D[:N], W, first_row)
        assert want[3] == int((z[:N] < 1.0).sum())                    # rows exactly on the hinge are not among the active
        np.testing.assert_array_equal(_bits(got), _bits(_pack(*want)), err_msg='N = %d' % N)
    # every row active (W = 0: r = sum x~, q = N) and no row active (first entries >= 1, W = (4, 0, ...): all sums zero)
    N = 3 * SLAB + 5
    S, r, q, count = tkr_hip.fusion_svm_unpack(_run(D, np.zeros(M + 1), first_row), M)
    X = O.rows(D, first_row)
    assert count == N and q == float(N) and np.array_equal(r, X.sum(axis=0)) and np.array_equal(S, X.T @ X)
    Dp = np.array(D)
    Dp[:, 0] = np.abs(Dp[:, 0]) + 1
    got = _run(Dp, np.concatenate([[4.0], np.zeros(M)]), first_row)
    assert not got.view(np.uint64).any()


@functools.lru_cache(maxsize=None)
def _generic_case(M):
    rng = np.random.Generator(np.random.PCG64(7 + M))
    D = rng.standard_normal((N_MAX, M)).astype(np.float32)
    W = rng.standard_normal(M + 1) * 0.3
    D.setflags(write=False)
    W.setflags(write=False)
    return D, W


@pytest.mark.parametrize('M', [3, 16])
def test_two_runs_and_runs_in_chunks_of_whole_slabs_give_the_same_bits(M):
    import tkr_hip
    D, W = _generic_case(M)
    Dd, Wd = _dev(D), _dev(W)
    whole = tkr_hip.fusion_svm_sums(Dd, Wd).cpu().numpy()
    assert tkr_hip.fusion_svm_unpack(whole, M)[3] > N_MAX // 4
    np.testing.assert_array_equal(_bits(tkr_hip.fusion_svm_sums(Dd, Wd).cpu().numpy()), _bits(whole))
    for per in (1, 2):
        partial = torch.empty(tkr_hip.fusion_svm_partial_bytes(N_MAX, M) // 8, dtype=torch.float64, device='cuda')
        status = torch.empty(1, dtype=torch.int64, device='cuda')
        out = None
        for c0 in range(0, N_MAX, per * SLAB):
            n = min(per * SLAB, N_MAX - c0)
            out = tkr_hip.fusion_svm_sums(Dd[c0:c0 + n], Wd, c0, partial=partial, slab_offset=c0 // SLAB, reduce=c0 + n >= N_MAX, status=status)
        np.testing.assert_array_equal(_bits(out.cpu().numpy()), _bits(whole), err_msg='%d slabs per call' % per)
    # ... and a D that is not 16-byte aligned takes the other load path to the same bits
    if M % 4 == 0:
        shifted = torch.empty(N_MAX * M + 1, dtype=torch.float32, device='cuda')[1:].view(N_MAX, M)
        shifted.copy_(Dd)
        assert shifted.data_ptr() % 16 == 4
        np.testing.assert_array_equal(_bits(tkr_hip.fusion_svm_sums(shifted, Wd).cpu().numpy()), _bits(whole))


@pytest.mark.parametrize('M', [3, 16])
def test_generic_sums_within_the_bound_of_the_sum_length(M):
    """every entry is a sum of at most N terms, each one rounding: |got - want| <= N 2^-53 sum|terms| whatever the order (the oracle
    sums forwards without fma, the kernel through its tree with fma).  Measured on MI355X: DESIGN.md section 4 K23."""
    import tkr_hip
    D, W = _generic_case(M)
    N = N_MAX
    want = O.sums(D, 0, W)
    got = tkr_hip.fusion_svm_unpack(_run(D, W), M)
    assert got[3] == want[3]
    X = O.rows(D, 0)
    a = 1.0 - O.margins(X, W)
    Xa, aa = np.abs(X[a > 0]), a[a > 0]
    eps = N * 2.0 ** -53
    worst = 0.0
    for name, g, w, mag in (('S', got[0], want[0], Xa.T @ Xa), ('r', got[1], want[1], aa @ Xa), ('q', got[2], want[2], aa @ aa)):
        ratio = float(np.max(np.abs(np.asarray(g) - np.asarray(w)) / (eps * np.asarray(mag))))
        print('M = %d, %s: worst |got - want| / (N 2^-53 sum|terms|) = %.3g' % (M, name, ratio))
        worst = max(worst, ratio)
        assert np.all(np.abs(np.asarray(g) - np.asarray(w)) <= eps * np.asarray(mag)), name
    assert worst <= 1.0


# ---- learn_svm ----------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _g2(golden_dir):
    d = os.path.join(golden_dir, 'g2')
    T = R.load_training(os.path.join(d, 'uid'), os.path.join(d, 'vid'), os.path.join(d, 'f0tr.txt'))
    rng = np.random.Generator(np.random.PCG64(23))
    models = tuple(((rng.standard_normal((T['n_users'], 8)) * 0.4).astype(np.float32), (rng.standard_normal((T['n_items'], 8)) * 0.4).astype(np.float32),
                    (rng.standard_normal(T['n_items']) * 0.3).astype(np.float32) if m == 1 else None) for m in range(3))
    row_ptr, pos, srt = P.build_csr(T['tr_data'], T['n_users'])
    return T, models, (row_ptr, pos, srt), FO.chain_scores(models)


def _csr(T):
    from single import _engine
    return _engine.TrainingCSR(T['tr_data'], T['tr_users'], T['n_users'], torch.device('cuda', torch.cuda.current_device()))


def _learn_against_the_oracle(T, csr_np, models, scores, n_samples, what):
    """Allowed distance: 16 x the largest distance between the oracle's runs with its row sums taken forwards, backwards and pairwise,
    and at least 64 N 2^-53 cond(H) max|w~| (sums of N terms, carried through the solve).  Measured: DESIGN.md section 4 K23."""
    import svmfusion
    row_ptr, pos, srt = csr_np
    seed, C_ = 5, 0.01
    u, i, j = P.sample_triplets(T['tr_users'], row_ptr, pos, srt, T['n_items'], seed, 0, n_samples)
    D = FO.features(scores, u, i, j)
    runs = [O.newton(D, C_, order=order) for order in ('forward', 'backward', 'pairwise')]
    ref = runs[0]
    assert all(r['converged'] for r in runs)
    spread = max(float(np.abs(a['w'] - b['w']).max()) for a in runs for b in runs)
    floor = 64 * n_samples * 2.0 ** -53 * np.linalg.cond(ref['H']) * float(np.abs(ref['w']).max())
    W, info = svmfusion.learn_svm(models, _csr(T), T['n_items'], n_samples=n_samples, C=C_, seed=seed, want_info=True)
    got = np.concatenate([info['weights'], [info['intercept']]])
    dist = float(np.abs(got - ref['w']).max())
    print('learn_svm %s, N = %d, M = %d: %d Newton steps (oracle %d), %d active, max|g| = %.3g, distance to the oracle %.3g, allowed '
          'max(16 x %.3g, %.3g), max|w~| = %.3g' % (what, n_samples, len(models), info['iterations'], ref['iterations'], info['active'],
                                                    info['grad'], dist, spread, floor, np.abs(ref['w']).max()))
    assert dist <= max(16 * spread, floor)
    assert info['converged'] and info['iterations'] == ref['iterations'] and info['active'] == ref['active']
    assert abs(info['objective'] - ref['objective']) <= 64 * n_samples * 2.0 ** -53 * max(ref['objective'], 1.0)
    assert W.dtype == np.float32 and np.array_equal(W, info['weights'].astype(np.float32))
    assert np.array_equal(svmfusion.learn_svm(models, _csr(T), T['n_items'], n_samples=n_samples, C=C_, seed=seed), W)
    return info


@pytest.mark.parametrize('n_models', [2, 3])
@pytest.mark.parametrize('n_samples', [1, 7, 2 * SLAB + 3])
def test_learn_svm_against_the_oracles_newton(golden_dir, n_samples, n_models):
    T, models, csr_np, scores = _g2(golden_dir)
    _learn_against_the_oracle(T, csr_np, list(models[:n_models]), scores[:n_models], n_samples, 'random models')


def test_learn_svm_with_a_model_that_fits_the_likes(golden_dir):
    """random models carry no signal: their weights stay small and every row stays active, one Newton step.  A model whose user rows
    are three times the mean of the liked items' rows scores the likes high: its weight grows until half the rows leave the hinge, and
    the iteration takes several steps over a changing active set"""
    T, models, csr_np, _ = _g2(golden_dir)
    V = models[0][1]
    U = np.zeros_like(models[0][0])
    for u, items in T['tr_data'].items():
        U[u] = 3 * V[items].mean(axis=0)
    models = [(U, V, None), models[1]]
    N = 2 * SLAB + 3
    info = _learn_against_the_oracle(T, csr_np, models, FO.chain_scores(models), N, 'a model that fits')
    assert info['iterations'] >= 3 and N // 4 < info['active'] < 3 * N // 4 and info['weights'][0] > 0.5


def test_learn_svm_does_not_depend_on_the_chunking(golden_dir):
    import svmfusion
    T, models, _, _ = _g2(golden_dir)
    kw = dict(n_samples=2 * SLAB + 3, C=0.01, seed=5, want_info=True)
    _, kept = svmfusion.learn_svm(list(models), _csr(T), T['n_items'], **kw)
    for chunk_bytes in (1, 2 * SLAB * 3 * 4):                        # the features regenerated every pass, one and two slabs at a time
        _, again = svmfusion.learn_svm(list(models), _csr(T), T['n_items'], chunk_bytes=chunk_bytes, **kw)
        for key in ('weights', 'intercept', 'iterations', 'grad', 'active', 'objective'):
            assert np.array_equal(np.asarray(kept[key]), np.asarray(again[key])), (chunk_bytes, key)


# ---- the command line on tests/golden/g4 -------------------------------------------------------------------------------------------
def test_fuse_cli_learns_svm_weights(golden_dir, tmp_path, capsys):
    import fuse
    import svmfusion
    import textio
    data, A, B, out = str(tmp_path / 'data'), str(tmp_path / 'A'), str(tmp_path / 'B'), str(tmp_path / 'fused')
    shutil.copytree(os.path.join(golden_dir, 'g4', 'data'), data)
    shutil.copytree(os.path.join(golden_dir, 'g4', 'model'), A)
    os.mkdir(B)
    rng = np.random.Generator(np.random.PCG64(44))
    textio.write_matrix(os.path.join(B, 'final-U.dat'), (rng.standard_normal((160, 5)) * 0.3).astype(np.float32), where='host')
    textio.write_matrix(os.path.join(B, 'final-V.dat'), (rng.standard_normal((120, 5)) * 0.3).astype(np.float32), where='host')
    textio.write_matrix(os.path.join(B, 'final-B.dat'), (rng.standard_normal((120, 1)) * 0.3).astype(np.float32), where='host')
    uids, vids = R.read_id_list(os.path.join(data, 'uid')), R.read_id_list(os.path.join(data, 'vid'))
    models = [(R.read_embed_text(os.path.join(A, 'final-U.dat'), uids), R.read_embed_text(os.path.join(A, 'final-V.dat'), vids), None),
              (R.read_embed_text(os.path.join(B, 'final-U.dat'), uids), R.read_embed_text(os.path.join(B, 'final-V.dat'), vids),
               R.read_embed_text(os.path.join(B, 'final-B.dat'), vids).reshape(-1))]
    w = fuse.main(['-d', data, '-m', A, B, '-o', out, '--method', 's', '--samples', '2000', '--seed', '3'])
    assert [float(x) for x in capsys.readouterr().out.strip().splitlines()[-1].split()] == [float('%.9g' % x) for x in w]
    T = R.load_training(os.path.join(data, 'uid'), os.path.join(data, 'vid'), os.path.join(data, 'f0tr.txt'))
    W, info = svmfusion.learn_svm(models, _csr(T), T['n_items'], n_samples=2000, C=0.01, seed=3, want_info=True)
    assert w.dtype == np.float32 and np.array_equal(w, W) and np.abs(w).max() > 0
    meta = json.load(open(os.path.join(out, 'fusion.json')))
    assert meta['method'] == 's' and meta['C'] == 0.01 and meta['samples'] == 2000 and meta['seed'] == 3
    assert meta['intercept'] == info['intercept'] and meta['iterations'] == info['iterations'] >= 1 and meta['grad_norm'] == info['grad']
    assert meta['grad_norm'] <= 1e-12 * max(1.0, 0.01 * 2000) and meta['weights'] == [float(x) for x in w]
    assert meta['active'] == info['active'] and meta['objective'] == info['objective']
    assert not os.path.exists(os.path.join(out, 'final-W.dat')) and not os.path.exists(os.path.join(out, 'final-B.dat'))
    # the fused directory read back as evaluate.py reads any model: U~ . V~ = sum_m w_m s_m, up to the six decimals of '%f'
    Uf, Vf = R.read_embed_text(os.path.join(out, 'final-U.dat'), uids), R.read_embed_text(os.path.join(out, 'final-V.dat'), vids)
    assert Uf.shape == (160, 8 + 5 + 1) and Vf.shape == (120, 14)
    want = FO.weighted_sum(models, w)
    for u, i in ((0, 0), (7, 119), (159, 3), (80, 60), (33, 77)):
        got = float(Uf[u].astype(np.float64) @ Vf[i].astype(np.float64))
        assert abs(got - want[u, i]) <= 5e-7 * float(np.abs(Uf[u]).sum() + np.abs(Vf[i]).sum()) + 1e-6, (u, i)
    import evaluate
    assert evaluate.main(['-d', data, '-m', out, '-sl', 'im', 'om']) == R.evaluate_cli(data, out, scenarios=('im', 'om'))


# ---- refusals -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('M,first_row', [(3, 0), (16, SLAB + 1)])
def test_a_row_that_is_not_finite_is_named_and_nothing_is_written(M, first_row):
    import tkr_hip
    D, W = _generic_case(M)
    D = np.array(D[:SLAB + 70])
    D[SLAB + 9, M - 1] = np.nan
    D[SLAB + 40, 0] = np.inf                                          # the smallest such row is the one that is named
    out = torch.full((tkr_hip.fusion_svm_words(M),), 7.0, dtype=torch.float64, device='cuda')
    with pytest.raises(tkr_hip.TkrError, match='row %d of the features' % (first_row + SLAB + 9)):
        tkr_hip.fusion_svm_sums(_dev(D), _dev(W), first_row, out=out)
    assert torch.all(out == 7.0)
    status = torch.empty(1, dtype=torch.int64, device='cuda')
    tkr_hip.fusion_svm_sums(_dev(D), _dev(W), first_row, out=out, status=status, check=False)
    assert int(status.item()) == first_row + SLAB + 9 and torch.all(out == 7.0)
    D[SLAB + 9, M - 1] = 0.0
    D[SLAB + 40, 0] = 0.0
    tkr_hip.fusion_svm_sums(_dev(D), _dev(W), first_row, out=out, status=status)
    assert int(status.item()) == -1 and not torch.any(out == 7.0)


def test_host_tensors_and_wrong_shapes_are_refused_without_a_launch():
    import tkr_hip
    D, W = _generic_case(3)
    Dd, Wd = _dev(D[:10]), _dev(W)
    with pytest.raises(tkr_hip.TkrError, match='must live on the GPU'):
        tkr_hip.fusion_svm_sums(torch.from_numpy(np.array(D[:10])), Wd)
    with pytest.raises(tkr_hip.TkrError, match='one GPU'):
        tkr_hip.fusion_svm_sums(Dd, torch.from_numpy(np.array(W)))
    with pytest.raises(tkr_hip.TkrError, match='W must be torch.float64'):
        tkr_hip.fusion_svm_sums(Dd, Wd.float())
    with pytest.raises(tkr_hip.TkrError, match='W must hold 4 values'):
        tkr_hip.fusion_svm_sums(Dd, Wd[:3])
    with pytest.raises(tkr_hip.TkrError, match='partial must hold at least 16 values'):
        tkr_hip.fusion_svm_sums(Dd, Wd, partial=torch.empty(15, dtype=torch.float64, device='cuda'))
    with pytest.raises(tkr_hip.TkrError, match='out must hold 16 values'):
        tkr_hip.fusion_svm_sums(Dd, Wd, out=torch.empty(17, dtype=torch.float64, device='cuda'))
    with pytest.raises(tkr_hip.TkrError, match='status must be one torch.int64 word'):
        tkr_hip.fusion_svm_sums(Dd, Wd, status=torch.empty(1, dtype=torch.int32, device='cuda'))
