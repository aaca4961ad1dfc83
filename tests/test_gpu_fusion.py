"""K16 on the GPU (csrc/fusion.hip; fusion.py, fuse.py): the features bit for bit against the oracle and against K12's own scores, the
one-workgroup SGD and the per-user weights within the project's measured-tolerance rule of the float64 oracle, bitwise repeatable and
independent of the chunking, and the command line on tests/golden/g4."""
import functools
import json
import os
import shutil
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _fusion_oracle as O
from oracle import plan_np as P
from oracle import ref_np as R

pytestmark = pytest.mark.gpu

N_USERS, N_ITEMS = 300, 200
FIRST = 2 ** 32 - 1000                       # the counter carries into its high word inside the call
KS16 = (8, 50, 128, 3, 24, 1, 64, 17, 8, 50, 2, 40, 128, 5, 16, 33)
GENERIC_KS = (8, 50, 128, 136, 17)           # test_features_generic_inputs_equal_the_difference_of_k12_scores


def _dev(a, dtype=None):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).to('cuda')


def _models_dev(models):
    return [(_dev(U), _dev(V), _dev(b)) for U, V, b in models]


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


@functools.lru_cache(maxsize=None)
def _training(n_users=N_USERS, n_items=N_ITEMS):
    """users without a row (every 7th), one user whose row is 199 of the 200 items (the cyclic scan of the negative's draw), the
    rest 1 .. 30 likes; tr_users in a shuffled first-appearance order"""
    rng = np.random.Generator(np.random.PCG64(77))
    tr = {}
    for u in rng.permutation(n_users):
        u = int(u)
        if u % 7 == 3:
            continue
        n = n_items - 1 if u == 5 else int(rng.integers(1, 31))
        tr[u] = [int(c) for c in rng.choice(n_items, n, replace=False)]
    row_ptr, pos, srt = P.build_csr(tr, n_users)
    return tr, list(tr.keys()), row_ptr, pos, srt


def _csr(n_users=N_USERS):
    from single import _engine
    tr, tr_users, _, _, _ = _training()
    return _engine.TrainingCSR(tr, tr_users, n_users, torch.device('cuda', torch.cuda.current_device()))


def _exact_models(ks, biased, n_users=N_USERS, n_items=N_ITEMS, seed=1):
    """entries m * 2^-6, biases m * 2^-12: every product and partial sum is exact in fp32"""
    rng = np.random.Generator(np.random.PCG64(seed))
    return [(rng.integers(-3, 4, (n_users, k)).astype(np.float32) / 64, rng.integers(-3, 4, (n_items, k)).astype(np.float32) / 64,
             (rng.integers(-2, 3, n_items).astype(np.float32) / 4096) if q in biased else None) for q, k in enumerate(ks)]


@functools.lru_cache(maxsize=None)
def _generic_models(M=3, n_users=N_USERS, n_items=N_ITEMS, seed=2, ks=KS16):
    """N(0, 0.1^2) tables rounded like '%f'; k = (8, 50, 128, ...), model 1 with a bias"""
    rng = np.random.Generator(np.random.PCG64(seed))
    return tuple((np.round(rng.standard_normal((n_users, k)) * 0.1, 6).astype(np.float32),
                  np.round(rng.standard_normal((n_items, k)) * 0.1, 6).astype(np.float32),
                  np.round(rng.standard_normal(n_items) * 0.1, 6).astype(np.float32) if q % 3 == 1 else None) for q, k in enumerate(ks[:M]))


@functools.lru_cache(maxsize=None)
def _oracle_D16():
    """the oracle's features of 40,037 triplets under 16 generic models, computed once and never written to"""
    _, tr_users, row_ptr, pos, srt = _training()
    u, i, j = P.sample_triplets(tr_users, row_ptr, pos, srt, N_ITEMS, 11, 0, 40037)
    D = O.features(O.chain_scores(_generic_models(16)), u, i, j)
    D.setflags(write=False)
    return D


# ---- features ----------------------------------------------------------------------------------------------------------------------
def test_features_exact_inputs_equal_the_oracle_bit_for_bit():
    import tkr_hip
    _, tr_users, row_ptr, pos, srt = _training()
    models = _exact_models((8, 50, 128), biased=(1,))
    count = 4133                                                      # no multiple of 64 or 256
    D, trip = tkr_hip.fusion_features(_models_dev(models), _csr(), N_ITEMS, 9, FIRST, count, want_triplets=True)
    u, i, j = P.sample_triplets(tr_users, row_ptr, pos, srt, N_ITEMS, 9, FIRST, count)
    assert FIRST + count > 2 ** 32 and (u == 5).any()
    np.testing.assert_array_equal(trip.cpu().numpy(), np.stack([u, i, j], axis=1))
    want = O.features(O.chain_scores(models), u, i, j)
    assert D.shape == (count, 3) and D.dtype == torch.float32
    np.testing.assert_array_equal(_bits(D.cpu().numpy()), _bits(want))
    assert len(np.unique(want)) > 50                                  # (the exact tables do not make the check trivial)


@pytest.mark.parametrize('M', [1, 16])
def test_features_one_and_sixteen_models(M):
    import tkr_hip
    _, tr_users, row_ptr, pos, srt = _training()
    models = _exact_models(KS16[:M], biased=(0, 3, 15), seed=3 + M)
    D, trip = tkr_hip.fusion_features(_models_dev(models), _csr(), N_ITEMS, 4, 123, 65, want_triplets=True)
    u, i, j = P.sample_triplets(tr_users, row_ptr, pos, srt, N_ITEMS, 4, 123, 65)
    np.testing.assert_array_equal(trip.cpu().numpy(), np.stack([u, i, j], axis=1))
    np.testing.assert_array_equal(_bits(D.cpu().numpy()), _bits(O.features(O.chain_scores(models), u, i, j)))
    only_D = tkr_hip.fusion_features(_models_dev(models), _csr(), N_ITEMS, 4, 123, 65)            # trip_out = NULL
    assert torch.equal(only_D, D)


def test_features_generic_inputs_equal_the_difference_of_k12_scores():
    """K12 (tkr_hip.rank_candidates, the parent's kernel) scores the two-column rows {i, j}: D is fl(a - b) of ITS bits.  Widths 8, 50
    and 128 as everywhere here, then 136 (aligned: 17 float4 steps, a remainder behind every unroll factor of the chain) and 17 (odd:
    one block of 8 paired steps, then the odd factor)"""
    import tkr_hip
    models = _generic_models(5, ks=GENERIC_KS)
    md = _models_dev(models)
    count = 4133
    D, trip = tkr_hip.fusion_features(md, _csr(), N_ITEMS, 21, FIRST, count, want_triplets=True)
    trip = trip.cpu().numpy()
    u, i, j = trip[:, 0], trip[:, 1], trip[:, 2]
    assert np.all(i != j)
    lo, hi = np.minimum(i, j), np.maximum(i, j)
    ptr = _dev(2 * np.arange(count + 1, dtype=np.int64))
    cols = _dev(np.stack([lo, hi], axis=1).reshape(-1), np.int32)
    for m, (U, V, b) in enumerate(md):
        s, _ = tkr_hip.rank_candidates(U, V, ptr, cols, bias=b, user_idx=_dev(u, np.int32))
        s = s.cpu().numpy().reshape(count, 2)
        a, c = np.where(i < j, s[:, 0], s[:, 1]), np.where(i < j, s[:, 1], s[:, 0])
        np.testing.assert_array_equal(_bits(D[:, m].cpu().numpy()), _bits((a - c).astype(np.float32)), err_msg='model %d' % m)
    np.testing.assert_array_equal(_bits(D.cpu().numpy()), _bits(O.features(O.chain_scores(models), u, i, j)))      # and the oracle's


# ---- SGD ---------------------------------------------------------------------------------------------------------------------------
LR, LAM = 1e-2, 0.0025
SGD_CASES = [(1, 5), (100, 301), (1024, 3 * 1024), (1025, 3 * 1025 + 1), (10000, 40037)]


def _within(name, got, x64, x32):
    d = float(np.abs(x32.astype(np.float64) - x64).max()) if x64.size else 0.0
    dist = np.abs(np.asarray(got, dtype=np.float64) - x64)
    bound = O.bound(x64, d)
    print('%s: d(fp32 oracle, fp64 oracle) = %.3g, kernel to fp64 = %.3g, max |x| = %.3g' %
          (name, d, float(dist.max()) if dist.size else 0.0, float(np.abs(x64).max()) if x64.size else 0.0))
    assert np.all(dist <= bound), (name, float((dist - bound).max()))


@pytest.mark.parametrize('B,n', SGD_CASES)
@pytest.mark.parametrize('M', [1, 3, 16])
def test_sgd_against_the_float64_oracle_split_and_repeat(M, B, n):
    import tkr_hip
    D = np.array(_oracle_D16()[:n, :M], order='C')                   # a copy: the shared reference stays as it is
    nb = O.n_batches(n, B)
    assert nb == {(1, 5): 4, (100, 301): 3, (1024, 3072): 2, (1025, 3076): 3, (10000, 40037): 4}[(B, n)]
    W64, c64 = O.sgd(D, B, nb, LR, LAM, dtype=np.float64)
    W32, c32 = O.sgd(D, B, nb, LR, LAM, dtype=np.float32)
    Dd = _dev(D)
    W, loss = tkr_hip.fusion_sgd(Dd, B, nb, LR, LAM, torch.zeros(M, device='cuda'), want_loss=True)
    W, loss = W.cpu().numpy(), loss.cpu().numpy()
    _within('W (M = %d, B = %d)' % (M, B), W, W64, W32)
    _within('loss (M = %d, B = %d)' % (M, B), loss, c64, c32)
    assert np.abs(W64).max() > 0
    # a second identical call: identical bits; without the loss: the same W
    W2, loss2 = tkr_hip.fusion_sgd(Dd, B, nb, LR, LAM, torch.zeros(M, device='cuda'), want_loss=True)
    np.testing.assert_array_equal(_bits(W2.cpu().numpy()), _bits(W))
    np.testing.assert_array_equal(_bits(loss2.cpu().numpy()), _bits(loss))
    W3 = tkr_hip.fusion_sgd(Dd, B, nb, LR, LAM, torch.zeros(M, device='cuda'))
    np.testing.assert_array_equal(_bits(W3.cpu().numpy()), _bits(W))
    # one call over all batches = two calls over the halves with W carried across
    h = nb // 2
    Wa = torch.zeros(M, device='cuda')
    _, la = tkr_hip.fusion_sgd(Dd, B, h, LR, LAM, Wa, want_loss=True)
    _, lb = tkr_hip.fusion_sgd(Dd[h * B:], B, nb - h, LR, LAM, Wa, want_loss=True)
    np.testing.assert_array_equal(_bits(Wa.cpu().numpy()), _bits(W))
    np.testing.assert_array_equal(_bits(torch.cat([la, lb]).cpu().numpy()), _bits(loss))


# ---- learn_pairwise ----------------------------------------------------------------------------------------------------------------
def test_learn_pairwise_end_to_end_and_chunking():
    import fusion
    _, tr_users, row_ptr, pos, srt = _training()
    models = list(_generic_models(3))
    kw = dict(n_samples=20000, batch_size=1000, lr=LR, lambda_w=LAM, seed=5)
    W, loss = fusion.learn_pairwise(models, _csr(), N_ITEMS, want_loss=True, **kw)
    assert W.shape == (3,) and W.dtype == np.float32 and loss.shape == (19,)
    W64, c64, _ = O.learn_pairwise(models, tr_users, row_ptr, pos, srt, N_ITEMS, 20000, 1000, LR, LAM, 5, dtype=np.float64)
    W32, c32, _ = O.learn_pairwise(models, tr_users, row_ptr, pos, srt, N_ITEMS, 20000, 1000, LR, LAM, 5, dtype=np.float32)
    _within('learn_pairwise W', W, W64, W32)
    _within('learn_pairwise loss', loss, c64, c32)
    Wc, lossc = fusion.learn_pairwise(models, _csr(), N_ITEMS, want_loss=True, chunk_bytes=1, **kw)        # one batch per chunk
    np.testing.assert_array_equal(_bits(Wc), _bits(W))
    np.testing.assert_array_equal(_bits(lossc), _bits(loss))
    np.testing.assert_array_equal(_bits(fusion.learn_pairwise(models, _csr(), N_ITEMS, **kw)), _bits(W))
    # batch_size above the number of training pairs is cut to it (ranking_fusion.py:40-42)
    Wb, lossb = fusion.learn_pairwise(models, _csr(), N_ITEMS, n_samples=3 * len(pos) + 1, batch_size=10 ** 6, lr=LR, lambda_w=LAM, seed=5,
                                      want_loss=True)
    W64b, c64b, _ = O.learn_pairwise(models, tr_users, row_ptr, pos, srt, N_ITEMS, 3 * len(pos) + 1, 10 ** 6, LR, LAM, 5)
    W32b, c32b, _ = O.learn_pairwise(models, tr_users, row_ptr, pos, srt, N_ITEMS, 3 * len(pos) + 1, 10 ** 6, LR, LAM, 5, dtype=np.float32)
    assert lossb.shape == (3,)
    _within('cut batch W', Wb, W64b, W32b)
    _within('cut batch loss', lossb, c64b, c32b)


# ---- per-user weights --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('n_items,lengths', [(200, (0, 1, 63, 64, 65)), (600, (0, 1, 63, 64, 65, 500))])
def test_user_weights_against_the_float64_oracle(n_items, lengths):
    import fusion
    import tkr_hip
    n_users = 70
    rng = np.random.Generator(np.random.PCG64(n_items))
    models = list(_generic_models(3, n_users, n_items, seed=8))
    rows = [np.sort(rng.choice(n_items, lengths[u % len(lengths)], replace=False)).astype(np.int32) for u in range(n_users)]
    ptr = np.zeros(n_users + 1, np.int64)
    np.cumsum([len(r) for r in rows], out=ptr[1:])
    cols = np.concatenate(rows)
    scores = O.chain_scores(models)
    r64, w64 = O.user_weights(scores, ptr, cols, dtype=np.float64)
    r32, w32 = O.user_weights(scores, ptr, cols, dtype=np.float32)
    w, rmse = fusion.learn_per_user(models, ptr, cols)
    assert w.shape == rmse.shape == (n_users, 3) and w.dtype == np.float32
    _within('rmse (%d items)' % n_items, rmse, r64, r32)
    _within('w (%d items)' % n_items, w, w64, w32)
    empty = np.flatnonzero(np.diff(ptr) == 0)
    assert len(empty) >= 10 and np.all(rmse[empty] == 0.0) and np.all(w[empty] == 1.0)              # the zero-mean rows: exactly 1.0
    again = tkr_hip.fusion_user_weights(_models_dev(models), _dev(ptr), _dev(cols))
    np.testing.assert_array_equal(_bits(again[0].cpu().numpy()), _bits(rmse))
    np.testing.assert_array_equal(_bits(again[1].cpu().numpy()), _bits(w))


def test_user_weights_without_any_like():
    import tkr_hip
    models = _exact_models((8, 50), biased=(1,), n_users=5, n_items=9)
    rmse, w = tkr_hip.fusion_user_weights(_models_dev(models), _dev(np.zeros(6, np.int64)), _dev(np.zeros(0, np.int32)))
    assert torch.all(rmse == 0) and torch.all(w == 1)


# ---- the command line on tests/golden/g4 -------------------------------------------------------------------------------------------
@pytest.fixture()
def g4(golden_dir, tmp_path):
    """g4 copied to tmp_path; model A is g4/model, model B a noise model with a bias"""
    import textio
    data, A, B = str(tmp_path / 'data'), str(tmp_path / 'A'), str(tmp_path / 'B')
    shutil.copytree(os.path.join(golden_dir, 'g4', 'data'), data)
    shutil.copytree(os.path.join(golden_dir, 'g4', 'model'), A)
    os.mkdir(B)
    rng = np.random.Generator(np.random.PCG64(44))
    textio.write_matrix(os.path.join(B, 'final-U.dat'), (rng.standard_normal((160, 5)) * 0.3).astype(np.float32), where='host')
    textio.write_matrix(os.path.join(B, 'final-V.dat'), (rng.standard_normal((120, 5)) * 0.3).astype(np.float32), where='host')
    textio.write_matrix(os.path.join(B, 'final-B.dat'), (rng.standard_normal((120, 1)) * 0.3).astype(np.float32), where='host')
    uids, vids = R.read_id_list(os.path.join(data, 'uid')), R.read_id_list(os.path.join(data, 'vid'))
    models = []
    for d in (A, B):
        b = os.path.join(d, 'final-B.dat')
        models.append((R.read_embed_text(os.path.join(d, 'final-U.dat'), uids), R.read_embed_text(os.path.join(d, 'final-V.dat'), vids),
                       R.read_embed_text(b, vids).reshape(-1) if os.path.exists(b) else None))
    models = [tuple(None if t is None else np.asarray(t, dtype=np.float32) for t in m) for m in models]
    return dict(data=data, A=A, B=B, out=str(tmp_path / 'fused'), models=models, tmp=tmp_path)


def _evaluate_equals_the_oracle(g):
    import evaluate
    assert evaluate.main(['-d', g['data'], '-m', g['out'], '-sl', 'im', 'om']) == R.evaluate_cli(g['data'], g['out'], scenarios=('im', 'om'))


def test_fuse_cli_given_weights_writes_the_oracles_tables(g4, capsys):
    import fuse
    import textio
    g = g4
    w = fuse.main(['-d', g['data'], '-m', g['A'], g['B'], '-o', g['out'], '--method', 'w', '--weights', '0.5', '2'])
    assert w.tolist() == [0.5, 2.0] and capsys.readouterr().out.split() == ['0.5', '2']
    Uo, Vo = O.fuse(g['models'], [0.5, 2.0])
    assert Uo.shape == (160, 8 + 5 + 1)
    for name, want in (('final-U.dat', Uo), ('final-V.dat', Vo)):
        ref = str(g['tmp'] / ('ref-' + name))
        textio.write_matrix(ref, want, where='host')
        assert open(os.path.join(g['out'], name), 'rb').read() == open(ref, 'rb').read(), name
    assert not os.path.exists(os.path.join(g['out'], 'final-B.dat')) and not os.path.exists(os.path.join(g['out'], 'final-W.dat'))
    meta = json.load(open(os.path.join(g['out'], 'fusion.json')))
    assert meta['method'] == 'w' and meta['weights'] == [0.5, 2.0] and [os.path.basename(m) for m in meta['models']] == ['A', 'B']
    _evaluate_equals_the_oracle(g)


def test_fuse_cli_learns_pairwise_weights(g4, capsys):
    import fuse
    g = g4
    w = fuse.main(['-d', g['data'], '-m', g['A'], g['B'], '-o', g['out'], '--method', 'b', '--samples', '20000', '--batch', '1000', '--seed', '3'])
    assert len(capsys.readouterr().out.strip().splitlines()[-1].split()) == 2
    T = R.load_training(os.path.join(g['data'], 'uid'), os.path.join(g['data'], 'vid'), os.path.join(g['data'], 'f0tr.txt'))
    row_ptr, pos, srt = P.build_csr(T['tr_data'], T['n_users'])
    args = (g['models'], T['tr_users'], row_ptr, pos, srt, T['n_items'], 20000, 1000, 1e-4, 0.0025, 3)
    W64, W32 = O.learn_pairwise(*args, dtype=np.float64)[0], O.learn_pairwise(*args, dtype=np.float32)[0]
    _within('fuse.py --method b', w, W64, W32)
    meta = json.load(open(os.path.join(g['out'], 'fusion.json')))
    assert len(pos) == 964                                           # fewer training pairs than --batch: the batch is cut to them
    assert meta['method'] == 'b' and meta['n_batches'] == 20 and meta['seed'] == 3 and meta['batch'] == 964 and meta['samples'] == 20000
    assert meta['lr'] == 1e-4 and meta['lambda_w'] == 0.0025 and meta['weights'] == [float(x) for x in w]
    assert not os.path.exists(os.path.join(g['out'], 'final-W.dat'))
    _evaluate_equals_the_oracle(g)


def test_fuse_cli_learns_per_user_weights(g4, capsys):
    import foldin
    import fuse
    import textio
    g = g4
    w = fuse.main(['-d', g['data'], '-m', g['A'], g['B'], '-o', g['out'], '--method', 'e'])
    assert w.shape == (160, 2)
    uids, vids = R.read_id_list(os.path.join(g['data'], 'uid')), R.read_id_list(os.path.join(g['data'], 'vid'))
    ptr, cols = foldin.liked_csr(textio.parse_ratings(os.path.join(g['data'], 'f0tr.txt'), uids, vids, where='host'), 160, 120)
    scores = O.chain_scores(g['models'])
    w64, w32 = O.user_weights(scores, ptr, cols, dtype=np.float64)[1], O.user_weights(scores, ptr, cols, dtype=np.float32)[1]
    _within('fuse.py --method e', w, w64, w32)
    ref = str(g['tmp'] / 'ref-final-W.dat')
    textio.write_matrix(ref, w, where='host')
    assert open(os.path.join(g['out'], 'final-W.dat'), 'rb').read() == open(ref, 'rb').read()
    meta = json.load(open(os.path.join(g['out'], 'fusion.json')))
    assert meta['method'] == 'e' and len(meta['weights']) == 2
    _evaluate_equals_the_oracle(g)
