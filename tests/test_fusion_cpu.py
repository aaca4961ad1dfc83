"""K16 (fusion of several models) without a GPU: the ABI and the wrappers' refusals, the oracle of tests/_fusion_oracle.py against
hand values, torch autograd and a dense restatement of the reference, and fusion.fuse / fusion.fixed_weights, which are host code."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _fusion_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ('tkr_fusion_features', 'tkr_fusion_sgd', 'tkr_fusion_user_weights')


def test_header_binding_and_library_declare_the_fusion_entry_points():
    import tkr_hip
    header = open(os.path.join(ROOT, 'include', 'tkr.h')).read()
    declared = re.findall(r'^int(?:32_t|64_t)? (tkr_\w+)\(', header, flags=re.M)
    lib = C.CDLL(tkr_hip.LIB_PATH)
    for name in NAMES:
        assert name in declared and name in tkr_hip.EXPORTS
        getattr(lib, name)
    assert int(re.search(r'#define TKR_FUSION_MAX_MODELS (\d+)', header).group(1)) == tkr_hip.FUSION_MAX_MODELS == 16
    assert callable(tkr_hip.fusion_features) and callable(tkr_hip.fusion_sgd) and callable(tkr_hip.fusion_user_weights)
    # the struct the header declares: 16 x (3 pointers, 2 int32) + 4 int32
    assert C.sizeof(tkr_hip.FusionModels) == 16 * 32 + 16
    # arguments are checked before any device access and before any launch: this runs on a machine without a GPU
    p = C.c_void_p(4096)                                              # never dereferenced: every call below fails its checks
    sgd = lib.tkr_fusion_sgd
    sgd.restype = C.c_int
    sgd.argtypes = [C.c_void_p, C.c_int64, C.c_int32, C.c_int32, C.c_int64, C.c_float, C.c_float, C.c_void_p, C.c_void_p, C.c_void_p]
    good = dict(D=p, n_rows=100, M=3, batch=10, nb=10, lr=0.1, lam=0.1, W=p, loss=None, stream=None)
    for change in (dict(D=None), dict(W=None), dict(M=0), dict(M=17), dict(batch=0), dict(nb=0), dict(nb=11), dict(n_rows=0)):
        assert sgd(*dict(good, **change).values()) == -1, change
    st = tkr_hip.FusionModels()
    st.n_models, st.n_users, st.n_items = 17, 5, 5
    feat = lib.tkr_fusion_features
    feat.restype = C.c_int
    feat.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_uint64, C.c_uint64, C.c_int64,
                     C.c_void_p, C.c_void_p, C.c_void_p]
    uw = lib.tkr_fusion_user_weights
    uw.restype = C.c_int
    uw.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p]
    assert feat(C.byref(st), p, 1, p, p, p, 5, 0, 0, 10, p, None, None) == -1          # 17 models
    assert uw(C.byref(st), p, p, 5, p, p, None) == -1
    st.n_models = 1                                                   # a model without tables
    assert feat(C.byref(st), p, 1, p, p, p, 5, 0, 0, 10, p, None, None) == -1
    assert uw(C.byref(st), p, p, 5, p, p, None) == -1
    assert feat(None, p, 1, p, p, p, 5, 0, 0, 10, p, None, None) == -1


class _Csr:
    def __init__(self):
        self.tr_users = torch.zeros(1, dtype=torch.int32)
        self.row_ptr = torch.zeros(5, dtype=torch.int32)
        self.pos_cols = self.cols_sorted = torch.zeros(1, dtype=torch.int32)


def test_wrappers_refuse_with_tkr_error_and_without_a_launch():
    import fusion
    import tkr_hip
    U, V = torch.zeros((4, 8)), torch.zeros((10, 8))
    ptr, cols = torch.tensor([0, 1, 2, 2, 3]), torch.tensor([1, 2, 3], dtype=torch.int32)
    csr = _Csr()

    def every_wrapper(models, match):
        with pytest.raises(tkr_hip.TkrError, match=match):
            tkr_hip.fusion_features(models, csr, 10, 0, 0, 5)
        with pytest.raises(tkr_hip.TkrError, match=match):
            tkr_hip.fusion_user_weights(models, ptr, cols)

    every_wrapper([(U, V, None)] * 17, '1 .. 16 models')
    every_wrapper([], '1 .. 16 models')
    every_wrapper([(U, V, None), (torch.zeros((5, 8)), V, None)], 'model 1 has 5 user and 10 item rows')
    every_wrapper([(U, V, None), (U, torch.zeros((11, 8)), None)], 'model 1 has 4 user and 11 item rows')
    every_wrapper([(U.double(), V, None)], 'U of model 0 must be torch.float32')
    every_wrapper([(U, V.half(), None)], 'V of model 0 must be torch.float32')
    every_wrapper([(U, torch.zeros((8, 10)).t(), None)], 'V of model 0 must be contiguous')
    every_wrapper([(U, V, torch.zeros(10, dtype=torch.float64))], 'bias of model 0 must be torch.float32')
    every_wrapper([(U, V, torch.zeros(9))], 'one value per item')
    every_wrapper([(U, torch.zeros((10, 9)), None)], 'must share k')
    every_wrapper([(U, V, None)], 'must live on')                     # host tensors: refused, never handed to the library
    D, W = torch.zeros((20, 3)), torch.zeros(3)
    for batch in (0, -4):
        with pytest.raises(tkr_hip.TkrError, match='batch >= 1'):
            tkr_hip.fusion_sgd(D, batch, 1, 0.1, 0.1, W)
    with pytest.raises(tkr_hip.TkrError, match='D must be torch.float32'):
        tkr_hip.fusion_sgd(D.double(), 5, 1, 0.1, 0.1, W)
    with pytest.raises(tkr_hip.TkrError, match='D must be contiguous'):
        tkr_hip.fusion_sgd(torch.zeros((3, 20)).t(), 5, 1, 0.1, 0.1, W)
    with pytest.raises(tkr_hip.TkrError, match='1 .. 16 models'):
        tkr_hip.fusion_sgd(torch.zeros((20, 17)), 5, 1, 0.1, 0.1, torch.zeros(17))
    with pytest.raises(tkr_hip.TkrError, match='one weight per column'):
        tkr_hip.fusion_sgd(D, 5, 1, 0.1, 0.1, torch.zeros(4))
    with pytest.raises(tkr_hip.TkrError, match='do not fit'):
        tkr_hip.fusion_sgd(D, 5, 5, 0.1, 0.1, W)
    with pytest.raises(tkr_hip.TkrError, match='one GPU'):
        tkr_hip.fusion_sgd(D, 5, 4, 0.1, 0.1, W)
    assert fusion.METHODS == ('a', 'p', 'b', 'e', 'w')


def test_oracle_sgd_first_step_by_hand_and_batch_counts():
    rng = np.random.Generator(np.random.PCG64(1))
    D = rng.standard_normal((7, 3))
    W, cost = O.sgd(D, 7, 1, 0.25, 0.0025)
    np.testing.assert_allclose(W, 0.25 * 0.5 * D.sum(axis=0), rtol=1e-14)      # W = 0: sigma(0) = 1/2 for every row
    np.testing.assert_allclose(cost, 7 * np.log(2.0), rtol=1e-14)
    import fusion
    for (n, B), want in (((10, 3), 3), ((9, 3), 2), ((3, 3), 0), ((2, 3), 0), ((10_000_000, 10_000), 999)):
        assert O.n_batches(n, B) == want == fusion.n_batches_of(n, B), (n, B)
    for n in range(0, 40):
        for B in range(1, 9):
            assert O.n_batches(n, B) == fusion.n_batches_of(n, B)


def test_oracle_sgd_gradient_equals_autograd_of_the_reference_cost():
    """ranking_fusion.py:25-32 written in torch: x_ui = W . S[u, i, :], x_uj likewise, obj = sum log sigmoid(x_ui - x_uj) -
    lambda_w / 2 sum W^2, cost = -obj"""
    rng = np.random.Generator(np.random.PCG64(2))
    S = torch.from_numpy(rng.standard_normal((6, 9, 4)))
    u, i, j = (torch.from_numpy(rng.integers(0, n, 50)) for n in (6, 9, 9))
    W0 = rng.standard_normal(4)
    lam, lr = 0.3, 0.01
    W = torch.tensor(W0, requires_grad=True)
    x_uij = torch.matmul(W, S[u, i, :].T) - torch.matmul(W, S[u, j, :].T)
    cost = -(torch.log(torch.sigmoid(x_uij)).sum() - lam * 0.5 * (W ** 2).sum())
    cost.backward()
    d = (S[u, i, :] - S[u, j, :]).numpy()
    W1, c = O.sgd_step(W0.copy(), d, lr, lam)
    np.testing.assert_allclose(c, cost.item(), rtol=1e-13)
    np.testing.assert_allclose(W1, W0 - lr * W.grad.numpy(), rtol=1e-12, atol=1e-15)
    # ... and the defaults of that class and its train(): ranking_fusion.py:8 (lambda_w, learning_rate), :39 (batch_size), :44 (samples)
    import inspect
    import fusion
    kw = {k: v.default for k, v in inspect.signature(fusion.learn_pairwise).parameters.items() if v.default is not inspect.Parameter.empty}
    assert (kw['lambda_w'], kw['lr'], kw['batch_size'], kw['n_samples'], kw['seed'], kw['want_loss']) == (0.0025, 1.0e-4, 10000, 10000000, 0, False)
    assert 'epochs' not in kw


def _small_models(rng, n_users, n_items, ks, biased):
    return [((rng.standard_normal((n_users, k)) * 0.3), (rng.standard_normal((n_items, k)) * 0.3),
             (rng.standard_normal(n_items) * 0.3) if q in biased else None) for q, k in enumerate(ks)]


def test_oracle_user_weights_equal_the_dense_restatement_of_the_reference():
    rng = np.random.Generator(np.random.PCG64(3))
    n_users, n_items, M = 20, 15, 3
    scores = [rng.standard_normal((n_users, n_items)) for _ in range(M)]
    lmat = (rng.random((n_users, n_items)) < 0.3).astype(np.float64)
    lmat[4] = 0                                                       # a user without likes: mean 0
    lmat[9] = 0
    lmat[9, 2] = 1
    for S in scores:
        S[9, 2] = 1.0                                                 # every model scores the user's one like exactly 1: mean 0, row not empty
    ptr = np.zeros(n_users + 1, np.int64)
    np.cumsum(lmat.sum(axis=1).astype(np.int64), out=ptr[1:])
    cols = np.nonzero(lmat)[1].astype(np.int32)
    rmse, w = O.user_weights(scores, ptr, cols)
    rmse_d, w_d = O.user_weights_dense(np.stack(scores, axis=2), lmat)
    np.testing.assert_allclose(rmse, rmse_d, rtol=1e-13, atol=1e-15)
    zero = np.array([4, 9])
    rest = np.setdiff1d(np.arange(n_users), zero)
    np.testing.assert_allclose(w[rest], w_d[rest], rtol=1e-13)
    assert np.all(rmse[zero] == 0) and np.all(w[zero] == 1.0) and np.all(w_d[zero] == 0.0)      # the stated departure
    np.testing.assert_allclose(np.log(w[rest]).sum(axis=1), 0, atol=1e-12)                    # the deviations from the mean add up to 0
    # the weights in use: models whose scores are these matrices (U = S, V = I), fused with w, score as efusion.py's do_fusion does
    import fusion
    models = [(S, np.eye(n_items), None) for S in scores]
    Uf, Vf = fusion.fuse(models, w, dtype=torch.float64)
    np.testing.assert_allclose(Uf @ Vf.T, O.do_fusion(w, np.stack(scores, axis=2)), rtol=0, atol=1e-12)


@pytest.mark.parametrize('per_user', [False, True])
def test_fuse_is_the_weighted_sum_of_the_models_scores(per_user):
    import fusion
    rng = np.random.Generator(np.random.PCG64(4))
    n_users, n_items = 23, 31
    models = _small_models(rng, n_users, n_items, (5, 8, 3), biased=(0, 2))
    w = rng.standard_normal((n_users, 3)) if per_user else rng.standard_normal(3)
    Uf, Vf = fusion.fuse(models, w, dtype=torch.float64)
    assert Uf.shape == (n_users, 5 + 8 + 3 + 2) and Vf.shape == (n_items, 18) and Uf.dtype == np.float64
    want = O.weighted_sum(models, w)
    err = float(np.abs(Uf @ Vf.T - want).max())
    print('per_user = %s: max |fused - weighted sum| = %.3g' % (per_user, err))
    assert err <= 1e-12
    U32, V32 = fusion.fuse([(U.astype(np.float32), V.astype(np.float32), None if b is None else b.astype(np.float32)) for U, V, b in models], w)
    assert U32.dtype == np.float32 and V32.dtype == np.float32 and U32.flags.c_contiguous and V32.flags.c_contiguous
    Uo, Vo = O.fuse(models, w)
    np.testing.assert_array_equal(U32, Uo)
    np.testing.assert_array_equal(V32, Vo)
    Ut, Vt = fusion.fuse([tuple(None if t is None else torch.from_numpy(t) for t in m) for m in models], torch.as_tensor(w), dtype=torch.float64)
    assert isinstance(Ut, torch.Tensor) and np.array_equal(Ut.numpy(), Uf) and np.array_equal(Vt.numpy(), Vf)
    with pytest.raises(ValueError, match='weights must be'):
        fusion.fuse(models, np.ones(4))


def test_fuse_ranks_exact_arithmetic_tables_like_do_fusion():
    """entries m * 2^-6, biases m * 2^-12, weights powers of two: every product and sum is exact in fp32 in any order, so the argsort
    of the fused product is the argsort of efusion.py's do_fusion"""
    import fusion
    rng = np.random.Generator(np.random.PCG64(5))
    n_users, n_items = 40, 60
    models = [(rng.integers(-3, 4, (n_users, k)).astype(np.float32) / 64, rng.integers(-3, 4, (n_items, k)).astype(np.float32) / 64,
               (rng.integers(-2, 3, n_items).astype(np.float32) / 4096) if q == 1 else None) for q, k in enumerate((8, 50, 128))]
    scores = np.stack([U @ V.T + (0 if b is None else b.reshape(1, -1)) for U, V, b in models], axis=2).astype(np.float32)
    for w in (np.array([0.5, 2.0, 0.25], np.float32), (2.0 ** rng.integers(-2, 3, (n_users, 3))).astype(np.float32)):
        Uf, Vf = fusion.fuse(models, w)
        fused = Uf @ Vf.T
        want = O.do_fusion(np.broadcast_to(w.reshape(-1, 3), (n_users, 3)), scores)
        np.testing.assert_array_equal(fused, want)
        np.testing.assert_array_equal(np.argsort(fused, axis=1, kind='stable'), np.argsort(want, axis=1, kind='stable'))


def test_planted_case_the_model_that_generated_the_likes_gets_the_weight():
    """model A generated the likes (each user's top items under A), model B is noise: order only, no thresholds"""
    rng = np.random.Generator(np.random.PCG64(6))
    n_users, n_items, k, n_like = 60, 80, 6, 8
    A = (rng.standard_normal((n_users, k)).astype(np.float32), rng.standard_normal((n_items, k)).astype(np.float32), None)
    B = ((rng.standard_normal((n_users, k))).astype(np.float32), (rng.standard_normal((n_items, k))).astype(np.float32), None)
    # A's scores of its likes are near 1: scale A so that the liked scores average 1 (efusion measures the distance to 1)
    SA = A[0] @ A[1].T
    likes = np.argsort(-SA, axis=1)[:, :n_like]
    scale = 1.0 / np.sqrt(np.take_along_axis(SA, likes, axis=1).mean())
    A = ((A[0] * scale).astype(np.float32), (A[1] * scale).astype(np.float32), None)
    tr = {u: [int(c) for c in likes[u]] for u in range(n_users)}
    from oracle import plan_np as P
    row_ptr, pos, srt = P.build_csr(tr, n_users)
    W, costs, _ = O.learn_pairwise([A, B], list(tr.keys()), row_ptr, pos, srt, n_items, 4001, 200, 1e-3, 0.0025, 1)
    assert len(costs) == 20 and W[0] > abs(W[1]), W
    ptr = np.arange(n_users + 1, dtype=np.int64) * n_like
    cols = np.sort(likes, axis=1).astype(np.int32).reshape(-1)
    _, w = O.user_weights(O.chain_scores([A, B]), ptr, cols)
    assert w[:, 0].mean() > w[:, 1].mean(), w.mean(axis=0)
    # the fused model (fusion.fuse on either set of weights) ranks the likes ahead of where the noise model alone puts them
    import fusion

    def mean_rank_of_likes(score):
        rank = np.argsort(np.argsort(-score, axis=1, kind='stable'), axis=1, kind='stable')
        return float(np.take_along_axis(rank, likes, axis=1).mean())

    noise = mean_rank_of_likes(B[0] @ B[1].T)
    for weights in (W, w):
        Uf, Vf = fusion.fuse([A, B], weights)
        assert mean_rank_of_likes(Uf @ Vf.T) < noise


def test_fixed_weights_against_the_cited_lines():
    import fusion
    for M in (1, 3, 8):
        a = fusion.fixed_weights(M, 'a')
        assert a.dtype == np.float32 and np.array_equal(a, np.full(M, np.float32(1.0 / M)))       # afusion.py:27
        for p in (0.1, 0.5, 0.9):
            want = np.zeros(M, dtype=np.float32)                      # pfusion.py:63-66
            for i in range(M):
                want[i] = np.power(1 - p, i) * p
            np.testing.assert_array_equal(fusion.fixed_weights(M, 'p', p=p), want)
    assert fusion.fixed_weights(3, 'p', p=0.5).tolist() == [0.5, 0.25, 0.125]
    assert fusion.fixed_weights(2, 'w', weights=[0.5, 2]).tolist() == [0.5, 2.0]
    with pytest.raises(ValueError):
        fusion.fixed_weights(2, 'w', weights=[1.0])
    with pytest.raises(ValueError):
        fusion.fixed_weights(2, 'p')
    with pytest.raises(ValueError):
        fusion.fixed_weights(2, 'b')
