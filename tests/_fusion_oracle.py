"""NumPy oracle of K16 (fusion of several models).  Theano is absent and the reference's fusion scripts are Python 2, so this file
RESTATES the cited lines of old/methods/{afusion,pfusion,efusion,ranking_fusion}.py, as oracle/ref_np.py restates the TF step;
nothing of theirs is copied.  The triplets are oracle.plan_np.sample_triplets, the per-model scores oracle.ref_np.mfma_chain_scores."""
import numpy as np

from oracle import plan_np as P
from oracle import ref_np as R

F32 = np.float32
ATOL, RTOL = 1e-5, 2e-4                      # the project's step tolerance (tests/test_gpu_foldin.py)


def bound(x64, d):
    """max(atol + rtol |x|, 4 d): d = the distance between the oracle in fp32 and in fp64 on the same input (4: the kernel sums in
    another order than NumPy) -- the rule of test_gpu_foldin.py::test_default_depth_within_measured_tolerance"""
    return np.maximum(ATOL + RTOL * np.abs(x64), 4 * d)


def n_batches(n_samples, batch):
    """ranking_fusion.py:46-54: z counts the batches run while (z + 1) * batch < n_samples"""
    z = 0
    while (z + 1) * batch < n_samples:
        z += 1
    return z


def chain_scores(models):
    """[S_m fp32 [n_users, n_items]]: every model's scores in the build's one order"""
    return [R.mfma_chain_scores(U, V, b) for U, V, b in models]


def features(scores, u, i, j):
    """D fp32 [n, M]: fl(s_m(u, i) - s_m(u, j))"""
    return np.stack([(S[u, i] - S[u, j]).astype(F32) for S in scores], axis=1)


def softplus_neg(x):
    return np.maximum(-x, 0) + np.log1p(np.exp(-np.abs(x)))


def sigmoid_neg(x):
    e = np.exp(-np.abs(x))
    return np.where(x >= 0, e / (1 + e), 1 / (1 + e))


def sgd_step(W, d, lr, lambda_w):
    """one call of train_model (ranking_fusion.py:25-37) on the batch's score differences d [B, M] = S[u, i, :] - S[u, j, :]:
    cost = -(sum log sigmoid(x) - lambda_w / 2 sum W^2), x = d W;  W <- W - lr * dcost/dW  -> (W', cost)"""
    x = d @ W
    cost = softplus_neg(x).sum(dtype=W.dtype) + W.dtype.type(0.5) * W.dtype.type(lambda_w) * (W * W).sum(dtype=W.dtype)
    grad = -(sigmoid_neg(x)[:, None] * d).sum(axis=0, dtype=W.dtype) + W.dtype.type(lambda_w) * W
    return (W - W.dtype.type(lr) * grad).astype(W.dtype), cost


def sgd(D, batch, nb, lr, lambda_w, W0=None, dtype=np.float64):
    """nb batches of D in order (ranking_fusion.py:48-54) -> (W, the cost of every batch)"""
    D = np.asarray(D, dtype=dtype)
    W = np.zeros(D.shape[1], dtype=dtype) if W0 is None else np.asarray(W0, dtype=dtype).copy()
    costs = np.zeros(nb, dtype=dtype)
    for z in range(nb):
        W, costs[z] = sgd_step(W, D[z * batch:(z + 1) * batch], lr, lambda_w)
    return W, costs


def learn_pairwise(models, tr_users, row_ptr, pos, srt, n_items, n_samples, batch, lr, lambda_w, seed, dtype=np.float64):
    """bfusion on K1's stream: sample_triplets -> chain scores -> sgd.  -> (W, costs, D)"""
    batch = min(batch, len(pos))
    nb = n_batches(n_samples, batch)
    u, i, j = P.sample_triplets(tr_users, row_ptr, pos, srt, n_items, seed, 0, max(nb * batch, 1))
    D = features(chain_scores(models), u, i, j)
    W, costs = sgd(D, batch, nb, lr, lambda_w, dtype=dtype)
    return W, costs, D


def user_weights(scores, like_ptr, like_cols, dtype=np.float64):
    """efusion.py:57-82 on sets of likes, with the zero-mean rows at 1.0 -> (rmse [n_users, M], w [n_users, M])"""
    n_users, M = len(like_ptr) - 1, len(scores)
    rmse = np.zeros((n_users, M), dtype=dtype)
    for u in range(n_users):
        cols = like_cols[like_ptr[u]:like_ptr[u + 1]]
        for m, S in enumerate(scores):
            err = S[u, cols].astype(dtype) - dtype(1)
            rmse[u, m] = np.sqrt((err * err).sum(dtype=dtype) / dtype(max(len(cols), 1)))
    mean = rmse.mean(axis=1, dtype=dtype)
    w = np.exp(-(rmse - mean[:, None])).astype(dtype)
    w[mean == 0] = 1
    return rmse, w


def user_weights_dense(trscores, lmat):
    """efusion.py:72-81 as it stands, on the dense [n_users, n_items, M] scores and the dense 0 / 1 like matrix (no duplicates): a row
    whose mean is 0 stays 0"""
    weight = np.zeros((trscores.shape[0], trscores.shape[2]), dtype=np.float64)
    svec = lmat.sum(axis=1)
    svec[svec == 0] = 1
    for m in range(trscores.shape[2]):
        weight[:, m] = np.sqrt((((trscores[:, :, m] - lmat) ** 2) * lmat).sum(axis=1) / svec)
    rmse = weight.copy()
    for r in range(weight.shape[0]):
        wmean = weight[r].mean()
        if wmean != 0:
            weight[r] = np.exp(-(weight[r] - wmean))
    return rmse, weight


def do_fusion(weights, scores):
    """efusion.py:84-89: fusion[u, :] = sum_m weights[u, m] * scores[u, :, m], accumulated in the order m = 0, 1, ..."""
    fusion = np.zeros(scores[:, :, 0].shape, dtype=scores.dtype)
    for m in range(scores.shape[2]):
        fusion += weights[:, m:m + 1] * scores[:, :, m]
    return fusion


def weighted_sum(models, weights, dtype=np.float64):
    """sum_m w_m (U_m V_m^T + b_m) in `dtype`; weights [M] or [n_users, M]"""
    n_users = len(models[0][0])
    w = np.asarray(weights, dtype=dtype)
    w = np.broadcast_to(w.reshape(1, -1), (n_users, w.size)) if w.ndim == 1 else w
    out = 0
    for m, (U, V, b) in enumerate(models):
        s = np.asarray(U, dtype=dtype) @ np.asarray(V, dtype=dtype).T
        if b is not None:
            s = s + np.asarray(b, dtype=dtype).reshape(1, -1)
        out = out + w[:, m:m + 1] * s
    return out


def fuse(models, weights):
    """the fused tables of fusion.fuse, restated in NumPy fp32: [w_m U_m ...| w_m for every biased m], [V_m ...| b_m]"""
    n_users = len(models[0][0])
    w = np.asarray(weights, dtype=F32)
    w = np.broadcast_to(w.reshape(1, -1), (n_users, w.size)) if w.ndim == 1 else w
    left = [(np.asarray(U, dtype=F32) * w[:, m:m + 1]).astype(F32) for m, (U, V, b) in enumerate(models)]
    right = [np.asarray(V, dtype=F32) for U, V, b in models]
    for m, (U, V, b) in enumerate(models):
        if b is not None:
            left.append(np.ascontiguousarray(w[:, m:m + 1]))
            right.append(np.asarray(b, dtype=F32).reshape(-1, 1))
    return np.concatenate(left, axis=1), np.concatenate(right, axis=1)
