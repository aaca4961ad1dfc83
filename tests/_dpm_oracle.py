"""NumPy restatement of K22 (an MLP content encoder trained by dense RMSProp, and DPM around it), written from the equations of
DESIGN.md section 4 K22 on top of _als_oracle / _cer_oracle:

    layer l:   x_l = h_{l-1} W_l + bias_l,   h_l = 1 / (1 + exp(-x_l)) for every layer but the last, h_L = x_L = F;   h_0 = the batch's rows of X
    batch:     obj = 1/2 sum (Y - F)^2;   delta_L = F - Y,   delta_{l-1} = (delta_l W_l^T) * h_{l-1} (1 - h_{l-1})
               g(W_l) = h_{l-1}^T delta_l,   g(bias_l) = sum_b delta_l[b]        every gradient from the parameters before the batch
    RMSProp:   ms' = ms + (g g - ms) (1 - RHO),   w' = w - lr g / sqrt(ms' + EPS)                      (oracle/ref_np.py:338-341, dense)
    DPM iteration (dpm.py:31-60):  Fe = net(F);  V = Fe;  U = user half-step against V;  V = item half-step with the prior Fe, weight lv;
               one epoch of the net towards V;  loss = sum row_loss + 1/2 lu |U|^2 + sum of the epoch's batch objectives

dtype float64 is the reference the GPU tests measure against; dtype float32 the yardstick for its error (`@` and every elementwise
operation in float32)."""
import numpy as np

from oracle.ref_np import EPS, RHO

import _cer_oracle as C

PARTS = ('W', 'bias', 'msW', 'msb')


def copy_params(params, dtype=np.float64):
    return [{name: np.array(layer[name], dtype=dtype) for name in PARTS} for layer in params]


def start(widths, seed):
    """the start als.MLP makes: W Glorot-uniform drawn in fp32 layer by layer from one PCG64 stream, biases 0, slots 1"""
    rng = np.random.Generator(np.random.PCG64(seed))
    params = []
    for fan_in, fan_out in zip(widths, widths[1:]):
        limit = np.float32(np.sqrt(6.0 / (fan_in + fan_out)))
        W = ((np.float32(2) * rng.random((fan_in, fan_out), dtype=np.float32) - np.float32(1)) * limit).astype(np.float32)
        params.append(dict(W=W, bias=np.zeros(fan_out, np.float32), msW=np.ones((fan_in, fan_out), np.float32), msb=np.ones(fan_out, np.float32)))
    return params


def epoch_order(seed, epoch, n):
    return np.random.Generator(np.random.PCG64(np.random.SeedSequence([seed, epoch]))).permutation(n)


def mlp_forward(params, X, dtype=np.float64, keep=False):
    """-> F [rows of X, k] (keep: the list h_0 .. h_L instead)"""
    dt = np.dtype(dtype).type
    h = np.asarray(X, dtype=dtype)
    hs = [h]
    for l, layer in enumerate(params):
        x = (h @ np.asarray(layer['W'], dtype=dtype) + np.asarray(layer['bias'], dtype=dtype)).astype(dtype)
        h = x if l + 1 == len(params) else (dt(1) / (dt(1) + np.exp(-x))).astype(dtype)
        hs.append(h)
    return hs if keep else h


def objective(params, X, Y):
    """1/2 sum (Y - F)^2 in float64"""
    return 0.5 * ((np.asarray(Y, dtype=np.float64) - mlp_forward(params, X)) ** 2).sum()


def gradients(params, X, Y, dtype=np.float64):
    """-> (objective, [(g(W_l), g(bias_l))])"""
    hs = mlp_forward(params, X, dtype, keep=True)
    Y = np.asarray(Y, dtype=dtype)
    dt = np.dtype(dtype).type
    obj = float(dt(0.5) * ((Y - hs[-1]) ** 2).sum())
    delta = (hs[-1] - Y).astype(dtype)
    grads = [None] * len(params)
    for l in range(len(params) - 1, -1, -1):
        grads[l] = ((hs[l].T @ delta).astype(dtype), delta.sum(axis=0).astype(dtype))
        if l:
            delta = ((delta @ np.asarray(params[l]['W'], dtype=dtype).T) * (hs[l] * (dt(1) - hs[l]))).astype(dtype)
    return obj, grads


def rmsprop(w, ms, g, lr, dtype=np.float64):
    """in place on w and ms; the constants are the float32 ones of oracle.ref_np in every dtype, lr is rounded to float32 first"""
    dt = np.dtype(dtype).type
    ms[...] = (ms + (g * g - ms) * (dt(1) - dt(RHO))).astype(dtype)
    w[...] = (w - dt(np.float32(lr)) * g / np.sqrt(ms + dt(EPS))).astype(dtype)


def mlp_batch(params, X, Y, lr, dtype=np.float64):
    """one batch, in place on params (arrays of `dtype`) -> its objective before the step"""
    obj, grads = gradients(params, X, Y, dtype)
    for layer, (gW, gb) in zip(params, grads):
        rmsprop(layer['W'], layer['msW'], gW, lr, dtype)
        rmsprop(layer['bias'], layer['msb'], gb, lr, dtype)
    return obj


def mlp_fit(params, X, Y, order, batch, lr, dtype=np.float64):
    """one epoch over the rows `order`, in place on params -> the list of batch objectives"""
    X, Y = np.asarray(X, dtype=dtype), np.asarray(Y, dtype=dtype)
    order = np.asarray(order, dtype=np.int64)
    return [mlp_batch(params, X[order[t:t + batch]], Y[order[t:t + batch]], lr, dtype) for t in range(0, len(order), batch)]


class Net:
    """the encoder as dpm_iteration sees it: out(F), and fit(F, V) -> the sum of an epoch's batch objectives.  orders: one row order per
    epoch, taken in turn"""

    def __init__(self, params, lr, batch, orders, dtype=np.float64):
        self.params, self.lr, self.batch, self.orders, self.dtype = copy_params(params, dtype), lr, batch, list(orders), dtype
        self.epochs_done = 0

    def out(self, F):
        return mlp_forward(self.params, F, self.dtype)

    def fit(self, F, V):
        order = self.orders[self.epochs_done]
        self.epochs_done += 1
        return float(np.sum(np.asarray(mlp_fit(self.params, F, V, order, self.batch, self.lr, self.dtype), dtype=np.float64)))


def dpm_iteration(U, V, F, user_likes, item_likes, encoder, *, a, b, lu, lv, dtype=np.float64):
    """one iteration of dpm.py:31-60 -> (U, V, loss); the encoder is trained in place"""
    u_rated = [u for u, l in enumerate(user_likes) if len(l)]
    i_rated = [i for i, l in enumerate(item_likes) if len(l)]
    Fe = np.asarray(encoder.out(F), dtype=dtype)
    U, _ = C.half_step(U, Fe, user_likes, i_rated, a=a, b=b, ridge_in_G=lu, ridge=0.0, dtype=dtype)
    V, rl = C.half_step_prior(Fe, U, item_likes, u_rated, Fe, a=a, b=b, ridge_in_G=0.0, ridge=lv, w_prior=lv, dtype=dtype)
    fit = encoder.fit(F, V)
    loss = rl.sum() + 0.5 * lu * (U.astype(np.float64) ** 2).sum() + fit
    return U, V, float(loss)


def dpm_train(U, V, F, user_likes, item_likes, encoder, *, a, b, lu, lv, max_iter, dtype=np.float64):
    """the loop of dpm.py:20-64 -> (U, V, losses); after it every item without a like holds its row of encoder.out(F)"""
    U, V = np.array(U, dtype=dtype), np.array(V, dtype=dtype)
    losses = []
    for _ in range(max_iter):
        U, V, loss = dpm_iteration(U, V, F, user_likes, item_likes, encoder, a=a, b=b, lu=lu, lv=lv, dtype=dtype)
        losses.append(loss)
    Fe = np.asarray(encoder.out(F), dtype=dtype)
    for j, likes in enumerate(item_likes):
        if len(likes) == 0:
            V[j] = Fe[j]
    return U, V, losses


# ---- the inputs the tests share (tests/test_dpm_cpu.py states their premises without a GPU, tests/test_gpu_dpm.py runs them) -------------
E2E = dict(k=16, d=24, hidden=(12, 8), lu=0.1, lv=0.1, a=1.0, b=0.01, batch=8, lr=1e-2, iters=4, seed=0, mlp_seed=5)    # als.DPM on tests/golden/g2


def net_inputs(d, hidden, k, n=150, seed=40):
    """-> (params fp32, X fp32 [n, d] uniform [-1, 1), Y fp32 [n, k] uniform [-1, 1), order: a permutation of the rows)"""
    rng = np.random.Generator(np.random.PCG64([seed, d, k, len(hidden)]))
    X = (2 * rng.random((n, d), dtype=np.float32) - 1).astype(np.float32)
    Y = (2 * rng.random((n, k), dtype=np.float32) - 1).astype(np.float32)
    return start((d,) + tuple(hidden) + (k,), int(rng.integers(1 << 30))), X, Y, rng.permutation(n)
