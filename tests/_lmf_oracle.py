"""NumPy restatement of K25 (logistic matrix factorisation, LMF), written from the equations of DESIGN.md section 4 K25.

Tables are augmented to K = k + 2 columns: a user row is [x, beta_u, 1], an item row [y, 1, beta_i]; the score of a pair is the dot
product over all K columns.  One column per side is fixed (the constant 1): column k + 1 of the users, column k of the items.

    loss = sum over ALL (u, i) of (1 + alpha r_ui) softplus(s_ui) - alpha sum over the likes of s_ui
           + 1/2 lam |non-fixed columns of the users|^2 + 1/2 lam |non-fixed columns of the items|^2

A half-step moves every row r of X against the frozen Y:

    D_r = sum over all rows c of Y of sigma(s_rc) y_c             L_r = sum over the likes c of r of (1 - sigma(s_rc)) y_c
    g_r = alpha L_r - D_r - lam x_r;  g_r[fixed] = 0;  h_r += g_r^2;  x_r += lr g_r / sqrt(h_r)

dtype float64 is the reference the GPU tests measure against; dtype float32 is the yardstick for its error and follows the kernels'
order: a score is a chain over the columns in column order, a slab's part of D a chain over the slab's rows in row order, the slabs are
added in fp64 in ascending order and rounded once; L is a chain over the likes in stored order, and for a row with more than
heavy_from likes the chains of its slabs of LIKE_SLAB likes, slab j added to accumulator j mod HEAVY_WAVES in fp64, the accumulators
added in ascending order.  (NumPy has no fma: a chain here rounds the product and the sum, the kernel's rounds once.)  sigma and softplus
are NumPy's, in their stable forms."""
import numpy as np

SLAB = 4096            # TKR_LMF_SLAB
LIKE_SLAB = 256        # TKR_LMF_LIKE_SLAB
HEAVY_WAVES = 16       # TKR_LMF_HEAVY_WAVES
NO_HEAVY = 1 << 62


def sigmoid(s):
    s = np.asarray(s)
    with np.errstate(over='ignore', under='ignore'):
        e = np.exp(-np.abs(s))
        return np.where(s >= 0, 1 / (1 + e), e / (1 + e)).astype(s.dtype)


def softplus(s):
    s = np.asarray(s)
    with np.errstate(over='ignore', under='ignore'):
        return (np.maximum(s, 0) + np.log1p(np.exp(-np.abs(s)))).astype(s.dtype)


def csr_rows(ptr, cols):
    ptr, cols = np.asarray(ptr, dtype=np.int64), np.asarray(cols, dtype=np.int64)
    return [cols[ptr[r]:ptr[r + 1]] for r in range(len(ptr) - 1)]


def to_csr(rows_likes):
    ptr = np.zeros(len(rows_likes) + 1, dtype=np.int64)
    np.cumsum([len(x) for x in rows_likes], out=ptr[1:])
    cols = np.concatenate([np.asarray(x, dtype=np.int32) for x in rows_likes] + [np.zeros(0, np.int32)]).astype(np.int32)
    return ptr, cols


def dense_rows(X, Y, dtype=np.float64, slab=SLAB):
    """-> (D [n_x, K] in dtype, sp float64 [n_x])"""
    X, Y = np.asarray(X, dtype=dtype), np.asarray(Y, dtype=dtype)
    if np.dtype(dtype) == np.float64:
        S = X @ Y.T
        return sigmoid(S) @ Y, softplus(S).sum(axis=1)
    n_x, K = X.shape
    D = np.zeros((n_x, K), dtype=np.float64)
    sp = np.zeros(n_x, dtype=np.float64)
    for first in range(0, len(Y), slab):
        Ys = Y[first:first + slab]
        S = np.zeros((n_x, len(Ys)), dtype=np.float32)
        for j in range(K):                                        # the first product: a chain over the columns
            S += X[:, j:j + 1] * Ys[:, j]
        P = sigmoid(S)
        part = np.zeros((n_x, K), dtype=np.float32)
        for c in range(len(Ys)):                                  # the second: a chain over the slab's rows
            part += P[:, c:c + 1] * Ys[c]
        D += part
        sp += softplus(S).astype(np.float64).sum(axis=1)
    return D.astype(np.float32), sp


def _like_sum(x, y, dtype):
    """-> (L, sum softplus(s), sum s) over the rows y, a chain in stored order"""
    L = np.zeros(len(x), dtype=dtype)
    sp = ss = 0.0
    for row in y:
        s = np.dot(x, row).astype(dtype)
        L += sigmoid(-s) * row
        sp += float(softplus(s))
        ss += float(s)
    return L, sp, ss


def step_rows(X, H, Y, D, rows_likes, *, fixed, alpha, lam, lr, dtype=np.float64, heavy_from=NO_HEAVY):
    """-> (X_new, H_new, row_loss float64): row_loss[r] = alpha sum_likes softplus(s) - alpha sum_likes s + 1/2 lam |x_r non-fixed|^2 at
    the X that came in.  A like listed twice counts twice"""
    dt = np.dtype(dtype).type
    Y, D = np.asarray(Y, dtype=dtype), np.asarray(D, dtype=dtype)
    Xn, Hn = np.array(X, dtype=dtype), np.array(H, dtype=dtype)
    K = Y.shape[1]
    free = np.arange(K) != fixed
    loss = np.zeros(len(rows_likes), dtype=np.float64)
    for r, likes in enumerate(rows_likes):
        x = Xn[r].copy()
        y = Y[np.asarray(likes, dtype=np.int64)]
        if np.dtype(dtype) == np.float32 and len(likes) > heavy_from:
            acc = np.zeros((HEAVY_WAVES, K + 2), dtype=np.float64)
            for j, first in enumerate(range(0, len(y), LIKE_SLAB)):
                L, sp, ss = _like_sum(x, y[first:first + LIKE_SLAB], dtype)
                acc[j % HEAVY_WAVES] += np.concatenate([L.astype(np.float64), [sp, ss]])
            total = np.zeros(K + 2, dtype=np.float64)
            for w in range(HEAVY_WAVES):
                total += acc[w]
            L, sp, ss = total[:K].astype(dtype), total[K], total[K + 1]
        else:
            L, sp, ss = _like_sum(x, y, dtype)
        g = (alpha * L.astype(np.float64) - D[r].astype(np.float64) - lam * x.astype(np.float64)).astype(dtype)
        hn = (g * g + Hn[r]).astype(dtype)
        xn = (x + (dt(lr) * g) / np.sqrt(hn)).astype(dtype)
        Xn[r, free], Hn[r, free] = xn[free], hn[free]
        loss[r] = alpha * sp - alpha * ss + 0.5 * lam * float((x[free].astype(np.float64) ** 2).sum())
    return Xn, Hn, loss


def gradient(X, Y, rows_likes, *, fixed, alpha, lam):
    """float64 -> g [n_x, K] = alpha L - D - lam x, zero in the fixed column: minus the derivative of `loss` by the rows of X"""
    X, Y = np.asarray(X, dtype=np.float64), np.asarray(Y, dtype=np.float64)
    S = X @ Y.T
    R = dense_counts(rows_likes, len(Y))
    g = alpha * ((R * (1 - sigmoid(S))) @ Y) - sigmoid(S) @ Y - lam * X
    g[:, fixed] = 0
    return g


def half_step(X, H, Y, rows_likes, *, fixed, alpha, lam, lr, dtype=np.float64, heavy_from=NO_HEAVY):
    """-> (X_new, H_new, the half-step's part of the loss at the X that came in: sum_r (sp_r + row_loss_r), without Y's regulariser)"""
    D, sp = dense_rows(X, Y, dtype)
    Xn, Hn, rl = step_rows(X, H, Y, D, rows_likes, fixed=fixed, alpha=alpha, lam=lam, lr=lr, dtype=dtype, heavy_from=heavy_from)
    return Xn, Hn, float(sp.sum() + rl.sum())


def reg(T, fixed, lam):
    T = np.asarray(T, dtype=np.float64)
    return 0.5 * lam * float((T[:, np.arange(T.shape[1]) != fixed] ** 2).sum())


def loss(Xa, Ya, R, *, alpha, lam):
    """the dense float64 objective written out; Xa [n_users, K] fixed column k + 1, Ya [n_items, K] fixed column k, R[u, i] = the number
    of times the like is listed"""
    Xa, Ya, R = (np.asarray(t, dtype=np.float64) for t in (Xa, Ya, R))
    k = Xa.shape[1] - 2
    S = Xa @ Ya.T
    return float(((1 + alpha * R) * softplus(S)).sum() - alpha * (R * S).sum()) + reg(Xa, k + 1, lam) + reg(Ya, k, lam)


def dense_counts(rows_likes, n_cols):
    R = np.zeros((len(rows_likes), n_cols), dtype=np.float64)
    for r, likes in enumerate(rows_likes):
        np.add.at(R[r], np.asarray(likes, dtype=np.int64), 1.0)
    return R


def init(n_users, n_items, k, seed):
    """-> (Xa fp32 [n_users, k + 2], Ya fp32 [n_items, k + 2]): the users' factors drawn first, then the items', N(0, 0.01); biases 0"""
    rng = np.random.Generator(np.random.PCG64(seed))
    Xa = np.zeros((n_users, k + 2), dtype=np.float32)
    Ya = np.zeros((n_items, k + 2), dtype=np.float32)
    Xa[:, :k] = rng.standard_normal((n_users, k), dtype=np.float32) * np.float32(0.01)
    Ya[:, :k] = rng.standard_normal((n_items, k), dtype=np.float32) * np.float32(0.01)
    Xa[:, k + 1] = 1
    Ya[:, k] = 1
    return Xa, Ya


def balance_alpha(n_users, n_items, n_likes):
    return (n_users * n_items - n_likes) / n_likes


def train(Xa, Ya, user_likes, item_likes, *, alpha, lam, lr, max_iter, dtype=np.float64, Hx=None, Hy=None):
    """-> (Xa, Ya, Hx, Hy, losses): per iteration a user half-step, then an item half-step; the logged loss is the objective where the
    item half-step took its gradient: at the new users and the old items"""
    Xa, Ya = np.array(Xa, dtype=dtype), np.array(Ya, dtype=dtype)
    k = Xa.shape[1] - 2
    Hx = np.ones_like(Xa) if Hx is None else np.array(Hx, dtype=dtype)
    Hy = np.ones_like(Ya) if Hy is None else np.array(Hy, dtype=dtype)
    hyper = dict(alpha=alpha, lam=lam, lr=lr, dtype=dtype)
    losses = []
    for _ in range(max_iter):
        Xa, Hx, _ = half_step(Xa, Hx, Ya, user_likes, fixed=k + 1, **hyper)
        Yn, Hy, part = half_step(Ya, Hy, Xa, item_likes, fixed=k, **hyper)
        losses.append(part + reg(Xa, k + 1, lam))
        Ya = Yn
    return Xa, Ya, Hx, Hy, losses


# ---- the inputs the tests share ------------------------------------------------------------------------------------------------------------
STEP_M = (0, 1, 2, 7, 8, 9, 31, 64, 65, 300, 5)          # likes per row: none, one, around heavy_from = 8, a wave's batch of 64, more than LIKE_SLAB


def step_inputs(k, side, n_x=23, n_y=41, seed=25):
    """-> (X fp32 [n_x, K], H, Y fp32 [n_y, K], rows_likes, fixed): normal(0, 0.5) tables with their constant columns, slots in [1, 2);
    side 'user': X rows are users (fixed k + 1); 'item': items (fixed k).  Row r has STEP_M[r mod 11] likes, with repeats where that
    is more than n_y"""
    rng = np.random.Generator(np.random.PCG64([seed, k, n_x, side == 'user']))
    K = k + 2
    X = (rng.standard_normal((n_x, K)) * 0.5).astype(np.float32)
    Y = (rng.standard_normal((n_y, K)) * 0.5).astype(np.float32)
    fixed, other = (k + 1, k) if side == 'user' else (k, k + 1)
    X[:, fixed] = 1
    Y[:, other] = 1
    H = (1 + rng.random((n_x, K))).astype(np.float32)
    rows = []
    for r in range(n_x):
        m = STEP_M[r % len(STEP_M)]
        rows.append(rng.integers(0, n_y, m) if m > n_y else rng.permutation(n_y)[:m])
    return X, H, Y, rows, fixed


E2E = dict(k=8, lam=0.6, alpha=10.0, lr=1.0, seed=0, iters=5)       # als-style end to end on tests/golden/g2
