"""NumPy restatement of K27 (softmax matrix factorisation, SMF), written from the equations of DESIGN.md section 4 K27.

Tables are augmented to K = k + 1 columns: a user row is [x, 1], an item row [y, beta_i]; the score of a pair is the dot product over
all K columns.  With n_u the likes of user u (a column named twice counts twice) and lse_u = log sum over ALL items c of exp(s_uc):

    F = sum_u (n_u lse_u - sum over the likes c of u of s_uc) + 1/2 lam (|x|^2 + |y|^2 + |beta|^2)

A half-step moves every row r of X against the frozen Y by full-gradient AdaGrad:

    D_r = sum over all rows c of Y of exp((s_rc - row_off[r]) - col_off[c]) y_c          L_r = sum over the likes c of r of y_c
    g_r = L_r - w_r D_r - lam x_r;  g_r[fixed] = 0;  h_r += g_r^2;  x_r += lr g_r / sqrt(h_r)

    users:  row_off = lse, w_r = n_r, fixed = k (the column of ones)
    items:  col_off[u] = lse_u - log n_u (+inf for a user without likes: its weight is +0), w_r = 1, nothing fixed

dtype float64 is the reference the GPU tests measure against; dtype float32 is the yardstick for its error and follows the kernels'
order: a score is a chain over the columns in column order; within a slab of SLAB rows of Y the log-sum-exp follows a running maximum
tile by tile (32 rows; the rows c mod 8 < 4 of a tile and the others apart, the two joined at the slab's end), a slab's part of D is a
chain over the slab's rows in row order, and the slabs are joined in fp64 in ascending order and rounded once; L is a chain over the
likes in stored order, and for a row with more than heavy_from likes the chains of its slabs of LIKE_SLAB likes, slab j added to
accumulator j mod HEAVY_WAVES in fp64, the accumulators added in ascending order.  (NumPy has no fma: a chain here rounds the product
and the sum, the kernel's rounds once.)"""
import numpy as np

SLAB = 4096            # TKR_SMF_SLAB
TILE = 32
LIKE_SLAB = 256        # TKR_LMF_LIKE_SLAB: the heavy rows are K25's
HEAVY_WAVES = 16       # TKR_LMF_HEAVY_WAVES
NO_HEAVY = 1 << 62


def csr_rows(ptr, cols):
    ptr, cols = np.asarray(ptr, dtype=np.int64), np.asarray(cols, dtype=np.int64)
    return [cols[ptr[r]:ptr[r + 1]] for r in range(len(ptr) - 1)]


def to_csr(rows_likes):
    ptr = np.zeros(len(rows_likes) + 1, dtype=np.int64)
    np.cumsum([len(x) for x in rows_likes], out=ptr[1:])
    cols = np.concatenate([np.asarray(x, dtype=np.int32) for x in rows_likes] + [np.zeros(0, np.int32)]).astype(np.int32)
    return ptr, cols


def _scores32(X, Ys):
    S = np.zeros((len(X), len(Ys)), dtype=np.float32)
    with np.errstate(over='ignore', invalid='ignore'):
        for j in range(X.shape[1]):                               # a chain over the columns
            S += X[:, j:j + 1] * Ys[:, j]
    return S


def lse_rows(X, Y, dtype=np.float64, slab=SLAB):
    """-> lse [n_x] in dtype: log sum over all rows c of Y of exp(X[r] . Y[c])"""
    X, Y = np.asarray(X, dtype=dtype), np.asarray(Y, dtype=dtype)
    if np.dtype(dtype) == np.float64:
        S = X @ Y.T
        m = S.max(axis=1)
        return m + np.log(np.exp(S - m[:, None]).sum(axis=1))
    n_x = len(X)
    pairs = []
    for first in range(0, len(Y), slab):
        S = _scores32(X, Y[first:first + slab])
        m = np.full((2, n_x), -np.inf, dtype=np.float32)
        l = np.zeros((2, n_x), dtype=np.float32)
        with np.errstate(under='ignore'):
            for base in range(0, S.shape[1], TILE):
                tile = S[:, base:base + TILE]
                at = np.arange(tile.shape[1])
                for half in (0, 1):
                    mine = tile[:, (at % 8 < 4) == (half == 0)]
                    if mine.shape[1] == 0:
                        continue
                    top = np.maximum(m[half], mine.max(axis=1))
                    l[half] = l[half] * np.exp(m[half] - top)
                    for c in range(mine.shape[1]):
                        l[half] = l[half] + np.exp(mine[:, c] - top)
                    m[half] = top
            top = np.maximum(m[0], m[1])
            pairs.append((top, l[0] * np.exp(m[0] - top) + l[1] * np.exp(m[1] - top)))
    M = np.max([p[0] for p in pairs], axis=0).astype(np.float64)
    total = np.zeros(n_x, dtype=np.float64)
    for m, l in pairs:
        total += l.astype(np.float64) * np.exp(m.astype(np.float64) - M)
    return (M + np.log(total)).astype(np.float32)


def _offsets(n_x, n_y, row_off, col_off, dtype):
    ro = np.zeros(n_x, dtype=dtype) if row_off is None else np.asarray(row_off, dtype=dtype)
    co = np.zeros(n_y, dtype=dtype) if col_off is None else np.asarray(col_off, dtype=dtype)
    assert ro.shape == (n_x,) and co.shape == (n_y,)
    return ro, co


def dense_rows(X, Y, row_off=None, col_off=None, dtype=np.float64, slab=SLAB):
    """-> D [n_x, K] in dtype: D[r] = sum_c exp((s_rc - row_off[r]) - col_off[c]) Y[c]; an offset of None is 0, +inf is legal"""
    X, Y = np.asarray(X, dtype=dtype), np.asarray(Y, dtype=dtype)
    ro, co = _offsets(len(X), len(Y), row_off, col_off, dtype)
    with np.errstate(under='ignore'):
        if np.dtype(dtype) == np.float64:
            return np.exp((X @ Y.T - ro[:, None]) - co[None, :]) @ Y
        D = np.zeros(X.shape, dtype=np.float64)
        for first in range(0, len(Y), slab):
            Ys = Y[first:first + slab]
            P = np.exp((_scores32(X, Ys) - ro[:, None]) - co[None, first:first + slab])
            part = np.zeros(X.shape, dtype=np.float32)
            for c in range(len(Ys)):                              # a chain over the slab's rows
                part += P[:, c:c + 1] * Ys[c]
            D += part
    return D.astype(np.float32)


def _like_sum(x, y, dtype):
    """-> (L, sum s) over the rows y, a chain in stored order"""
    L = np.zeros(len(x), dtype=dtype)
    ss = 0.0
    for row in y:
        L += row
        ss += float(np.dot(x, row).astype(dtype))
    return L, ss


def like_sums(X, Y, rows_likes, dtype=np.float64, heavy_from=NO_HEAVY):
    """-> (L [n_x, K] in dtype, ss float64 [n_x])"""
    X, Y = np.asarray(X, dtype=dtype), np.asarray(Y, dtype=dtype)
    K = Y.shape[1]
    Ls, sss = np.zeros(X.shape, dtype=dtype), np.zeros(len(X), dtype=np.float64)
    for r, likes in enumerate(rows_likes):
        y = Y[np.asarray(likes, dtype=np.int64)]
        if np.dtype(dtype) == np.float32 and len(likes) > heavy_from:
            acc = np.zeros((HEAVY_WAVES, K + 1), dtype=np.float64)
            for j, first in enumerate(range(0, len(y), LIKE_SLAB)):
                L, ss = _like_sum(X[r], y[first:first + LIKE_SLAB], dtype)
                acc[j % HEAVY_WAVES] += np.concatenate([L.astype(np.float64), [ss]])
            total = np.zeros(K + 1, dtype=np.float64)
            for w in range(HEAVY_WAVES):
                total += acc[w]
            Ls[r], sss[r] = total[:K].astype(dtype), total[K]
        else:
            Ls[r], sss[r] = _like_sum(X[r], y, dtype)
    return Ls, sss


def step_rows(X, H, Y, D, rows_likes, *, fixed, scale_by_likes, lam, lr, dtype=np.float64, heavy_from=NO_HEAVY):
    """-> (X_new, H_new, row_loss float64): row_loss[r] = -sum_likes s + 1/2 lam |x_r non-fixed|^2 at the X that came in; fixed = -1:
    no column is fixed.  A like listed twice counts twice"""
    dt = np.dtype(dtype).type
    D = np.asarray(D, dtype=dtype)
    Xn, Hn = np.array(X, dtype=dtype), np.array(H, dtype=dtype)
    free = np.arange(Xn.shape[1]) != fixed
    L, ss = like_sums(Xn, Y, rows_likes, dtype, heavy_from)
    w = np.asarray([len(x) if scale_by_likes else 1 for x in rows_likes], dtype=np.float64)[:, None]
    g = (L.astype(np.float64) - w * D.astype(np.float64) - lam * Xn.astype(np.float64)).astype(dtype)
    hn = (g * g + Hn).astype(dtype)
    xn = (Xn + (dt(lr) * g) / np.sqrt(hn)).astype(dtype)
    loss = -ss + 0.5 * lam * (Xn[:, free].astype(np.float64) ** 2).sum(axis=1)
    Xn[:, free], Hn[:, free] = xn[:, free], hn[:, free]
    return Xn, Hn, loss


def gradient(X, Y, rows_likes, *, fixed, scale_by_likes, row_off=None, col_off=None, lam):
    """float64 -> g [n_x, K] = L - w D - lam x, zero in the fixed column: minus the derivative of F by the rows of X"""
    X = np.asarray(X, dtype=np.float64)
    D = dense_rows(X, Y, row_off, col_off)
    L = like_sums(X, Y, rows_likes)[0]
    w = np.asarray([len(x) if scale_by_likes else 1 for x in rows_likes], dtype=np.float64)[:, None]
    g = L - w * D - lam * X
    if fixed >= 0:
        g[:, fixed] = 0
    return g


def counts(rows_likes):
    return np.asarray([len(x) for x in rows_likes], dtype=np.int64)


def item_offsets(lse, n_u, dtype=np.float64):
    """-> lse_u - log n_u in dtype; +inf for a user without likes"""
    with np.errstate(divide='ignore'):
        return (np.asarray(lse, dtype=dtype) - np.log(np.asarray(n_u).astype(dtype))).astype(dtype)


def half_step(X, H, Y, rows_likes, *, side, n_u=None, lam, lr, dtype=np.float64, heavy_from=NO_HEAVY):
    """side 'user': X the users, Y the items -> (X_new, H_new, sum_u n_u lse_u + sum of the row losses: F at the tables that came in,
    without 1/2 lam |Y|^2).  side 'item': X the items, Y the users, n_u the users' like counts -> (X_new, H_new, None)"""
    K = np.shape(X)[1]
    if side == 'user':
        lse = lse_rows(X, Y, dtype)
        D = dense_rows(X, Y, row_off=lse, dtype=dtype)
        Xn, Hn, rl = step_rows(X, H, Y, D, rows_likes, fixed=K - 1, scale_by_likes=True, lam=lam, lr=lr, dtype=dtype, heavy_from=heavy_from)
        return Xn, Hn, float((counts(rows_likes) * lse.astype(np.float64)).sum() + rl.sum())
    lse = lse_rows(Y, X, dtype)
    D = dense_rows(X, Y, col_off=item_offsets(lse, n_u, dtype), dtype=dtype)
    Xn, Hn, _ = step_rows(X, H, Y, D, rows_likes, fixed=-1, scale_by_likes=False, lam=lam, lr=lr, dtype=dtype, heavy_from=heavy_from)
    return Xn, Hn, None


def loss(Xa, Ya, user_likes, *, lam):
    """the float64 objective written out; Xa [n_users, K] with its column of ones, Ya [n_items, K]"""
    Xa, Ya = np.asarray(Xa, dtype=np.float64), np.asarray(Ya, dtype=np.float64)
    S = Xa @ Ya.T
    m = S.max(axis=1)
    lse = m + np.log(np.exp(S - m[:, None]).sum(axis=1))
    liked = sum(float(S[u, np.asarray(likes, dtype=np.int64)].sum()) for u, likes in enumerate(user_likes))
    return float((counts(user_likes) * lse).sum()) - liked + 0.5 * lam * float((Xa[:, :-1] ** 2).sum() + (Ya ** 2).sum())


def init(n_users, n_items, k, seed):
    """-> (Xa fp32 [n_users, k + 1], Ya fp32 [n_items, k + 1]): the users' factors drawn first, then the items', N(0, 0.01); biases 0"""
    rng = np.random.Generator(np.random.PCG64(seed))
    Xa = np.ones((n_users, k + 1), dtype=np.float32)
    Ya = np.zeros((n_items, k + 1), dtype=np.float32)
    Xa[:, :k] = rng.standard_normal((n_users, k), dtype=np.float32) * np.float32(0.01)
    Ya[:, :k] = rng.standard_normal((n_items, k), dtype=np.float32) * np.float32(0.01)
    return Xa, Ya


def train(Xa, Ya, user_likes, item_likes, *, lam, lr, max_iter, dtype=np.float64, Hx=None, Hy=None):
    """-> (Xa, Ya, Hx, Hy, losses): per iteration a user half-step, then an item half-step against the moved users; the logged loss
    is F at the tables entering the iteration"""
    Xa, Ya = np.array(Xa, dtype=dtype), np.array(Ya, dtype=dtype)
    Hx = np.ones_like(Xa) if Hx is None else np.array(Hx, dtype=dtype)
    Hy = np.ones_like(Ya) if Hy is None else np.array(Hy, dtype=dtype)
    n_u = counts(user_likes)
    losses = []
    for _ in range(max_iter):
        reg_y = 0.5 * lam * float((Ya.astype(np.float64) ** 2).sum())
        Xa, Hx, part = half_step(Xa, Hx, Ya, user_likes, side='user', lam=lam, lr=lr, dtype=dtype)
        Ya, Hy, _ = half_step(Ya, Hy, Xa, item_likes, side='item', n_u=n_u, lam=lam, lr=lr, dtype=dtype)
        losses.append(part + reg_y)
    return Xa, Ya, Hx, Hy, losses


def fold_in(Ya, histories, *, steps, lam, lr, dtype=np.float64):
    """-> X [n_new, K]: `steps` user half-steps from zero rows (slots 1.0) against the frozen item table"""
    K = np.shape(Ya)[1]
    X = np.zeros((len(histories), K), dtype=dtype)
    X[:, K - 1] = 1
    H = np.ones_like(X)
    for _ in range(steps):
        X, H, _ = half_step(X, H, Ya, histories, side='user', lam=lam, lr=lr, dtype=dtype)
    return X


# ---- the inputs the tests share ------------------------------------------------------------------------------------------------------------
STEP_M = (0, 1, 2, 7, 65, 300, 700, 5)                  # likes per row: none, one, a wave's batch of 64 and one more, past heavy_from = 300


def step_inputs(k, n_y=41, seed=27):
    """-> (X fp32 [n_x, K], H, Y fp32 [n_y, K], rows_likes, D fp32 [n_x, K]): normal(0, 0.5) tables, slots in [1, 2), D in [0, 1); row r
    has STEP_M[r mod 8] likes, with repeats where that is more than n_y"""
    rng = np.random.Generator(np.random.PCG64([seed, k]))
    K, n_x = k + 1, 2 * len(STEP_M) + 1
    X = (rng.standard_normal((n_x, K)) * 0.5).astype(np.float32)
    Y = (rng.standard_normal((n_y, K)) * 0.5).astype(np.float32)
    X[:, k] = 1
    H = (1 + rng.random((n_x, K))).astype(np.float32)
    D = rng.random((n_x, K)).astype(np.float32)
    rows = []
    for r in range(n_x):
        m = STEP_M[r % len(STEP_M)]
        rows.append(rng.integers(0, n_y, m) if m > n_y else rng.permutation(n_y)[:m])
    return X, H, Y, rows, D


E2E = dict(k=8, lam=0.01, lr=0.1, seed=0, iters=5)      # end to end on tests/golden/g2
