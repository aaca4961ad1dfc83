"""NumPy restatement of K20 (implicit-feedback ALS, WMF), written from the equations of DESIGN.md section 4 K20:

    G   = scale * sum over the rated rows y of Y of  y y^T  (+ ridge_in_G * I)
    x_r = (G + (a - b) * sum_{y in L_r} y y^T + ridge * I)^-1  (a * sum_{y in L_r} y)            for every row r with likes
    row_loss_r = 1/2 x^T A x - a * sum y.x + 1/2 a |L_r|        A = the system's matrix without `ridge`

Every stored like counts r = 1, a like listed twice counts twice, rows without likes are left as they are.  dtype float64 is the
reference the GPU tests measure against; dtype float32 is the yardstick for its error: the same system formed with `@` and solved
with np.linalg.solve, everything in float32."""
import numpy as np


def csr_rows(ptr, cols):
    """(ptr, cols) -> a list of int arrays, one per row"""
    ptr = np.asarray(ptr, dtype=np.int64)
    cols = np.asarray(cols, dtype=np.int64)
    return [cols[ptr[r]:ptr[r + 1]] for r in range(len(ptr) - 1)]


def gram(Y, rows, scale, ridge, dtype=np.float64):
    dt = np.dtype(dtype).type
    Yr = np.asarray(Y, dtype=dtype)[np.asarray(rows, dtype=np.int64)]
    k = Y.shape[1]
    return (dt(scale) * (Yr.T @ Yr) + dt(ridge) * np.eye(k, dtype=dtype)).astype(dtype)


def half_step(X, Y, rows_likes, rated, *, a, b, ridge_in_G, ridge, dtype=np.float64, G=None):
    """-> (X_new, row_loss).  rows_likes: per row of X the rows of Y it likes (repeats allowed); rated: the rows of Y in the shared Gram.
    The system of row r is G + ridge_in_G I + (a - b) sum y y^T + ridge I; the loss is taken with A = that matrix without `ridge`
    (wmf.py:88-96: the item step's A holds no regulariser; the user step computes no row loss, and none is asked of it).
    G: the shared Gram (with ridge_in_G) when the caller has it already, e.g. the GPU's, so that only the solve is compared."""
    dt = np.dtype(dtype).type
    Y = np.asarray(Y, dtype=dtype)
    Xn = np.array(X, dtype=dtype)
    k = Y.shape[1]
    if G is None:
        G = gram(Y, rated, b, ridge_in_G, dtype)
    G = np.asarray(G, dtype=dtype)
    eye = np.eye(k, dtype=dtype)
    loss = np.zeros(len(rows_likes), dtype=np.float64)
    for r, likes in enumerate(rows_likes):
        if len(likes) == 0:
            continue
        y = Y[np.asarray(likes, dtype=np.int64)]
        A = (G + dt(a - b) * (y.T @ y)).astype(dtype)
        rhs = (dt(a) * y.sum(axis=0)).astype(dtype)
        x = np.linalg.solve(A + dt(ridge) * eye, rhs).astype(dtype)
        Xn[r] = x
        loss[r] = float(dt(0.5) * (x @ A @ x) - dt(a) * (y @ x).sum() + dt(0.5) * dt(a) * dt(len(likes)))
    return Xn, loss


def loss_dense(U, V, R, u_rated, i_rated, *, a, b, lu, lv):
    """the dense float64 objective: 1/2 sum over rated u x rated i of c_ui (r_ui - u.v)^2 + 1/2 lu |U|^2 + 1/2 lv |V|^2, with R[u, i] =
    the number of times the like is listed: a like listed n times is n observations r = 1 at weight a in place of ONE r = 0 at weight
    b, which is what `G + (a - b) sum` over a list with repeats states"""
    U, V, R = (np.asarray(x, dtype=np.float64) for x in (U, V, R))
    u_rated, i_rated = np.asarray(u_rated, dtype=np.int64), np.asarray(i_rated, dtype=np.int64)
    P = U[u_rated] @ V[i_rated].T
    Rr = R[np.ix_(u_rated, i_rated)]
    fit = 0.5 * (Rr * (a * (1.0 - P) ** 2 - b * P ** 2) + b * P ** 2).sum()
    return fit + 0.5 * lu * (U ** 2).sum() + 0.5 * lv * (V ** 2).sum()


def dense_counts(rows_likes, n_cols):
    R = np.zeros((len(rows_likes), n_cols), dtype=np.float64)
    for r, likes in enumerate(rows_likes):
        np.add.at(R[r], np.asarray(likes, dtype=np.int64), 1.0)
    return R


def iteration(U, V, user_likes, item_likes, *, a, b, lu, lv, dtype=np.float64):
    """one iteration -> (U, V, loss): users against V (lu inside the Gram, wmf.py:71-72), then items against the NEW U, the loss from
    the item rows plus both regularisers over ALL rows"""
    u_rated = [u for u, l in enumerate(user_likes) if len(l)]
    i_rated = [i for i, l in enumerate(item_likes) if len(l)]
    U, _ = half_step(U, V, user_likes, i_rated, a=a, b=b, ridge_in_G=lu, ridge=0.0, dtype=dtype)
    V, rl = half_step(V, U, item_likes, u_rated, a=a, b=b, ridge_in_G=0.0, ridge=lv, dtype=dtype)
    loss = rl.sum() + 0.5 * lu * (U.astype(np.float64) ** 2).sum() + 0.5 * lv * (V.astype(np.float64) ** 2).sum()
    return U, V, float(loss)


def train(U, V, user_likes, item_likes, *, a, b, lu, lv, max_iter, tol, dtype=np.float64):
    """the loop of wmf.py:62,98-101 -> (U, V, losses)"""
    U, V = np.array(U, dtype=dtype), np.array(V, dtype=dtype)
    loss, losses = np.exp(50), []
    for _ in range(max_iter):
        loss_old = loss
        U, V, loss = iteration(U, V, user_likes, item_likes, a=a, b=b, lu=lu, lv=lv, dtype=dtype)
        losses.append(loss)
        if abs(loss_old - loss) / loss_old < tol:
            break
    return U, V, losses


# ---- the inputs the tests share (tests/test_als_cpu.py states their premises without a GPU, tests/test_gpu_als.py runs them) -------------
SOLVE_M = (0, 1, 2, 7, 8, 9, 31, 32, 33, 45, 60)         # likes per row: around heavy_from = 8, around the 32-row tile, every column, repeats
SOLVE_A, SOLVE_B = 1.0, 0.01


def solve_inputs(k, n_x=37, n_y=45, seed=20):
    """-> (Y fp32 [n_y, k], X0 fp32 [n_x, k], rows_likes, rated): uniform [0, 1) tables; row r has SOLVE_M[r mod 11] likes (n_x = 1: 33),
    distinct columns except the rows of 60, which repeat some; rated = the columns somebody likes"""
    rng = np.random.Generator(np.random.PCG64([seed, k, n_x]))
    Y = rng.random((n_y, k), dtype=np.float32)
    X0 = rng.random((n_x, k), dtype=np.float32)
    rows = []
    for r in range(n_x):
        m = 33 if n_x == 1 else SOLVE_M[r % len(SOLVE_M)]
        rows.append(rng.integers(0, n_y, m) if m > n_y else rng.permutation(n_y)[:m])
    rated = sorted({int(c) for likes in rows for c in likes})
    return Y, X0, rows, rated


def to_csr(rows_likes):
    ptr = np.zeros(len(rows_likes) + 1, dtype=np.int64)
    np.cumsum([len(x) for x in rows_likes], out=ptr[1:])
    cols = np.concatenate([np.asarray(x, dtype=np.int32) for x in rows_likes] + [np.zeros(0, np.int32)]).astype(np.int32)
    return ptr, cols


E2E = dict(k=16, lu=0.1, lv=0.1, seed=0, iters=6)         # test 5: als.WMF on tests/golden/g2
