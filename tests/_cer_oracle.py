"""NumPy restatement of K21 (content-aware ALS, CER), written from the equations of DESIGN.md section 4 K21 on top of _als_oracle:

    row r with likes:     x_r = (G + (a - b) sum y y^T + ridge I)^-1 (a sum y + w_prior p_r)
                          row_loss_r = 1/2 x^T A x - a sum y.x + 1/2 a |L_r| + 1/2 w_prior |x - p_r|^2     A = the matrix without `ridge`
    row r without likes:  x_r = (G + ridge I)^-1 (w_prior p_r),   row_loss_r = 1/2 w_prior |x - p_r|^2     (cer.py:61-63: no quadratic term)
    E = (lv F^T F + le I)^-1 (lv F^T V)
    loss = sum row_loss + 1/2 lu |U|^2 + 1/2 le |E|^2      the NEW E beside the Fe = F E_old that entered the item solve (cer.py:63-65)

dtype float64 is the reference the GPU tests measure against; dtype float32 the yardstick for its error: the same systems formed with
`@` and solved with np.linalg.solve, everything in float32."""
import numpy as np

from _als_oracle import csr_rows, gram, half_step, solve_inputs, to_csr  # noqa: F401  (the tests reach them through this module)


def half_step_prior(X, Y, rows_likes, rated, prior, *, a, b, ridge_in_G, ridge, w_prior, dtype=np.float64, G=None):
    """-> (X_new, row_loss): _als_oracle.half_step with the prior, every row solved"""
    dt = np.dtype(dtype).type
    Y = np.asarray(Y, dtype=dtype)
    P = np.asarray(prior, dtype=dtype)
    Xn = np.array(X, dtype=dtype)
    k = Y.shape[1]
    if G is None:
        G = gram(Y, rated, b, ridge_in_G, dtype)
    G = np.asarray(G, dtype=dtype)
    eye = np.eye(k, dtype=dtype)
    loss = np.zeros(len(rows_likes), dtype=np.float64)
    for r, likes in enumerate(rows_likes):
        if len(likes):
            y = Y[np.asarray(likes, dtype=np.int64)]
            A = (G + dt(a - b) * (y.T @ y)).astype(dtype)
            rhs = (dt(a) * y.sum(axis=0) + dt(w_prior) * P[r]).astype(dtype)
            x = np.linalg.solve(A + dt(ridge) * eye, rhs).astype(dtype)
            fit = float(dt(0.5) * (x @ A @ x) - dt(a) * (y @ x).sum() + dt(0.5) * dt(a) * dt(len(likes)))
        else:
            x = np.linalg.solve(G + dt(ridge) * eye, (dt(w_prior) * P[r]).astype(dtype)).astype(dtype)
            fit = 0.0
        Xn[r] = x
        loss[r] = fit + float(dt(0.5) * dt(w_prior) * ((x - P[r]) ** 2).sum())
    return Xn, loss


def e_step(F, V, *, lv, le, dtype=np.float64):
    F, V = np.asarray(F, dtype=dtype), np.asarray(V, dtype=dtype)
    dt = np.dtype(dtype).type
    FF = dt(lv) * (F.T @ F) + dt(le) * np.eye(F.shape[1], dtype=dtype)
    return np.linalg.solve(FF, dt(lv) * (F.T @ V)).astype(dtype)


def cer_iteration(U, V, E, F, user_likes, item_likes, *, a, b, lu, lv, le, dtype=np.float64):
    """one iteration of cer.py:33-65 -> (U, V, E, loss)"""
    u_rated = [u for u, l in enumerate(user_likes) if len(l)]
    i_rated = [i for i, l in enumerate(item_likes) if len(l)]
    Fe = (np.asarray(F, dtype=dtype) @ np.asarray(E, dtype=dtype)).astype(dtype)
    U, _ = half_step(U, V, user_likes, i_rated, a=a, b=b, ridge_in_G=lu, ridge=0.0, dtype=dtype)
    V, rl = half_step_prior(V, U, item_likes, u_rated, Fe, a=a, b=b, ridge_in_G=0.0, ridge=lv, w_prior=lv, dtype=dtype)
    E = e_step(F, V, lv=lv, le=le, dtype=dtype)
    loss = rl.sum() + 0.5 * lu * (U.astype(np.float64) ** 2).sum() + 0.5 * le * (E.astype(np.float64) ** 2).sum()
    return U, V, E, float(loss)


def cer_train(U, V, E, F, user_likes, item_likes, *, a, b, lu, lv, le, max_iter, tol, dtype=np.float64):
    """the loop of cer.py:24-73 -> (U, V, E, losses); after it every item without a like holds its row of F E"""
    U, V, E = np.array(U, dtype=dtype), np.array(V, dtype=dtype), np.array(E, dtype=dtype)
    loss, losses = np.exp(50), []
    for _ in range(max_iter):
        loss_old = loss
        U, V, E, loss = cer_iteration(U, V, E, F, user_likes, item_likes, a=a, b=b, lu=lu, lv=lv, le=le, dtype=dtype)
        losses.append(loss)
        if abs(loss_old - loss) / loss_old < tol:
            break
    Fe = (np.asarray(F, dtype=dtype) @ E).astype(dtype)
    for j, likes in enumerate(item_likes):
        if len(likes) == 0:
            V[j] = Fe[j]
    return U, V, E, losses


# ---- the inputs the tests share (tests/test_cer_cpu.py states their premises without a GPU, tests/test_gpu_cer.py runs them) -------------
E2E = dict(k=16, d=24, lu=0.1, lv=0.1, le=1.0, a=1.0, b=0.01, seed=0, iters=6, feat_seed=21, density=0.2)     # als.CER on tests/golden/g2


def e2e_features(n_items):
    """synthetic content for g2: fp32 [n_items, d], about a fifth of the entries nonzero, uniform (0, 1]"""
    rng = np.random.Generator(np.random.PCG64(E2E['feat_seed']))
    keep = rng.random((n_items, E2E['d'])) < E2E['density']
    return (keep * (1.0 - rng.random((n_items, E2E['d'])))).astype(np.float32)


def e2e_start(n_users, n_items, seed=None):
    """the start als.CER makes from one seed: fue, fie uniform [0, 1) as WMF draws them, then E standard normal from the same generator"""
    rng = np.random.Generator(np.random.PCG64(E2E['seed'] if seed is None else seed))
    U = rng.random((n_users, E2E['k']), dtype=np.float32)
    V = rng.random((n_items, E2E['k']), dtype=np.float32)
    return U, V, rng.standard_normal((E2E['d'], E2E['k']), dtype=np.float32)
