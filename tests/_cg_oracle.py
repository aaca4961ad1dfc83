"""NumPy restatement of K24 (the ALS half-step by conjugate gradients), written from the recurrence of include/tkr.h at tkr_als_cg_rows:

    A v = G v + (a - b) sum_y (y . v) y + ridge v          b = a sum_y y + w_prior prior
    x <- X[r];  r <- b - A x;  p <- r;  rho <- r . r
    `steps` times, unless rho < 1e-20:  q <- A p;  alpha <- rho / (p . q);  x <- x + alpha p;  r <- r - alpha q;  rho' <- r . r;
                                         p <- r + (rho' / rho) p;  rho <- rho'
    row_loss = 1/2 x . (A - ridge I) x - a sum_y y . x + 1/2 a |L_r|  (+ 1/2 w_prior |x - prior|^2; a row without likes: that term alone)

dtype float64 is the reference the GPU tests measure against: the recurrence in float64 with NumPy's own dot products.  dtype float32
is the yardstick for its error AND the kernel's stated order, every operation rounded on its own:
  * G v: per element one fma chain over the columns j ascending from +0.0;
  * a dot product: the vector padded with zeros to 64 lanes x KC, lane l chains its elements l, l + 64, .. by fma from +0.0, then
    s += s[lane ^ 32], ^ 16, .. ^ 1;
  * s = sum_y t_y y: one fma chain per component over the likes in stored order, t_y = y . v;
  * A v = fp32(G v + w_like s + ridge v), b = fp32(a sum y + w_prior prior): the terms in float64, rounded once;
  * alpha, beta: float32 divisions; the three updates are fmas.
An fma is float32(float64(a) * float64(b) + float64(c)): the product is exact in float64, the sum rounds twice, which differs from a
true fma in rare last-bit cases and is far inside what the tests allow (they hold the kernel to a multiple of this oracle's own error)."""
import numpy as np

from _als_oracle import SOLVE_M, gram, solve_inputs, to_csr  # noqa: F401  (the shared inputs: imported, not copied)

DONE = 1e-20


def _fma(a, b, c):
    return (np.asarray(a, np.float64) * np.asarray(b, np.float64) + np.asarray(c, np.float64)).astype(np.float32)


def dot32(a, b):
    """the kernel's one dot product: float32 [.., k] x float32 [.., k] -> float32 [..]"""
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    k = a.shape[-1]
    kc = (k + 63) // 64
    pa, pb = np.zeros(a.shape[:-1] + (64 * kc,), np.float32), np.zeros(a.shape[:-1] + (64 * kc,), np.float32)
    pa[..., :k], pb[..., :k] = a, b
    s = np.zeros(a.shape[:-1] + (64,), np.float32)
    for c in range(kc):
        s = _fma(pa[..., 64 * c:64 * c + 64], pb[..., 64 * c:64 * c + 64], s)
    lanes = np.arange(64)
    d = 32
    while d >= 1:
        s = (s + s[..., lanes ^ d]).astype(np.float32)
        d >>= 1
    return s[..., 0]


class _Rows:
    """the operators of all rows of a call, in the arithmetic of `dtype`: the rows move in step, as the kernel's tile does"""

    def __init__(self, G, ys, w_like, ridge, dtype):
        self.G, self.ys, self.w_like, self.ridge, self.exact = G, ys, float(w_like), float(ridge), np.dtype(dtype) == np.float64

    def dot(self, a, b):
        return np.einsum('ij,ij->i', a, b) if self.exact else dot32(a, b)

    def apply(self, V, ridge=True):
        """-> (A_r v_r for every row, [t_y] per row); ridge=False: (A_r - ridge I) v_r"""
        if self.exact:
            T = [y @ v for y, v in zip(self.ys, V)]
            Q = V @ self.G + self.w_like * np.stack([t @ y for t, y in zip(T, self.ys)])
            return (Q + self.ridge * V if ridge else Q), T
        gq = np.zeros(V.shape, np.float32)
        for j in range(V.shape[1]):
            gq = _fma(V[:, j:j + 1], self.G[j][None, :], gq)
        S, T = np.zeros(V.shape, np.float32), []
        for r, (y, v) in enumerate(zip(self.ys, V)):
            t = np.zeros(len(y), np.float32)
            s = S[r]
            for e, row in enumerate(y):
                t[e] = dot32(row, v)
                s = _fma(t[e], row, s)
            S[r] = s
            T.append(t)
        Q = gq.astype(np.float64) + self.w_like * S.astype(np.float64)
        if ridge:
            Q = Q + self.ridge * V.astype(np.float64)
        return Q.astype(np.float32), T


def cg_half_step(X0, Y, rows_likes, rated, *, a, b, ridge_in_G, ridge, steps, dtype=np.float64, prior=None, w_prior=0.0, G=None, done=DONE):
    """-> (X_new, row_loss float64).  The arguments of _als_oracle.half_step, and: steps; prior [n_x, k] and w_prior (every row is then
    solved); G: the shared Gram when the caller has it already (the GPU's, so that only the solve is compared).  A like outside the
    table is skipped; a row the kernel refuses (p . q not positive and finite) is left as it came in with loss 0.  done: the recurrence's
    exit rho < done, the kernel's 1e-20; 0 runs every step while a residual is left (the float64 statement of finite termination)."""
    dt = np.dtype(dtype).type
    Y = np.asarray(Y, dtype=dtype)
    Xn = np.array(X0, dtype=dtype)
    k = Y.shape[1]
    if G is None:
        G = gram(Y, rated, b, ridge_in_G, dtype)
    G = np.asarray(G, dtype=dtype)
    w_like, w_rhs = float(a) - float(b), float(a)
    loss = np.zeros(len(rows_likes), dtype=np.float64)
    at, ys = [], []
    for r, likes in enumerate(rows_likes):
        likes = np.asarray(likes, dtype=np.int64)
        valid = likes[(likes >= 0) & (likes < len(Y))]
        if len(valid) == 0 and (prior is None or len(likes) > 0):
            continue
        at.append(r)
        ys.append(Y[valid])
    if not at:
        return Xn, loss
    op = _Rows(G, ys, w_like, ridge, dtype)
    rhs = np.zeros((len(at), k), np.float64)
    for i, y in enumerate(ys):
        for row in y:
            rhs[i] = rhs[i] + row.astype(np.float64)
    rhs = w_rhs * rhs
    if prior is not None:
        pr = np.asarray(prior, dtype=dtype)[at]
        rhs = rhs + float(w_prior) * pr.astype(np.float64)
    rhs = rhs.astype(dtype)
    with np.errstate(all='ignore'):
        x = Xn[at].copy()
        res = (rhs - op.apply(x)[0]).astype(dtype)
        p = res.copy()
        rho = op.dot(res, res).astype(dtype)
        refused = np.zeros(len(at), bool)
        for _ in range(steps):
            active = ~refused & ~((rho < done) | (rho == 0))
            if not active.any():
                break
            q = op.apply(p)[0]
            pq = op.dot(p, q).astype(dtype)
            refused |= active & ~((pq > 0) & np.isfinite(pq))
            go = active & ~refused
            alpha = (rho / pq).astype(dtype)[:, None]
            if op.exact:
                x2, res2 = x + alpha * p, res - alpha * q
            else:
                x2, res2 = _fma(alpha, p, x), _fma(-alpha, q, res)
            rho2 = op.dot(res2, res2).astype(dtype)
            beta = (rho2 / rho).astype(dtype)[:, None]
            p2 = res2 + beta * p if op.exact else _fma(beta, p, res2)
            x[go], res[go], p[go], rho[go] = x2[go], res2[go], p2[go], rho2[go]
        refused |= ~np.isfinite(x).all(axis=1)
        q, T = op.apply(np.where(refused[:, None], dt(0), x), ridge=False)
    for i, r in enumerate(at):
        if refused[i]:
            continue
        Xn[r] = x[i]
        x64 = x[i].astype(np.float64)
        if len(ys[i]):
            loss[r] = (0.5 * float(np.dot(x64, q[i].astype(np.float64))) - w_rhs * float(T[i].astype(np.float64).sum())) + 0.5 * w_rhs * len(ys[i])
        if prior is not None:
            loss[r] += 0.5 * float(w_prior) * float(((x64 - pr[i].astype(np.float64)) ** 2).sum())
    return Xn, loss


def iteration_cg(U, V, user_likes, item_likes, *, a, b, lu, lv, steps, dtype=np.float64):
    """_als_oracle.iteration with the half-step above"""
    u_rated = [u for u, l in enumerate(user_likes) if len(l)]
    i_rated = [i for i, l in enumerate(item_likes) if len(l)]
    U, _ = cg_half_step(U, V, user_likes, i_rated, a=a, b=b, ridge_in_G=lu, ridge=0.0, steps=steps, dtype=dtype)
    V, rl = cg_half_step(V, U, item_likes, u_rated, a=a, b=b, ridge_in_G=0.0, ridge=lv, steps=steps, dtype=dtype)
    loss = rl.sum() + 0.5 * lu * (U.astype(np.float64) ** 2).sum() + 0.5 * lv * (V.astype(np.float64) ** 2).sum()
    return U, V, float(loss)


def train_cg(U, V, user_likes, item_likes, *, a, b, lu, lv, max_iter, tol, steps=3, dtype=np.float64):
    """_als_oracle.train with the half-step above -> (U, V, losses)"""
    U, V = np.array(U, dtype=dtype), np.array(V, dtype=dtype)
    loss, losses = np.exp(50), []
    for _ in range(max_iter):
        loss_old = loss
        U, V, loss = iteration_cg(U, V, user_likes, item_likes, a=a, b=b, lu=lu, lv=lv, steps=steps, dtype=dtype)
        losses.append(loss)
        if abs(loss_old - loss) / loss_old < tol:
            break
    return U, V, losses


def cer_train_cg(U, V, E, F, user_likes, item_likes, *, a, b, lu, lv, le, max_iter, tol, steps=3, dtype=np.float64):
    """_cer_oracle.cer_train with the half-step above (the prior on every item row, the E-step as it is) -> (U, V, E, losses)"""
    from _cer_oracle import e_step
    U, V, E = np.array(U, dtype=dtype), np.array(V, dtype=dtype), np.array(E, dtype=dtype)
    u_rated = [u for u, l in enumerate(user_likes) if len(l)]
    i_rated = [i for i, l in enumerate(item_likes) if len(l)]
    loss, losses = np.exp(50), []
    for _ in range(max_iter):
        loss_old = loss
        Fe = (np.asarray(F, dtype=dtype) @ E).astype(dtype)
        U, _ = cg_half_step(U, V, user_likes, i_rated, a=a, b=b, ridge_in_G=lu, ridge=0.0, steps=steps, dtype=dtype)
        V, rl = cg_half_step(V, U, item_likes, u_rated, a=a, b=b, ridge_in_G=0.0, ridge=lv, steps=steps, dtype=dtype, prior=Fe, w_prior=lv)
        E = e_step(F, V, lv=lv, le=le, dtype=dtype)
        loss = float(rl.sum() + 0.5 * lu * (U.astype(np.float64) ** 2).sum() + 0.5 * le * (E.astype(np.float64) ** 2).sum())
        losses.append(loss)
        if abs(loss_old - loss) / loss_old < tol:
            break
    Fe = (np.asarray(F, dtype=dtype) @ E).astype(dtype)
    for j, likes in enumerate(item_likes):
        if len(likes) == 0:
            V[j] = Fe[j]
    return U, V, E, losses
