"""NumPy restatement of K26 (csrc/sparse.hip), written from the contract of include/tkr.h at tkr_csr_spmm and tkr_estep_cg:

    out[r] = fp32(alpha * s_r + beta * Z[r]),   s_r = sum over row r's nonzeros e of val[e] * X[col[e]]
    B = lv F^T V;  R = B - (lv F^T (F E) + le E);  P = R;  rho_c = R_c . R_c
    `steps` times, in the columns with rho_c >= 1e-20:  T = F P;  Q = lv F^T T + le P;  alpha_c = rho_c / (P_c . Q_c);  E_c += alpha_c P_c;
                                                         R_c -= alpha_c Q_c;  rho'_c = R_c . R_c;  P_c = R_c + (rho'_c / rho_c) P_c

dtype float64 is the reference the GPU tests measure against: the same recurrence with NumPy's own products.  dtype float32 is the
yardstick for its error AND the kernel's stated order, every operation rounded on its own:
  * a row of at most heavy_from nonzeros: one fma chain per component over its nonzeros in stored order from +0.0;
  * a longer row: slabs of 256 nonzeros in stored order, each slab that chain, the slab sums added in ascending order in float64;
  * alpha * s + beta * z in float64, rounded once;
  * a dot product of a column: slabs of 1024 rows, a slab 16 runs of 64 rows; a run is an fma chain from +0.0 over its rows, the 16 run
    sums are added in ascending order in float32, the slabs' partials in ascending order in float64, rounded once;
  * R = B - W is a float32 subtraction, alpha and beta float32 divisions, the three updates fmas.
An fma is _cg_oracle._fma: float32(float64(a) * float64(b) + float64(c))."""
import functools

import numpy as np
import scipy.sparse as ss

from _als_oracle import csr_rows, half_step  # noqa: F401  (the shared inputs and the row solve: imported, not copied)
from _cer_oracle import E2E, cer_train, e2e_features, e2e_start, e_step, half_step_prior  # noqa: F401
from _cg_oracle import _fma

DONE = 1e-20
SPMM_SLAB, HEAVY_FROM, DOT_SLAB, DOT_RUNS, DOT_RUN = 256, 2048, 1024, 16, 64


def _chains(ptr, col, val, X, first, count):
    """the fp32 chain of every segment [first[i], first[i] + count[i]) of the nonzeros -> float32 [segments, k]"""
    s = np.zeros((len(first), X.shape[1]), np.float32)
    for e in range(int(count.max()) if len(count) else 0):
        on = np.flatnonzero(count > e)
        at = first[on] + e
        s[on] = _fma(val[at][:, None], X[col[at]], s[on])
    return s


def spmm(A, X, alpha=1.0, Z=None, beta=0.0, heavy_from=HEAVY_FROM, dtype=np.float64):
    """A: a scipy CSR (its stored order is the order of the chain) -> [n_rows, k] of `dtype`"""
    A = A.tocsr()
    if np.dtype(dtype) == np.float64:
        out = float(alpha) * (A.astype(np.float64) @ np.asarray(X, np.float64))
        return out if Z is None else out + float(beta) * np.asarray(Z, np.float64)
    ptr, col, val = A.indptr.astype(np.int64), A.indices.astype(np.int64), A.data.astype(np.float32)
    X = np.asarray(X, np.float32)
    m = np.diff(ptr)
    s = np.zeros((A.shape[0], X.shape[1]), np.float64)
    light = np.flatnonzero(m <= heavy_from)
    s[light] = _chains(ptr, col, val, X, ptr[light], m[light]).astype(np.float64)
    for r in np.flatnonzero(m > heavy_from):
        first = np.arange(ptr[r], ptr[r + 1], SPMM_SLAB)
        slabs = _chains(ptr, col, val, X, first, np.minimum(SPMM_SLAB, ptr[r + 1] - first))
        for slab in slabs:                                         # ascending, in float64
            s[r] = s[r] + slab.astype(np.float64)
    out = float(alpha) * s
    if Z is not None:
        out = out + float(beta) * np.asarray(Z, np.float32).astype(np.float64)
    return out.astype(np.float32)


def dot_columns(A, B, dtype=np.float64):
    """[d, k] x [d, k] -> [k]: the column dot products, in float32 by the kernel's one tree"""
    if np.dtype(dtype) == np.float64:
        return np.einsum('ij,ij->j', np.asarray(A, np.float64), np.asarray(B, np.float64))
    A, B = np.asarray(A, np.float32), np.asarray(B, np.float32)
    d, k = A.shape
    n_slabs = (d + DOT_SLAB - 1) // DOT_SLAB
    pa, pb = np.zeros((n_slabs * DOT_SLAB, k), np.float32), np.zeros((n_slabs * DOT_SLAB, k), np.float32)
    pa[:d], pb[:d] = A, B                                          # (a row past d adds fma(0, 0, s) = s: no chain is ever -0.0)
    pa, pb = pa.reshape(n_slabs, DOT_RUNS, DOT_RUN, k), pb.reshape(n_slabs, DOT_RUNS, DOT_RUN, k)
    runs = np.zeros((n_slabs, DOT_RUNS, k), np.float32)
    for i in range(DOT_RUN):
        runs = _fma(pa[:, :, i], pb[:, :, i], runs)
    part = runs[:, 0]
    for j in range(1, DOT_RUNS):
        part = (part + runs[:, j]).astype(np.float32)
    total = np.zeros(k, np.float64)
    for b in range(n_slabs):
        total = total + part[b].astype(np.float64)
    return total.astype(np.float32)


def estep_cg(F, V, E0, *, lv, le, steps, heavy_from=HEAVY_FROM, dtype=np.float64, done=DONE, Ft=None):
    """-> (E, refused): `steps` steps from E0; refused: the columns whose p . q was not positive and finite (they hold E0)"""
    F = F.tocsr()
    Ft = canonical(F.T) if Ft is None else Ft
    exact = np.dtype(dtype) == np.float64
    V, E0 = np.asarray(V, dtype), np.asarray(E0, dtype)
    mm = functools.partial(spmm, heavy_from=heavy_from, dtype=dtype)
    with np.errstate(all='ignore'):
        B = mm(Ft, V, alpha=lv)
        W = mm(Ft, mm(F, E0), alpha=lv, Z=E0, beta=le)
        X, R = E0.copy(), (B - W).astype(dtype)
        P = R.copy()
        rho = dot_columns(R, R, dtype)
        refused = np.zeros(E0.shape[1], bool)
        for _ in range(steps):
            on = ~refused & (rho >= done)
            Q = mm(Ft, mm(F, P), alpha=lv, Z=P, beta=le)
            pq = dot_columns(P, Q, dtype)
            refused |= on & ~((pq > 0) & np.isfinite(pq))
            on &= ~refused
            alpha = np.where(on, rho / pq, 0).astype(dtype)
            if exact:
                X2, R2 = X + alpha * P, R - alpha * Q
            else:
                X2, R2 = _fma(alpha, P, X), _fma(-alpha, Q, R)
            rho2 = dot_columns(R2, R2, dtype)
            beta = (rho2 / rho).astype(dtype)
            P2 = R2 + beta * P if exact else _fma(beta, P, R2)
            X[:, on], R[:, on], P[:, on], rho[on] = X2[:, on], R2[:, on], P2[:, on], rho2[on]
    X[:, refused] = E0[:, refused]
    return X, refused


def canonical(m):
    m = ss.csr_matrix(m, dtype=np.float32, copy=True)
    m.sum_duplicates()
    m.eliminate_zeros()
    m.sort_indices()
    return m


def cer_train_cg_estep(U, V, E, F, user_likes, item_likes, *, a, b, lu, lv, le, max_iter, tol, e_steps, heavy_from=HEAVY_FROM, dtype=np.float64):
    """_cer_oracle.cer_train with Fe = F E the sparse product and the E-step e_steps steps from the E before -> (U, V, E, losses)"""
    F = canonical(F)
    Ft = canonical(F.T)
    U, V, E = np.array(U, dtype=dtype), np.array(V, dtype=dtype), np.array(E, dtype=dtype)
    u_rated = [u for u, l in enumerate(user_likes) if len(l)]
    i_rated = [i for i, l in enumerate(item_likes) if len(l)]
    loss, losses = np.exp(50), []
    for _ in range(max_iter):
        loss_old = loss
        Fe = spmm(F, E, heavy_from=heavy_from, dtype=dtype)
        U, _ = half_step(U, V, user_likes, i_rated, a=a, b=b, ridge_in_G=lu, ridge=0.0, dtype=dtype)
        V, rl = half_step_prior(V, U, item_likes, u_rated, Fe, a=a, b=b, ridge_in_G=0.0, ridge=lv, w_prior=lv, dtype=dtype)
        E, _ = estep_cg(F, V, E, lv=lv, le=le, steps=e_steps, heavy_from=heavy_from, dtype=dtype, Ft=Ft)
        loss = float(rl.sum() + 0.5 * lu * (U.astype(np.float64) ** 2).sum() + 0.5 * le * (E.astype(np.float64) ** 2).sum())
        losses.append(loss)
        if abs(loss_old - loss) / loss_old < tol:
            break
    Fe = spmm(F, E, heavy_from=heavy_from, dtype=dtype)
    for j, likes in enumerate(item_likes):
        if len(likes) == 0:
            V[j] = Fe[j]
    return U, V, E, losses


# ---- the inputs the tests share (tests/test_estep_cpu.py states their premises without a GPU, tests/test_gpu_estep.py runs them) ---------
N_ITEMS, PER_ROW, TEST_HEAVY_FROM = 300, 12, 64
GENERIC_D, GENERIC_K, GENERIC_STEPS = (1, 63, 400, 1025, 2100), (1, 16, 50, 128), (1, 3, 8)
GENERIC = dict(lv=0.1, le=1.0)
CONVERGE = ((10.0, 10e3, 8), (0.1, 1.0, 24))                         # (lv, le, steps): the reference's pair, and E2E's
CONVERGE_D, CONVERGE_K = 400, 16
WIDE = dict(d=200000, per_row=6, k=8, seed=27)


@functools.lru_cache(maxsize=None)
def features(d, n_items=N_ITEMS, per_row=PER_ROW, seed=26):
    """canonical fp32 CSR [n_items, d]: column 0 in every item (a row of n_items nonzeros in the transpose) and per_row more columns
    per item where d has them, values uniform (0, 1], every row scaled to unit length"""
    rng = np.random.Generator(np.random.PCG64([seed, d, n_items]))
    rows, cols = [], []
    for j in range(n_items):
        extra = rng.choice(d - 1, size=min(per_row, d - 1), replace=False) + 1 if d > 1 else np.zeros(0, np.int64)
        c = np.concatenate([[0], np.sort(extra)])
        rows.append(np.full(len(c), j))
        cols.append(c)
    rows, cols = np.concatenate(rows), np.concatenate(cols)
    F = ss.csr_matrix((1.0 - rng.random(len(rows)), (rows, cols)), shape=(n_items, d))
    F = ss.diags(1.0 / np.sqrt(np.asarray(F.multiply(F).sum(axis=1)).ravel())) @ F
    return canonical(F)


@functools.lru_cache(maxsize=None)
def tables(d, k, n_items=N_ITEMS, seed=28):
    """-> (V uniform [0, 1) fp32 [n_items, k], E0 standard normal fp32 [d, k]), read-only"""
    rng = np.random.Generator(np.random.PCG64([seed, d, k, n_items]))
    V, E0 = rng.random((n_items, k), dtype=np.float32), rng.standard_normal((d, k), dtype=np.float32)
    V.setflags(write=False)
    E0.setflags(write=False)
    return V, E0


@functools.lru_cache(maxsize=None)
def estep_case(d, k, steps, lv, le, heavy_from=TEST_HEAVY_FROM):
    """-> (E64, E32, refused64, refused32) of the shared inputs, computed once and read-only"""
    V, E0 = tables(d, k)
    F = features(d)
    e64, r64 = estep_cg(F, V, E0, lv=lv, le=le, steps=steps, heavy_from=heavy_from, dtype=np.float64)
    e32, r32 = estep_cg(F, V, E0, lv=lv, le=le, steps=steps, heavy_from=heavy_from, dtype=np.float32)
    for a in (e64, e32):
        a.setflags(write=False)
    return e64, e32, r64, r32


def cg_bound(F, lv, le, steps):
    """-> (kappa, 2 sqrt(kappa) ((sqrt(kappa) - 1) / (sqrt(kappa) + 1))^steps): the bound of conjugate gradients on the 2-norm of the
    error of a column, as a multiple of its start error, kappa from the eigenvalues of the dense system"""
    Fd = np.asarray(F.todense(), np.float64)
    w = np.linalg.eigvalsh(lv * (Fd.T @ Fd) + le * np.eye(Fd.shape[1]))
    kappa = w[-1] / w[0]
    return kappa, 2 * np.sqrt(kappa) * ((np.sqrt(kappa) - 1) / (np.sqrt(kappa) + 1)) ** steps


def wide_features(n_items):
    """features of width 200,000 for g2, a handful of nonzeros per item: the width the dense path cannot hold"""
    rng = np.random.Generator(np.random.PCG64(WIDE['seed']))
    rows = np.repeat(np.arange(n_items), WIDE['per_row'])
    cols = rng.integers(0, WIDE['d'], len(rows))
    return canonical(ss.csr_matrix((1.0 - rng.random(len(rows)), (rows, cols)), shape=(n_items, WIDE['d'])))
