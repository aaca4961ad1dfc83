"""NumPy fp64 oracle of K23 (the SVM fusion).  The reference's old/methods/sfusion.py:28-63 hands the rows +d_t (label +1, t even) and
-d_t (label -1, t odd) to scikit-learn's LinearSVC(C=0.01): squared hinge, L2 penalty, the intercept regularised as one more feature of
value 1, coef_[0] returned.  This file RESTATES that objective and minimises it by Newton's method; nothing of the reference or of
scikit-learn is copied, and scikit-learn is not needed to run it (tests/golden/g10 holds its recorded fits).

In the space of margins row t (row g = first_row + t of the run) is x~ = (d, y), y = +1 for even g and -1 for odd g:
    z = w . d + y b,   f(w~) = |w~|^2 / 2 + C sum_t max(0, 1 - z_t)^2,   w~ = (w, b).
NumPy has no fma: z and the sums below round every product, where the kernel rounds once per fma.  On inputs whose products and sums
are exact in fp64 the two agree bit for bit; elsewhere the tests allow the bound of the sum length."""
import numpy as np

C1 = 1e-4                                    # Armijo: f(w + t p) <= f(w) + C1 t g.p
F_SLACK = 2.0 ** -40                         # ... up to the rounding of f itself, a relative 2^-40
MIN_STEP = 2.0 ** -30


def rows(D, first_row):
    """x~ fp64 [N, M + 1] = (d, y)"""
    D = np.asarray(D)
    y = np.where((first_row + np.arange(len(D))) % 2 == 0, 1.0, -1.0)
    return np.concatenate([D.astype(np.float64), y[:, None]], axis=1)


def _total(terms, order):
    """the sum over axis 0: 'forward' and 'backward' one term after the other, 'pairwise' NumPy's own tree; from +0.0"""
    if len(terms) == 0:
        return np.zeros(terms.shape[1:])
    if order == 'forward':
        return np.cumsum(terms, axis=0)[-1] + 0.0
    if order == 'backward':
        return np.cumsum(terms[::-1], axis=0)[-1] + 0.0
    assert order == 'pairwise'
    return np.sum(terms, axis=0) + 0.0


def margins(X, w):
    """z: the chain of include/tkr.h, m ascending, the intercept last"""
    z = np.zeros(len(X))
    for m in range(X.shape[1]):
        z = z + w[m] * X[:, m]
    return z


def sums(D, first_row, w, order='forward'):
    """-> (S [M + 1, M + 1], r [M + 1], q, count) over the active rows, 1 - z > 0 strictly"""
    X = rows(D, first_row)
    w = np.asarray(w, dtype=np.float64)
    a = 1.0 - margins(X, w)
    act = a > 0
    Xa, aa = X[act], a[act]
    S = _total(Xa[:, :, None] * Xa[:, None, :], order)
    r = _total(aa[:, None] * Xa, order)
    q = float(_total(aa * aa, order))
    return S, r, q, int(act.sum())


def objective(w, q, C):
    return 0.5 * float(np.dot(w, w)) + C * q


def newton(D, C, first_row=0, max_iter=50, order='forward'):
    """Newton's method from zeros with Armijo backtracking (halving); g = w~ - 2 C r, H = I + 2 C S, H p = -g; stops at
    max|g| <= 1e-12 max(1, C N).  -> dict(w [M + 1] (weights, then intercept), iterations, grad, active, objective, converged, H)"""
    D = np.asarray(D)
    N, M = D.shape
    tol = 1e-12 * max(1.0, C * N)
    w = np.zeros(M + 1)
    S, r, q, count = sums(D, first_row, w, order)
    f = objective(w, q, C)
    it = 0
    while True:
        g = w - 2.0 * C * r
        gmax = float(np.abs(g).max())
        H = np.eye(M + 1) + 2.0 * C * S
        if gmax <= tol or it >= max_iter:
            break
        p = np.linalg.solve(H, -g)
        gp = float(np.dot(g, p))
        t = 1.0
        while True:
            w2 = w + t * p
            S2, r2, q2, count2 = sums(D, first_row, w2, order)
            f2 = objective(w2, q2, C)
            if f2 <= f + C1 * t * gp + F_SLACK * abs(f) or t < MIN_STEP:
                break
            t *= 0.5
        if t < MIN_STEP:
            break
        w, S, r, q, count, f = w2, S2, r2, q2, count2, f2
        it += 1
    return dict(w=w, iterations=it, grad=gmax, active=count, objective=f, converged=gmax <= tol, H=H)
