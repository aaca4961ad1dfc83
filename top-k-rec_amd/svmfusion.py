"""SVM fusion (K23): the last of the reference's fusions, old/methods/sfusion.py there -- one weight per model from a linear SVM on the
score differences of sampled triplets.

    models = fusion.load_models('data', ['embed/bpr', 'embed/vbpr_cnn', 'embed/vbpr_mfcc'])
    w = learn_svm(models, csr, n_items)                            # sfusion: LinearSVC(C=0.01) on 1,000,000 sampled triplets
    U, V = fusion.fuse(models, w)                                  # served like every other fusion (fusion.py)

sfusion.py:28-63 samples a triplet per row as bfusion does (user uniform over the users with likes, positive uniform in the row, negative
uniform outside it), enters row t as +d_t with label +1 (t even) or -d_t with label -1 (t odd), d_t = s(u, i) - s(u, j) per model, fits
scikit-learn's LinearSVC(C=0.01) and returns coef_[0].  That estimator minimises, with y_t = +1 for even t and -1 for odd t,

    f(w, b) = (|w|^2 + b^2) / 2 + C sum_t max(0, 1 - (w . d_t + y_t b))^2

(squared hinge, L2 penalty; liblinear regularises the intercept as one more feature of value 1).  f is strictly convex and piecewise
quadratic, so no library is needed: Newton's method with Armijo backtracking reaches the one minimiser in a handful of passes.  The
rows are K16's features on K1's stream (tkr_hip.fusion_features, from triplet 0); every pass is one reduction over all rows, the sums
of csrc/fusion_svm.hip (tkr_hip.fusion_svm_sums), and the (M + 1) x (M + 1) Newton step runs on the host in fp64.  The intercept is
learned and dropped, as the reference drops it.

What differs from the reference, on purpose: the negatives are drawn over the whole ``vid``, as K16's learn_pairwise draws them; the
reference draws over f?tr.idl.
"""
from __future__ import annotations

import warnings

import numpy as np
import torch

import fusion
import tkr_hip

METHODS = ('s',)
ARMIJO_C1 = 1e-4              # f(w + t p) <= f(w) + c1 t g.p, t halved until it holds
F_SLACK = 2.0 ** -40          # ... up to the rounding of f itself: a relative 2^-40
MIN_STEP = 2.0 ** -30         # a step below this means f cannot be decreased any further in fp64


def newton(sums, M, N, C, max_iter):
    """minimise f from zeros.  ``sums(w~)`` -> (S, r, q, count) over the active rows under w~ = (w, b) fp64 [M + 1]
    (tkr_hip.fusion_svm_unpack); g = w~ - 2 C r, H = I + 2 C S, H p = -g; the trial point's sums are the next pass's.
    -> dict(w, iterations, grad = the final max|g|, active, objective, converged)"""
    tol = 1e-12 * max(1.0, C * N)
    w = np.zeros(M + 1)
    S, r, q, count = sums(w)
    f = 0.5 * float(np.dot(w, w)) + C * q
    it = 0
    while True:
        g = w - 2.0 * C * r
        gmax = float(np.abs(g).max())
        if gmax <= tol or it >= max_iter:
            break
        p = np.linalg.solve(np.eye(M + 1) + 2.0 * C * S, -g)
        gp = float(np.dot(g, p))
        t = 1.0
        while True:
            w2 = w + t * p
            S2, r2, q2, count2 = sums(w2)
            f2 = 0.5 * float(np.dot(w2, w2)) + C * q2
            if f2 <= f + ARMIJO_C1 * t * gp + F_SLACK * abs(f) or t < MIN_STEP:
                break
            t *= 0.5
        if t < MIN_STEP:
            break
        w, S, r, q, count, f = w2, S2, r2, q2, count2, f2
        it += 1
    return dict(w=w, iterations=it, grad=gmax, active=count, objective=f, converged=gmax <= tol)


def learn_svm(models, csr, n_items, *, n_samples=1_000_000, C=0.01, seed=0, max_iter=50, want_info=False, chunk_bytes=None):
    """sfusion.py:28-63 -> W float32 [M] (with want_info: (W, dict(weights fp64 [M], intercept, iterations, grad, active, objective,
    converged))).  ``csr`` is the TrainingCSR of the training likes (BPR.load_training_data + BPR._make_csr); row t is triplet t of K1's
    stream under ``seed``.  The features stay on the device when they fit ``chunk_bytes`` (default fusion.CHUNK_BYTES); otherwise every
    pass regenerates them chunk by chunk, in chunks of whole slabs, and the slabs' partial sums are reduced together: the result does
    not depend on the chunking.  Only the sums and the status word come down per pass."""
    device = csr.tr_users.device
    models = fusion._on_device(models, device)
    M, N, C = len(models), int(n_samples), float(C)
    if N < 1:
        raise tkr_hip.TkrError('learn_svm: n_samples >= 1 required, got %d' % N)
    if not (C > 0.0 and np.isfinite(C)):
        raise tkr_hip.TkrError('learn_svm: C must be positive and finite, got %r' % (C,))
    if not 1 <= M <= tkr_hip.FUSION_MAX_MODELS:
        raise tkr_hip.TkrError('learn_svm: 1 .. %d models required, got %d' % (tkr_hip.FUSION_MAX_MODELS, M))
    limit = fusion.CHUNK_BYTES if chunk_bytes is None else int(chunk_bytes)
    slab = tkr_hip.FUSION_SVM_SLAB
    words = tkr_hip.fusion_svm_words(M)
    kept = tkr_hip.fusion_features(models, csr, n_items, seed, 0, N) if 4 * M * N <= limit else None
    per_chunk = max(1, limit // (4 * M * slab)) * slab
    partial = torch.empty(tkr_hip.fusion_svm_partial_bytes(N, M) // 8, dtype=torch.float64, device=device)
    down = torch.empty(words + 1, dtype=torch.float64, device=device)          # what a pass brings down: the sums, then the status word
    out, status = down[:words], down[words:].view(torch.int64)
    Wd = torch.zeros(M + 1, dtype=torch.float64, device=device)

    def sums(w):
        Wd.copy_(torch.from_numpy(w))
        if kept is not None:
            tkr_hip.fusion_svm_sums(kept, Wd, 0, partial=partial, out=out, status=status, check=False)
        else:
            for c0 in range(0, N, per_chunk):
                n = min(per_chunk, N - c0)
                D = tkr_hip.fusion_features(models, csr, n_items, seed, c0, n)
                tkr_hip.fusion_svm_sums(D, Wd, c0, partial=partial, slab_offset=c0 // slab, reduce=c0 + n >= N, out=out, status=status,
                                        check=False)
                del D
        host = down.cpu().numpy()
        tkr_hip.fusion_svm_check(int(host[words:].view(np.int64)[0]))
        return tkr_hip.fusion_svm_unpack(host[:words], M)

    res = newton(sums, M, N, C, int(max_iter))
    if not res['converged']:
        warnings.warn('learn_svm: stopped after %d Newton steps at max|g| = %.3g (the bound is %.3g)'
                      % (res['iterations'], res['grad'], 1e-12 * max(1.0, C * N)), RuntimeWarning)
    W = res['w'][:M].astype(np.float32)
    if want_info:
        return W, dict(weights=res['w'][:M].copy(), intercept=float(res['w'][M]), iterations=res['iterations'], grad=res['grad'],
                       active=res['active'], objective=res['objective'], converged=res['converged'])
    return W
