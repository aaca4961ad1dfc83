"""NumPy oracle of K9 (tkr_bpr_foldin, csrc/foldin.hip): the draw restated on oracle/plan_np.py's Philox, and the step as
``oracle.ref_np.bpr_step`` on P copies of the user with the item state put back afterwards.  Not a test module.

    draw(ptr, cols, n_items, seed, steps, P, first_row)   -> trip int32 [m, steps, P, 2]  (-1 in rows without a triplet)
    fold_in(V, b, ptr, cols, trip, lu, lr, mode, U0)       -> U fp32 [m, k], loss fp32 [m]: bpr_step, literally
    fold_in_direct(..., dtype)                             -> the same formulas written out, in fp32 or fp64 (the measured
                                                              tolerance of the default depth needs an fp64 run of the same triplets)
"""
import numpy as np

from oracle import plan_np as P_
from oracle import ref_np as R

U64 = np.uint64
_MASK = U64(0xFFFFFFFF)
STREAM = 1            # fourth Philox counter word: K1 draws with 0


def live_rows(ptr, n_items):
    """rows that have a triplet at all: at least one positive, at least one column left for the negative"""
    deg = np.diff(np.asarray(ptr, dtype=np.int64))
    return (deg > 0) & (deg < n_items)


def draw(ptr, cols, n_items, seed, steps, P, first_row=0):
    """trip[x, t, p] = (i, j) of counter g = ((first_row + x) * steps + t) * P + p (mod 2^64): positive = the row's column number
    mulhi64(w2 | w3 << 32, deg) of round 0, negative = the first of the two candidates of rounds 1 .. MAX_ROUNDS that is not in
    the row, then the cyclic scan -- oracle/plan_np.py sample_triplets with the user fixed and the stream word set."""
    ptr = np.asarray(ptr, dtype=np.int64)
    cols = np.asarray(cols, dtype=np.int32)
    m = len(ptr) - 1
    trip = np.full((m, steps, P, 2), -1, dtype=np.int32)
    rows = np.flatnonzero(live_rows(ptr, n_items))
    if len(rows) == 0:
        return trip
    k0, k1 = seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF
    with np.errstate(over='ignore'):
        x = (np.asarray(rows, dtype=U64) + U64(first_row & 0xFFFFFFFFFFFFFFFF))[:, None, None]
        g = ((x * U64(steps) + np.arange(steps, dtype=U64)[None, :, None]) * U64(P) + np.arange(P, dtype=U64)[None, None, :]).reshape(-1)
    u = np.repeat(rows, steps * P)
    c0, c1 = (g & _MASK).astype(np.uint32), (g >> U64(32)).astype(np.uint32)
    n = len(g)
    stream = np.full(n, STREAM, dtype=np.uint32)
    _, _, w2, w3 = P_.philox4x32_10(c0, c1, np.zeros(n, np.uint32), stream, k0, k1)
    deg = ptr[u + 1] - ptr[u]
    i = cols[ptr[u] + P_.mulhi64(w2, w3, deg)]
    j = np.zeros(n, dtype=np.int32)
    pending = np.arange(n)
    for rnd in range(1, P_.MAX_ROUNDS + 1):
        if len(pending) == 0:
            break
        w0, w1, w2, w3 = P_.philox4x32_10(c0[pending], c1[pending], np.full(len(pending), rnd, np.uint32), stream[pending], k0, k1)
        ca = P_.mulhi64(w0, w1, n_items).astype(np.int32)
        cb = P_.mulhi64(w2, w3, n_items).astype(np.int32)
        ra = P_._member(u[pending], ca, ptr, cols, n_items)
        rb = P_._member(u[pending], cb, ptr, cols, n_items)
        j[pending] = np.where(~ra, ca, cb)
        pending = pending[ra & rb]
    for q in pending:                                   # cyclic scan (a row that holds almost every column)
        rated = set(cols[ptr[u[q]]:ptr[u[q] + 1]].tolist())
        cand = int(j[q])
        for _ in range(int(n_items)):
            if cand not in rated:
                break
            cand = (cand + 1) % int(n_items)
        j[q] = cand
    trip[rows] = np.stack([i, j], axis=1).reshape(len(rows), steps, P, 2)
    return trip


def _hp(lu, lr, mode):
    """the fold-in objective has no item terms: they are constants of u"""
    return dict(lu=lu, li=0.0, lj=0.0, lb=0.0, lr=lr, mode=mode)


def step_ref(state, rows, ij, hp):
    """ONE fold-in step of the listed user rows of state['U'] (ij [len(rows), P, 2]): ref_np.bpr_step on P copies of every user,
    then V, b, msV, msb restored.  Users do not meet: a step of several users is the step of each (the gradient of a row sums its
    own slices in order p).  -> what bpr_step returns (the objective summed over the rows)"""
    ib, jb = ij[:, :, 0].reshape(-1), ij[:, :, 1].reshape(-1)
    ub = np.repeat(np.asarray(rows), ij.shape[1])
    touched = np.unique(np.concatenate([ib, jb]))
    keep = {n: state[n][touched].copy() for n in ('V', 'b', 'msV', 'msb')}
    loss = R.bpr_step(state, ub, ib, jb, hp)
    for n, v in keep.items():
        state[n][touched] = v
    return loss


def fold_in(V, b, ptr, cols, trip, lu, lr, mode='l2', U0=None):
    """-> (U [m, k], loss [m]): steps 0 .. T-2 for all users in one bpr_step each, the last step user by user (bpr_step returns
    one number per call: the objective of that user's last step at its pre-step vector)"""
    m, T = trip.shape[0], trip.shape[1]
    n_items, k = V.shape
    state = dict(U=np.zeros((m, k), np.float32) if U0 is None else np.array(U0, dtype=np.float32),
                 V=np.array(V, dtype=np.float32), b=np.zeros(n_items, np.float32) if b is None else np.array(b, dtype=np.float32).reshape(-1),
                 msU=np.ones((m, k), np.float32), msV=np.ones((n_items, k), np.float32), msb=np.ones(n_items, np.float32))
    hp = _hp(lu, lr, mode)
    rows = np.flatnonzero(live_rows(ptr, n_items))
    loss = np.zeros(m, np.float32)
    if len(rows):
        for t in range(T - 1):
            step_ref(state, rows, trip[rows, t], hp)
        for x in rows:
            loss[x] = step_ref(state, [x], trip[[x], T - 1], hp)
    return state['U'], loss


def fold_in_direct(V, b, ptr, cols, trip, lu, lr, mode='l2', U0=None, dtype=np.float32):
    """the same steps with the formulas of ref_np.bpr_step written out for the user row alone, every operand and result in `dtype`"""
    F = dtype
    m, T, P = trip.shape[:3]
    n_items, k = V.shape
    V = np.asarray(V).astype(F)
    b = np.zeros(n_items, F) if b is None else np.asarray(b).reshape(-1).astype(F)
    U = np.zeros((m, k), F) if U0 is None else np.asarray(U0).astype(F)
    ms = np.ones((m, k), F)
    lu_, lr_, rho, eps = F(lu), F(lr), F(R.RHO), F(R.EPS)
    rows = np.flatnonzero(live_rows(ptr, n_items))
    loss = np.zeros(m, F)
    for t in range(T):
        ue = U[rows][:, None, :]                                     # [r, 1, k]
        ie, je = V[trip[rows, t, :, 0]], V[trip[rows, t, :, 1]]      # [r, P, k]
        x = (b[trip[rows, t, :, 0]] - b[trip[rows, t, :, 1]] + np.sum(ue * ie, axis=2, dtype=F) - np.sum(ue * je, axis=2, dtype=F)).astype(F)
        e = np.exp(-np.abs(x)).astype(F)
        s = np.where(x >= 0, e / (F(1) + e), F(1) / (F(1) + e)).astype(F)[:, :, None]
        reg = lu_ * ue if mode == 'l2' else lu_ * np.sign(ue)
        gp = (-s * (ie - je) + reg).astype(F)
        g = np.zeros((len(rows), k), F)
        for p in range(P):                                           # sequential, in order p
            g = (g + gp[:, p]).astype(F)
        if t == T - 1:
            soft = (np.maximum(-x, F(0)) + np.log1p(np.exp(-np.abs(x)))).astype(F)
            uu = np.broadcast_to(ue, ie.shape)
            pen = F(0.5) * np.sum(uu * uu * lu_, axis=(1, 2), dtype=F) if mode == 'l2' else np.sum(np.abs(uu) * lu_, axis=(1, 2), dtype=F)
            loss[rows] = np.sum(soft, axis=1, dtype=F) + pen
        new_ms = (rho * ms[rows] + (F(1) - rho) * g * g).astype(F)
        ms[rows] = new_ms
        U[rows] = (U[rows] - lr_ * g / np.sqrt(new_ms + eps)).astype(F)
    return U, loss


def csr(rows):
    """list of ascending unique column lists -> (ptr int64, cols int32)"""
    ptr = np.zeros(len(rows) + 1, np.int64)
    np.cumsum([len(x) for x in rows], out=ptr[1:])
    cols = np.concatenate([np.asarray(x, np.int32) for x in rows] + [np.zeros(0, np.int32)]).astype(np.int32)
    return ptr, cols


def auc_of(U, V, b, train, held):
    """mean over users of the share of (held-out like, unseen item) pairs ranked the right way; train / held: column lists"""
    s = U.astype(np.float64) @ V.astype(np.float64).T + (0.0 if b is None else np.asarray(b, np.float64).reshape(1, -1))
    out = []
    for x in range(len(U)):
        pos = np.asarray(held[x], dtype=np.int64)
        neg = np.setdiff1d(np.arange(V.shape[0]), np.concatenate([pos, np.asarray(train[x], dtype=np.int64)]))
        if len(pos) and len(neg):
            out.append(np.mean(s[x, pos][:, None] > s[x, neg][None, :]))
    return float(np.mean(out))
