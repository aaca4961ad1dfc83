"""NumPy oracle of K10 (tkr_bpr_foldin_items, csrc/foldin_items.hip): the draw restated on oracle/plan_np.py's Philox, and the step
as ``oracle.ref_np.bpr_step`` with the new item appended as row n_items of a copy of V / b and every other row and slot put back
afterwards.  Not a test module.

    draw(uptr, ucols, lptr, lrows, thresh, n_items, seed, steps, P, first_row) -> trip int32 [m, steps, P, 3] = (role, u, other item),
                                                                  (-1, -1, -1) where no legal draw exists; word uint32 [m, steps, P]
    fold_in_items(U, V, b, trip, li, lj, lb, lr, mode, V0, b0)   -> Vn fp32 [m, k], bn fp32 [m], loss fp32 [m]: bpr_step, literally
    fold_in_items_direct(..., dtype)                              -> the same formulas written out, sums in the order p, fp32 or fp64
    role_thresh(uptr, lptr, lrows, n_items)                       -> the thresholds, by a direct loop in exact rational arithmetic
"""
from fractions import Fraction

import numpy as np

from oracle import plan_np as P_
from oracle import ref_np as R

U64 = np.uint64
_MASK = U64(0xFFFFFFFF)
STREAM = 2            # fourth Philox counter word: K1 draws with 0, K9 with 1
ALWAYS = 0xFFFFFFFF


def _philox(c0, c1, rnd, k0, k1):
    n = len(c0)
    return P_.philox4x32_10(c0, c1, np.full(n, rnd, np.uint32), np.full(n, STREAM, np.uint32), k0, k1)


def draw(uptr, ucols, lptr, lrows, thresh, n_items, seed, steps, P, first_row=0):
    """Counter g = ((first_row + x) * steps + t) * P + p (mod 2^64), stream word 2.  Round 0: word 0 < thresh[x] (or thresh =
    0xffffffff) = role 1, words 2, 3 = the pick from a list.  Role 1: u = liker number mulhi64(w2 | w3 << 32, likers) of x, j = the
    first of the two candidates of rounds 1 .. MAX_ROUNDS that is not in u's row, then the cyclic scan (oracle/plan_np.py
    sample_triplets); no liker, or a row that is the whole catalogue: no triplet.  Role 0: u = the first of the two candidates of
    rounds 1 .. MAX_ROUNDS over [0, n_users) that has a row and is no liker of x, then a cyclic scan of at most n_users; i = column
    number mulhi64(w2 | w3 << 32, deg u) of u's row; no such user: no triplet."""
    uptr, lptr = np.asarray(uptr, dtype=np.int64), np.asarray(lptr, dtype=np.int64)
    ucols, lrows = np.asarray(ucols, dtype=np.int32), np.asarray(lrows, dtype=np.int32)
    thresh = np.asarray(thresh, dtype=np.int64)
    n_users, m = len(uptr) - 1, len(lptr) - 1
    udeg, nl_of = np.diff(uptr), np.diff(lptr)
    k0, k1 = seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF
    with np.errstate(over='ignore'):
        x3 = (np.arange(m, dtype=U64) + U64(first_row & 0xFFFFFFFFFFFFFFFF))[:, None, None]
        g = ((x3 * U64(steps) + np.arange(steps, dtype=U64)[None, :, None]) * U64(P) + np.arange(P, dtype=U64)[None, None, :]).reshape(-1)
    xs = np.repeat(np.arange(m), steps * P)
    c0, c1 = (g & _MASK).astype(np.uint32), (g >> U64(32)).astype(np.uint32)
    n = len(g)
    w0, _, w2, w3 = _philox(c0, c1, 0, k0, k1)
    positive = (thresh[xs] == ALWAYS) | (w0.astype(np.int64) < thresh[xs])
    role, uu, other = (np.full(n, -1, dtype=np.int32) for _ in range(3))

    # ---- role 1
    idx = np.flatnonzero(positive & (nl_of[xs] > 0))
    if len(idx):
        u = lrows[lptr[xs[idx]] + P_.mulhi64(w2[idx], w3[idx], nl_of[xs[idx]])].astype(np.int64)
        keep = udeg[u] < n_items
        idx, u = idx[keep], u[keep]
        j = np.zeros(len(idx), dtype=np.int32)
        found = np.zeros(len(idx), dtype=bool)
        pending = np.arange(len(idx))
        for rnd in range(1, P_.MAX_ROUNDS + 1):
            if len(pending) == 0:
                break
            a0, a1, a2, a3 = _philox(c0[idx[pending]], c1[idx[pending]], rnd, k0, k1)
            ca, cb = P_.mulhi64(a0, a1, n_items).astype(np.int32), P_.mulhi64(a2, a3, n_items).astype(np.int32)
            ra, rb = P_._member(u[pending], ca, uptr, ucols, n_items), P_._member(u[pending], cb, uptr, ucols, n_items)
            j[pending] = np.where(~ra, ca, cb)
            found[pending] = ~(ra & rb)
            pending = pending[ra & rb]
        for q in pending:                                   # cyclic scan (a row that holds almost every column)
            rated = set(ucols[uptr[u[q]]:uptr[u[q] + 1]].tolist())
            cand = int(j[q])
            for _ in range(int(n_items)):
                if cand not in rated:
                    found[q] = True
                    break
                cand = (cand + 1) % int(n_items)
            j[q] = cand
        assert found.all()                                  # (deg < n_items: the scan finds the column)
        role[idx], uu[idx], other[idx] = 1, u, j

    # ---- role 0
    idx = np.flatnonzero(~positive)
    if len(idx):
        def legal(xq, c):
            return (udeg[c] > 0) & ~P_._member(xq, c, lptr, lrows, n_users)
        u = np.zeros(len(idx), dtype=np.int64)
        found = np.zeros(len(idx), dtype=bool)
        pending = np.arange(len(idx))
        for rnd in range(1, P_.MAX_ROUNDS + 1):
            if len(pending) == 0:
                break
            a0, a1, a2, a3 = _philox(c0[idx[pending]], c1[idx[pending]], rnd, k0, k1)
            ca, cb = P_.mulhi64(a0, a1, n_users), P_.mulhi64(a2, a3, n_users)
            la, lb = legal(xs[idx[pending]], ca), legal(xs[idx[pending]], cb)
            u[pending] = np.where(la, ca, cb)
            found[pending] = la | lb
            pending = pending[~(la | lb)]
        for q in pending:                                   # cyclic scan (nearly every user with a row is a liker)
            likers = set(lrows[lptr[xs[idx[q]]]:lptr[xs[idx[q]] + 1]].tolist())
            cand = int(u[q])
            for _ in range(int(n_users)):
                if udeg[cand] > 0 and cand not in likers:
                    found[q] = True
                    break
                cand = (cand + 1) % int(n_users)
            u[q] = cand
        idx, u = idx[found], u[found]
        i = ucols[uptr[u] + P_.mulhi64(w2[idx], w3[idx], udeg[u])]
        role[idx], uu[idx], other[idx] = 0, u, i
    trip = np.stack([role, uu, other], axis=1).reshape(m, steps, P, 3)
    return trip, w0.reshape(m, steps, P)


def role_thresh(uptr, lptr, lrows, n_items):
    """floor(2^32 w+ / (w+ + w-)),  w+ = sum over likers of 1 / (deg_u + 1),  w- = sum over non-likers with a row of
    1 / (n_items + 1 - deg_u): the rates at which the model's own sampler (u uniform over the users with a row, i uniform over the
    row, j uniform over the rest of the catalogue) would draw x as positive and as negative from the training set grown by x, up to
    the common factor 1 / n_tr.  0xffffffff when no non-liker has a row.  A direct loop, in exact arithmetic."""
    udeg = np.diff(np.asarray(uptr, dtype=np.int64))
    out = []
    for x in range(len(lptr) - 1):
        likers = set(int(u) for u in lrows[lptr[x]:lptr[x + 1]])
        wp, wm, rows = Fraction(0), Fraction(0), 0
        for u in range(len(udeg)):
            d = int(udeg[u])
            if u in likers:
                wp += Fraction(1, d + 1)
            elif d > 0:
                wm += Fraction(1, int(n_items) + 1 - d)
                rows += 1
        out.append(ALWAYS if rows == 0 else min((wp * 2 ** 32 / (wp + wm)).__floor__(), ALWAYS))
    return np.asarray(out, dtype=np.int64)


def _hp(li, lj, lb, lr, mode):
    """the user side is frozen and restored: its regulariser is a constant of (v_x, b_x)"""
    return dict(lu=0.0, li=li, lj=lj, lb=lb, lr=lr, mode=mode)


def step_ref(state, tr, hp):
    """ONE fold-in step of the item in the LAST row of state['V'] / state['b'] on its triplets tr [P, 3] (those with role >= 0):
    ref_np.bpr_step with that row as i (role 1) or as j (role 0), then every other row and slot restored.  -> the objective bpr_step
    returns minus its terms that do not depend on the last row (the regularisers of the other item of every triplet), or None when
    the step has no triplet (nothing changes then)."""
    x = state['V'].shape[0] - 1
    tr = tr[tr[:, 0] >= 0]
    if len(tr) == 0:
        return None
    pos = tr[:, 0] == 1
    ub, ob = tr[:, 1].astype(np.int64), tr[:, 2].astype(np.int64)
    ib, jb = np.where(pos, x, ob), np.where(pos, ob, x)
    items, users = np.unique(ob), np.unique(ub)
    keep = {n: state[n][items].copy() for n in ('V', 'b', 'msV', 'msb')}
    keep_u = {n: state[n][users].copy() for n in ('U', 'msU')}
    V, b = state['V'].astype(np.float64), state['b'].astype(np.float64)
    lam = np.where(pos, hp['lj'], hp['li'])                    # the other item is the negative of a role-1 triplet
    if hp['mode'] == 'l2':
        const = 0.5 * np.sum(lam * np.sum(V[ob] ** 2, axis=1)) + 0.5 * hp['lb'] * np.sum(b[ob] ** 2)
    else:
        const = np.sum(lam * np.sum(np.abs(V[ob]), axis=1)) + hp['lb'] * np.sum(np.abs(b[ob]))
    loss = R.bpr_step(state, ub, ib, jb, hp)
    for n, v in keep.items():
        state[n][items] = v
    for n, v in keep_u.items():
        state[n][users] = v
    return np.float32(np.float64(loss) - const)


def fold_in_items(U, V, b, trip, li, lj, lb, lr, mode='l2', V0=None, b0=None):
    """-> (Vn [m, k], bn [m], loss [m]).  b None: no bias enters the score and none is learnt (bn = b0)."""
    m, T = trip.shape[0], trip.shape[1]
    n_items, k = V.shape
    n_users = U.shape[0]
    has_b = b is not None
    Vn = np.zeros((m, k), np.float32) if V0 is None else np.array(V0, dtype=np.float32)
    bn = np.zeros(m, np.float32) if b0 is None else np.array(b0, dtype=np.float32).reshape(-1)
    loss = np.zeros(m, np.float32)
    state = dict(U=np.array(U, dtype=np.float32), msU=np.ones((n_users, k), np.float32),
                 V=np.concatenate([np.asarray(V, np.float32), np.zeros((1, k), np.float32)]), msV=np.ones((n_items + 1, k), np.float32),
                 b=np.concatenate([np.asarray(b, np.float32).reshape(-1) if has_b else np.zeros(n_items, np.float32), np.zeros(1, np.float32)]),
                 msb=np.ones(n_items + 1, np.float32))
    hp = _hp(li, lj, lb if has_b else 0.0, lr, mode)
    for x in range(m):
        state['V'][n_items], state['msV'][n_items] = Vn[x], 1.0
        state['b'][n_items], state['msb'][n_items] = (bn[x] if has_b else 0.0), 1.0
        for t in range(T):
            out = step_ref(state, trip[x, t], hp)
            if not has_b:
                state['b'][n_items] = 0.0
            if t == T - 1 and out is not None:
                loss[x] = out
        Vn[x] = state['V'][n_items]
        if has_b:
            bn[x] = state['b'][n_items]
    return Vn, bn, loss


def fold_in_items_direct(U, V, b, trip, li, lj, lb, lr, mode='l2', V0=None, b0=None, dtype=np.float32):
    """the same steps with the formulas of ref_np.bpr_step written out for the new rows alone, all items at once, every operand and
    result in `dtype`, the sums over a step's triplets in the order p = 0 .. P-1 (as the kernel; bpr_step sums the role-1 slices
    before the role-0 slices, which differs by rounding only)"""
    F = dtype
    m, T, P = trip.shape[:3]
    n_items, k = V.shape
    has_b = b is not None
    U, V = np.asarray(U).astype(F), np.asarray(V).astype(F)
    bb = np.asarray(b).reshape(-1).astype(F) if has_b else np.zeros(n_items, F)
    Vn = np.zeros((m, k), F) if V0 is None else np.asarray(V0).astype(F)
    b_start = np.zeros(m, F) if b0 is None else np.asarray(b0).reshape(-1).astype(F)
    bn = b_start.copy() if has_b else np.zeros(m, F)
    ms, msb = np.ones((m, k), F), np.ones(m, F)
    li_, lj_, lb_, lr_, rho, eps = F(li), F(lj), F(lb), F(lr), F(R.RHO), F(R.EPS)
    l2 = mode == 'l2'
    loss = np.zeros(m, F)
    for t in range(T):
        role = trip[:, t, :, 0]
        valid, pos = role >= 0, role == 1
        live = valid.any(axis=1)
        ue, oe = U[np.maximum(trip[:, t, :, 1], 0)], V[np.maximum(trip[:, t, :, 2], 0)]         # [m, P, k]
        bo = bb[np.maximum(trip[:, t, :, 2], 0)]
        dx = np.sum(ue * Vn[:, None, :], axis=2, dtype=F)
        do = np.sum(ue * oe, axis=2, dtype=F)
        bx = bn[:, None]
        xs = np.where(pos, bx - bo + dx - do, bo - bx + do - dx).astype(F)
        e = np.exp(-np.abs(xs)).astype(F)
        s = np.where(xs >= 0, e / (F(1) + e), F(1) / (F(1) + e)).astype(F)
        c = np.where(pos, -s, s).astype(F)
        lam = np.where(pos, li_, lj_).astype(F)
        rv = Vn if l2 else np.sign(Vn)
        rb = bn if l2 else np.sign(bn)
        gp = np.where(valid[:, :, None], c[:, :, None] * ue + lam[:, :, None] * rv[:, None, :], F(0)).astype(F)
        gbp = np.where(valid, c + lb_ * rb[:, None], F(0)).astype(F)
        g, gb = np.zeros((m, k), F), np.zeros(m, F)
        for p in range(P):                                           # sequential, in order p
            g = (g + gp[:, p]).astype(F)
            gb = (gb + gbp[:, p]).astype(F)
        if t == T - 1:
            soft = np.where(valid, np.maximum(-xs, F(0)) + np.log1p(np.exp(-np.abs(xs))), F(0)).astype(F)
            n1, n0 = np.sum(pos, axis=1).astype(F), np.sum(valid & ~pos, axis=1).astype(F)
            pv = F(0.5) * np.sum(Vn * Vn, axis=1, dtype=F) if l2 else np.sum(np.abs(Vn), axis=1, dtype=F)
            pb = F(0.5) * bn * bn if l2 else np.abs(bn)
            loss = (np.sum(soft, axis=1, dtype=F) + (n1 * li_ + n0 * lj_) * pv + (n1 + n0) * lb_ * pb).astype(F)
        new_ms = (rho * ms + (F(1) - rho) * g * g).astype(F)
        new_v = (Vn - lr_ * g / np.sqrt(new_ms + eps)).astype(F)
        ms, Vn = np.where(live[:, None], new_ms, ms), np.where(live[:, None], new_v, Vn)
        if has_b:
            new_msb = (rho * msb + (F(1) - rho) * gb * gb).astype(F)
            new_b = (bn - lr_ * gb / np.sqrt(new_msb + eps)).astype(F)
            msb, bn = np.where(live, new_msb, msb), np.where(live, new_b, bn)
    return Vn, (bn if has_b else b_start), loss


def csr(rows):
    """list of ascending unique index lists -> (ptr int64, idx int32)"""
    ptr = np.zeros(len(rows) + 1, np.int64)
    np.cumsum([len(x) for x in rows], out=ptr[1:])
    idx = np.concatenate([np.asarray(x, np.int32) for x in rows] + [np.zeros(0, np.int32)]).astype(np.int32)
    return ptr, idx


def outrank_share(U, v_new, b_new, V, b, likers, rated):
    """mean over (new item x, liker u) of the share of the items u has not rated that x outranks for u (ties count as losses).
    likers[x]: user rows; rated[u]: the catalogue columns u has rated"""
    V64, U64_ = V.astype(np.float64), U.astype(np.float64)
    b64 = np.zeros(len(V)) if b is None else np.asarray(b, np.float64).reshape(-1)
    out = []
    for x, users in enumerate(likers):
        for u in users:
            s = V64 @ U64_[u] + b64
            sx = float(v_new[x].astype(np.float64) @ U64_[u] + (0.0 if b_new is None else float(np.asarray(b_new).reshape(-1)[x])))
            free = np.ones(len(V), dtype=bool)
            free[np.asarray(rated[u], dtype=np.int64)] = False
            if free.any():
                out.append(float(np.mean(sx > s[free])))
    return float(np.mean(out))


N_USERS, N_ITEMS = 300, 200
LIKER_COUNTS = [1, 2, 37, 150, 299, 0, 300, 12]


def shapes(seed=5):
    """the shapes of the draw tests, CPU and GPU: 300 users (ten without a row, one with the whole catalogue, one with all but one
    column), 200 items, eight new items with 1 .. 300 likers -> (uptr, ucols, user rows, lptr, lrows, liker lists)"""
    rng = np.random.Generator(np.random.PCG64(seed))
    deg = [int(d) for d in rng.integers(1, 40, N_USERS)]
    for u in range(10, 20):
        deg[u] = 0
    deg[3], deg[4] = N_ITEMS, N_ITEMS - 1
    rows = [np.sort(rng.choice(N_ITEMS, d, replace=False)).astype(np.int32) for d in deg]
    likers = [np.sort(rng.choice(N_USERS, c, replace=False)).astype(np.int32) for c in LIKER_COUNTS]
    likers[0] = np.array([3], np.int32)                               # a liker without a free column ...
    likers[1] = np.array([4, 12], np.int32)                           # ... one with a single free column and one without a row
    return csr(rows) + (rows,) + csr(likers) + (likers,)
