"""Float64 oracles WITH ERROR INTERVALS for the training-step kernels in the trained regime.  Not a test module.

The other step tests start from the initial state (factors ~ 1e-2, slots = 1) where x ~ 0, sigma ~ 0.5 and sqrt(ms + eps) ~ 1, and
compare through a fixed tolerance.  Here the state is the one a trained model is in -- |x| from 0 to > 100, RMSProp slots spread over
fourteen decades with exact zeros, exact +0.0 / -0.0 in the tables -- and a fixed tolerance is the wrong instrument: where sigma is
saturated the update is known to a relative 1e-7, where x is a cancelled sum of terms of 1e3 it is not known to 1e-3.  So every
function of this module returns, per element, the float64 value and an INTERVAL that any correct fp32 evaluation must lie in.

    trained_state / trained_vbpr_state      the state (the recipe below)
    bpr_step64                              K2 / K2f / K2o (RMSProp and SGD, l2 and l1); with ``unc`` also the later steps of a fold-in
    vbpr_step64                             K3
    fold_user64 / fold_item64               K9 / K10: T steps of one row each, on bpr_step64
    fusion_step64                           K16: one SGD batch on the weights
    share(box, got)                         the share of its interval an fp32 result uses, per element (<= 1: inside)

State recipe (trained_state): U, V ~ N(0, 0.5^2); a quarter of the user rows x 4 and a sixteenth x 16 (|x| from ~0 to > 100);
b ~ N(0, 1); 1/32 of the elements of U and V set to +0.0, 1/64 of U to -0.0, 1/16 of b to 0; every slot 10^uniform(-14, 0), 1/16 of
them exactly 0.  ``x16`` / ``x4`` are the shares of the scaled rows: the non-vacuity test (test_step_regimes_cpu.py) asks that 98 % of
the touched elements have an interval within 10 x the project's step tolerance, and shapes whose x is a sum of many large terms
(k = 600, the five-step fold-ins, the fusion batch) only meet that with smaller factors (``sd``; ``sb`` scales the biases) -- a
condition on the inputs, never on the check; state_kw, fold_kw and fusion_case say which and why.

The interval, with u = 2^-24 (the unit roundoff of fp32):

    dx_t      = c_x u (k + 4) sum|terms of x_t|                     (+ the uncertainty of the inputs, for the later fold-in steps)
    dsigma_t  = min(sigma_t, 1 - sigma_t) expm1(dx_t) + c_s u sigma_t  (|dsigma/dx| = sigma (1 - sigma), and both sigma and 1 - sigma change by
                                                                     at most a factor e^d over a distance d: tight where sigma is saturated)
    per gradient term +-sigma_t p:   d = |p| dsigma_t + u |term|    (|p| taken as |p_i| + |p_j| for the user's p = v_i - v_j)
    dg(e)     = sum_occ d + u (n_occ + 2) sum|terms of g(e)|        (the regulariser's terms included)

g -> lr g / sqrt(rho ms + (1 - rho) g^2 + eps) increases with g, so the bounds of the new P are that expression in float64 at
g - dg and g + dg, widened by c_r u (|P| + |update|) and by the smallest normal fp32 (elements with updates of 1e-58 exist; a result
below the normal range may also be flushed by a hardware rsq / rcp).  Slots: (1 - rho)(2 |g| dg + dg^2) + c_r u ms' (+ the same
floor).  Loss: sum_t (sigma_t expm1(dx_t) + c_l ulp32(max(|x_t|, 1))) + depth u sum|terms|, where depth bounds the number of additions
any term passes through (the kernels add a row's terms in a wave and the rows with one atomic each: <= 3 B + k / 64 + 8; K3 adds B^2
pair terms in blocks: B + 72).  K3's pair form log(1 + e^x) - x loses an ulp of |x| per pair by construction (csrc/tkr_common.h):
c_l covers it.

THE CONSTANTS are measured against the fp32 oracles (oracle/ref_np.bpr_step / vbpr_step, tests/_foldin_oracle.py,
_item_foldin_oracle.py, _fusion_oracle.py), never against a kernel: the smallest round values for which every fp32 oracle uses at
most HALF of every interval on every element of every shape of tests/test_gpu_step_regimes.py.  The other half is for a kernel that
sums in another order and uses hardware exp / rcp / rsq of 1 ulp.

    C = dict(x=1, s=8, r=8, l=2)

Measured: with (x, s, r) = (1, 8, 4) ref_np.bpr_step uses up to 0.77 of an interval and vbpr_step 0.80; doubling c_x or c_s changes no maximum
(they do not bind: the (k + 4) of dx is already a worst case, and sigma's own rounding is small beside it), doubling c_r halves it:
what binds is the last line, P - lr g / sqrt(ms' + eps) -- a square root, a division, a product and a difference, each rounded.
c_r = 6 gives 0.52 / 0.53, so 8 is the smallest round value.  c_l = 2: the stable softplus is good to an ulp of max(|x|, 1), the pair form
to two.  The largest shares with these constants, per table over all cases (K2 / K2f / K2o: U 0.383, V 0.387, b 0.267, slots
0.315; K3: cem 0.400, uce 0.389, ure 0.374, ire 0.326, irb 0.330, icb 0.309, slots 0.211; fold-in: U 0.115, new item rows 0.133,
their biases 0.043; fusion: W 0.005) are kept in MEASURED, and the test asserts them.
"""
import numpy as np

F32 = np.float32
U32 = 2.0 ** -24
TINY = float(np.finfo(np.float32).tiny)
RHO = float(F32(0.9))
EPS = float(F32(1e-10))
C = dict(x=1.0, s=8.0, r=8.0, l=2.0)

# largest share of an interval that the fp32 oracles use with C, per table, over all cases below (from a run of
# test_step_regimes_cpu.py, which asserts that none is exceeded and that all are <= 0.5)
MEASURED = {'bpr': {'U': 0.383, 'V': 0.387, 'b': 0.267, 'msU': 0.315, 'msV': 0.289, 'msb': 0.116},
            'vbpr': {'ure': 0.374, 'ms_ure': 0.206, 'uce': 0.389, 'ms_uce': 0.211, 'ire': 0.326, 'ms_ire': 0.2, 'irb': 0.33, 'ms_irb': 0.015,
                     'cem': 0.4, 'ms_cem': 0.035, 'icb': 0.309, 'ms_icb': 0.007},
            'fold': {'U': 0.115, 'Vn': 0.133, 'bn': 0.043}, 'fusion': {'W': 0.005}}


class Box:
    """float64 value, bounds and the mask of the elements the step touched"""

    def __init__(self, val, lo, hi, touched):
        self.val, self.lo, self.hi, self.touched = val, lo, hi, touched

    def half(self):
        return 0.5 * (self.hi - self.lo)


def share(box, got):
    """per element: the distance of ``got`` from the float64 value as a share of the interval's side it lies on (<= 1: inside;
    NaN / inf in ``got`` -> inf)"""
    got = np.asarray(got, dtype=np.float64)
    up, dn = box.hi - box.val, box.val - box.lo
    with np.errstate(invalid='ignore', divide='ignore'):
        r = np.where(got >= box.val, (got - box.val) / up, (box.val - got) / dn)
    r = np.where(got == box.val, 0.0, r)                  # (an untouched element has no interval: equal or outside)
    return np.where(np.isfinite(got) & ~np.isnan(r), r, np.inf)


# ---------------------------------------------------------------------------------------------------------------- state
def _zeros_and_slots(rng, shape):
    ms = (10.0 ** rng.uniform(-14, 0, shape)).astype(F32)
    ms[rng.random(shape) < 1 / 16] = 0.0
    return ms


def _factor(rng, n, k, neg_zero, sd=0.5):
    M = (rng.standard_normal((n, k)) * sd).astype(F32)
    M[rng.random((n, k)) < 1 / 32] = 0.0
    if neg_zero:
        M[rng.random((n, k)) < 1 / 64] = -0.0
    return M


def trained_state(n_users, n_items, k, rng, x16=1 / 16, x4=1 / 4, sd=0.5, sb=1.0):
    U = (rng.standard_normal((n_users, k)) * sd).astype(F32)
    r = rng.random(n_users)
    U[r < x4] *= F32(4)
    U[r >= 1 - x16] *= F32(16)
    U[rng.random((n_users, k)) < 1 / 32] = 0.0
    U[rng.random((n_users, k)) < 1 / 64] = -0.0
    V = _factor(rng, n_items, k, False, sd)
    b = (rng.standard_normal(n_items) * sb).astype(F32)
    b[rng.random(n_items) < 1 / 16] = 0.0
    return dict(U=U, V=V, b=b, msU=_zeros_and_slots(rng, (n_users, k)), msV=_zeros_and_slots(rng, (n_items, k)),
                msb=_zeros_and_slots(rng, n_items))


def plant_zero_gradient(state, u, i, j, col=0):
    """make element ``col`` of user row u an exact ms = 0, g = 0 case (u drawn once, with items i, j): U = +0, both item elements 0"""
    state['U'][u, col] = 0.0
    state['msU'][u, col] = 0.0
    state['V'][i, col] = 0.0
    state['V'][j, col] = 0.0


def trained_vbpr_state(n_users, n_items, k, d, feat, rng, x16=1 / 16, x4=1 / 4, span=40.0):
    """the VBPR twin: ure / uce / ire as U / V above at width k // 2, uce at a quarter of the scale; cem ~ N(0, 0.5^2), irb and icb
    of a few units; zeros in cem / icb, slots from the recipe for every table.  scale_vbpr_state then sets the reach of alpha and beta."""
    kh = k // 2
    base = trained_state(n_users, n_items, kh, rng, x16, x4)
    st = dict(ure=base['U'], ire=base['V'], ms_ure=base['msU'], ms_ire=base['msV'], ms_irb=base['msb'])
    uce = trained_state(n_users, 1, kh, rng, x16, x4)
    st['uce'], st['ms_uce'] = (uce['U'] * F32(0.25)).astype(F32), uce['msU']
    icb = rng.standard_normal(d)
    proj = feat.astype(np.float64) @ icb
    icb *= 0.25 * span / max(np.abs(proj[:, None] - proj[None, :]).max(), 1e-30)
    st['icb'] = icb.astype(F32)
    st['icb'][rng.random(d) < 1 / 16] = 0.0
    st['irb'] = (base['b'] * F32(0.12 * span)).astype(F32)
    cem = rng.standard_normal((d, kh)) * 0.5
    cem[rng.random((d, kh)) < 1 / 32] = 0.0
    st['cem'] = cem.astype(F32)
    st['ms_cem'], st['ms_icb'] = _zeros_and_slots(rng, (d, kh)), _zeros_and_slots(rng, d)
    return st


def scale_vbpr_state(st, feat, ub, ib, jb, reach=60.0):
    """scale irb / icb and ure / uce so that the batch's alpha and beta each reach ``reach`` in magnitude, and beta with both signs
    (the user with the second largest |beta| is scaled to -+0.9 reach): e^alpha e^beta overflows (alpha + beta > 88.7) and underflows
    (< -87.3) for some pairs, and both stay inside the documented +-80 (include/tkr.h tkr_vbpr_run)"""
    f = feat.astype(np.float64)
    alpha = st['irb'].astype(np.float64)[ib] - st['irb'][jb] + (f[ib] - f[jb]) @ st['icb'].astype(np.float64)
    fa = F32(reach / np.abs(alpha).max())
    st['irb'], st['icb'] = (st['irb'] * fa).astype(F32), (st['icb'] * fa).astype(F32)
    ie = np.concatenate([st['ire'].astype(np.float64), f @ st['cem'].astype(np.float64)], axis=1)

    def beta():
        ue = np.concatenate([st['ure'], st['uce']], axis=1).astype(np.float64)
        return np.sum(ue[ub] * (ie[ib] - ie[jb]), axis=1)
    fb = F32(reach / np.abs(beta()).max())
    st['ure'], st['uce'] = (st['ure'] * fb).astype(F32), (st['uce'] * fb).astype(F32)
    be = beta()
    t0 = int(np.argmax(np.abs(be)))
    t1 = int(np.argmax(np.abs(be) * (ub != ub[t0])))
    f1 = F32(-np.sign(be[t0]) * 0.9 * reach / be[t1])
    for n in ('ure', 'uce'):
        st[n][ub[t1]] = (st[n][ub[t1]] * f1).astype(F32)
    return st


# ---------------------------------------------------------------------------------------------------------------- helpers
def _sig(x):
    e = np.exp(-np.abs(x))
    return np.where(x >= 0, e / (1 + e), 1 / (1 + e))


def _soft(x):
    return np.maximum(-x, 0) + np.log1p(np.exp(-np.abs(x)))


def _ulp32(v):
    return np.spacing(np.maximum(np.abs(v), 1.0).astype(F32)).astype(np.float64)


def _hp64(hp, names):
    return [float(F32(hp[n])) for n in names]


def _reg(P, lam, mode, dP=None):
    """regulariser's gradient term, its magnitude and its error"""
    if mode == 'l2':
        r = lam * P
        return r, np.abs(r), U32 * np.abs(r) + (0 if dP is None else lam * dP)
    r = lam * np.sign(P)
    unsure = 0 if dP is None else np.where(np.abs(P) <= dP, 2 * lam, 0.0) * (dP > 0)
    return r, np.abs(r), unsure


def _seg(index, rows, *vals):
    """sums of the slices per unique row: rows = np.unique(index)"""
    inv = np.searchsorted(rows, index)
    out = []
    for v in vals:
        acc = np.zeros((len(rows),) + v.shape[1:])
        np.add.at(acc, inv, v)
        out.append(acc)
    cnt = np.zeros(len(rows))
    np.add.at(cnt, inv, 1.0)
    return out, cnt


def _rms(P, ms, g, dg, lr, opt, dP=0.0, dms=0.0):
    """-> (P', lo, hi), (ms', lo, hi) of the optimiser's update of elements P with gradient g +- dg"""
    if opt == 'sgd':
        val = P - lr * g
        w = C['r'] * U32 * (np.abs(P) + lr * (np.abs(g) + dg)) + TINY + dP
        return (val, P - lr * (g + dg) - w, P - lr * (g - dg) + w), (ms, ms, ms)

    def upd(gg, mm):
        return lr * gg / np.sqrt(RHO * mm + (1 - RHO) * gg * gg + EPS)
    m_lo, m_hi = np.maximum(ms - dms, 0.0), ms + dms
    cands = [upd(g + s * dg, m) for s in (-1, 1) for m in (m_lo, m_hi)]
    u_lo, u_hi = np.minimum.reduce(cands), np.maximum.reduce(cands)
    w = C['r'] * U32 * (np.abs(P) + np.maximum(np.abs(u_lo), np.abs(u_hi))) + TINY + dP
    new = RHO * ms + (1 - RHO) * g * g
    dnew = RHO * dms + (1 - RHO) * (2 * np.abs(g) * dg + dg * dg) + C['r'] * U32 * new + TINY
    return (P - upd(g, ms), P - u_hi - w, P - u_lo + w), (new, new - dnew, new + dnew)


def _apply(out, name, msname, P, ms, rows, g, dg, lr, opt, dP=None, dms=None):
    val, lo, hi = P.copy(), P.copy(), P.copy()
    mval, mlo, mhi = ms.copy(), ms.copy(), ms.copy()
    if dP is not None:
        lo, hi = lo - dP, hi + dP
        mlo, mhi = np.maximum(mlo - dms, 0), mhi + dms
    (v, l, h), (mv, ml, mh) = _rms(P[rows], ms[rows], g, dg, lr, opt, 0.0 if dP is None else dP[rows], 0.0 if dms is None else dms[rows])
    val[rows], lo[rows], hi[rows] = v, l, h
    mval[rows], mlo[rows], mhi[rows] = mv, ml, mh
    touched = np.zeros(P.shape, dtype=bool)
    touched[rows] = True
    out[name], out[msname] = Box(val, lo, hi, touched), Box(mval, mlo, mhi, touched)


# ---------------------------------------------------------------------------------------------------------------- BPR
def bpr_step64(state, ub, ib, jb, hp, unc=None, loss_depth=None):
    """one mini-batch of oracle/ref_np.bpr_step in float64 on the fp32 ``state`` (not changed) -> dict of Box for U, V, b, msU, msV,
    msb, and 'loss' -> (value, lo, hi).  ``unc``: dict of half-widths of U / msU (the earlier steps of a fold-in row) or of V / b /
    msV / msb; the tables not named are exact."""
    lu, li, lj, lb, lr = _hp64(hp, ('lu', 'li', 'lj', 'lb', 'lr'))
    mode, opt = hp.get('mode', 'l2'), hp.get('opt', 'rmsprop')
    T = {n: state[n].astype(np.float64) for n in ('U', 'V', 'b')}
    M = {n: (state[n].astype(np.float64) if state.get(n) is not None else np.zeros_like(T[n[2:]])) for n in ('msU', 'msV', 'msb')}
    unc = unc or {}
    ub, ib, jb = (np.asarray(a, dtype=np.int64) for a in (ub, ib, jb))
    B, k = len(ub), T['U'].shape[1]
    ue, ie, je, bi, bj = T['U'][ub], T['V'][ib], T['V'][jb], T['b'][ib], T['b'][jb]
    zU, zV, zb = (unc.get(n) for n in ('U', 'V', 'b'))
    dU = None if zU is None else zU[ub]
    dVi, dVj = (None, None) if zV is None else (zV[ib], zV[jb])
    dbi, dbj = (None, None) if zb is None else (zb[ib], zb[jb])
    x = bi - bj + np.sum(ue * ie, axis=1) - np.sum(ue * je, axis=1)
    ax = np.abs(bi) + np.abs(bj) + np.sum(np.abs(ue) * (np.abs(ie) + np.abs(je)), axis=1)
    dx = C['x'] * U32 * (k + 4) * ax
    if dU is not None:
        dx = dx + np.sum(dU * (np.abs(ie) + np.abs(je)), axis=1)
    if dVi is not None:
        dx = dx + np.sum((np.abs(ue) + (0 if dU is None else dU)) * (dVi + dVj), axis=1)
    if dbi is not None:
        dx = dx + dbi + dbj
    s = _sig(x)
    ds = np.minimum(s, 1 - s) * np.expm1(dx) + s * C['s'] * U32
    s_, ds_ = s[:, None], ds[:, None]

    def terms(coef_mag, coef_unc, P, lam, dP):
        """+-s * coef + reg(P): the regulariser's term, the magnitude of both terms, their error"""
        r, ar, er = _reg(P, lam, mode, dP)
        mag = s_ * coef_mag if coef_mag.ndim == 2 else s * coef_mag
        e = (coef_mag * (ds_ if coef_mag.ndim == 2 else ds)) + U32 * mag
        if coef_unc is not None:
            e = e + (s_ + ds_ if coef_mag.ndim == 2 else s + ds) * coef_unc
        return r, mag + ar, e + er

    out = {}
    rU, aU, eU = terms(np.abs(ie) + np.abs(je), None if dVi is None else dVi + dVj, ue, lu, dU)
    gU = -s_ * (ie - je) + rU
    rows_u = np.unique(ub)
    (G, A, D), n = _seg(ub, rows_u, gU, aU, eU)
    _apply(out, 'U', 'msU', T['U'], M['msU'], rows_u, G, D + U32 * (n[:, None] + 2) * A, lr, opt, zU, unc.get('msU'))
    items = np.concatenate([ib, jb])
    rows_v = np.unique(items)
    rI, aI, eI = terms(np.abs(ue), dU, ie, li, dVi)
    rJ, aJ, eJ = terms(np.abs(ue), dU, je, lj, dVj)
    (G, A, D), n = _seg(items, rows_v, np.concatenate([-s_ * ue + rI, s_ * ue + rJ]), np.concatenate([aI, aJ]), np.concatenate([eI, eJ]))
    _apply(out, 'V', 'msV', T['V'], M['msV'], rows_v, G, D + U32 * (n[:, None] + 2) * A, lr, opt, zV, unc.get('msV'))
    one = np.ones(B)
    rI, aI, eI = terms(one, None, bi, lb, dbi)
    rJ, aJ, eJ = terms(one, None, bj, lb, dbj)
    (G, A, D), n = _seg(items, rows_v, np.concatenate([-s + rI, s + rJ]), np.concatenate([aI, aJ]), np.concatenate([eI, eJ]))
    _apply(out, 'b', 'msb', T['b'], M['msb'], rows_v, G, D + U32 * (n + 2) * A, lr, opt, zb, unc.get('msb'))
    if mode == 'l2':
        pen = 0.5 * np.sum(ue * ue * lu + ie * ie * li + je * je * lj) + 0.5 * lb * np.sum(bi * bi + bj * bj)
        dpen = 0.0 if dU is None else np.sum(lu * np.abs(ue) * dU + 0.5 * lu * dU * dU) * 1.0
    else:
        pen = np.sum(np.abs(ue) * lu + np.abs(ie) * li + np.abs(je) * lj) + lb * np.sum(np.abs(bi) + np.abs(bj))
        dpen = 0.0 if dU is None else np.sum(lu * dU)
    if dVi is not None:
        dpen = dpen + np.sum(li * (np.abs(ie) + 1) * dVi + lj * (np.abs(je) + 1) * dVj) + lb * np.sum((np.abs(bi) + 1) * dbi + (np.abs(bj) + 1) * dbj)
    val = np.sum(_soft(x)) + pen
    depth = loss_depth if loss_depth is not None else 3 * B + (k + 63) // 64 + 8
    dl = np.sum(s * np.expm1(dx) + C['l'] * _ulp32(x)) + depth * U32 * val + dpen
    out['loss'] = (val, val - dl, val + dl)
    out['x'] = x
    return out


# ---------------------------------------------------------------------------------------------------------------- fold-in
def fold_user64(V, b, U0, trip, lu, lr, mode):
    """K9: T steps of every row of U0 [m, k] on its own triplets trip [m, T, P, 2]; the item side is exact, the row's own value and
    slot carry their interval from step to step.  The slot starts at 1 (where the kernel starts it).  -> Box of U after the T steps,
    (loss, lo, hi) [m] of the last step"""
    m, T_, P = trip.shape[:3]
    hp = dict(lu=lu, li=0.0, lj=0.0, lb=0.0, lr=lr, mode=mode)
    k = V.shape[1]
    st = dict(U=np.array(U0, dtype=np.float64), V=np.asarray(V, dtype=F32), b=(np.zeros(len(V), F32) if b is None else np.asarray(b, F32).reshape(-1)),
              msU=np.ones((m, k)), msV=None, msb=None)
    unc = dict(U=np.zeros((m, k)), msU=np.zeros((m, k)))
    lo, hi = st['U'].copy(), st['U'].copy()
    loss = np.zeros((3, m))
    for t in range(T_):
        ub = np.repeat(np.arange(m), P)
        if t < T_ - 1:
            out = bpr_step64(st, ub, trip[:, t, :, 0].reshape(-1), trip[:, t, :, 1].reshape(-1), hp, unc)
            boxes = [out]
        else:                                   # the last step row by row: one loss per row
            boxes = [bpr_step64(st, np.full(P, r), trip[r, t, :, 0], trip[r, t, :, 1], hp, unc, loss_depth=P + (k + 63) // 64 + 8) for r in range(m)]
            for r in range(m):
                loss[:, r] = boxes[r]['loss']
        newU, newms = st['U'].copy(), st['msU'].copy()
        for o in boxes:
            tch = o['U'].touched
            newU[tch], newms[tch] = o['U'].val[tch], o['msU'].val[tch]
            lo[tch], hi[tch] = o['U'].lo[tch], o['U'].hi[tch]
            unc['U'][tch] = np.maximum(o['U'].hi - o['U'].val, o['U'].val - o['U'].lo)[tch]
            unc['msU'][tch] = np.maximum(o['msU'].hi - o['msU'].val, o['msU'].val - o['msU'].lo)[tch]
        st['U'], st['msU'] = newU, newms
    return Box(st['U'], lo, hi, np.ones((m, k), dtype=bool)), tuple(loss)


def fold_item64(U, V, b, V0, b0, trip, li, lj, lb, lr, mode):
    """K10: T steps of every new item x (row V0[x], bias b0[x]) on trip [m, T, P, 3] = (role, u, other item), all roles >= 0; the
    new item is row n_items of a copy of V / b (tests/_item_foldin_oracle.py), everything else is exact and stays.  -> Box of the new
    rows, Box of the new biases, (loss, lo, hi) [m] of the last step without the terms that do not depend on the new row"""
    m, T_, P = trip.shape[:3]
    n_items, k = V.shape
    hp = dict(lu=0.0, li=li, lj=lj, lb=lb, lr=lr, mode=mode)
    V64, b64 = np.asarray(V, dtype=np.float64), np.asarray(b, dtype=np.float64).reshape(-1)
    res = [np.zeros((m, k)) for _ in range(3)] + [np.zeros(m) for _ in range(3)]
    loss = np.zeros((3, m))
    live = np.zeros(m, dtype=bool)
    for x in range(m):
        st = dict(U=np.asarray(U, F32), V=np.concatenate([V64, np.asarray(V0[x], np.float64)[None]]), b=np.concatenate([b64, [float(b0[x])]]),
                  msU=None, msV=np.ones((n_items + 1, k)), msb=np.ones(n_items + 1))
        unc = dict(V=np.zeros((n_items + 1, k)), b=np.zeros(n_items + 1), msV=np.zeros((n_items + 1, k)), msb=np.zeros(n_items + 1))
        for t in range(T_):
            tr = trip[x, t]
            tr = tr[tr[:, 0] >= 0]
            if len(tr) == 0:                    # no legal draw: the step changes nothing
                continue
            pos = tr[:, 0] == 1
            ob = tr[:, 2].astype(np.int64)
            ibb, jbb = np.where(pos, n_items, ob), np.where(pos, ob, n_items)
            o = bpr_step64(st, tr[:, 1], ibb, jbb, hp, unc, loss_depth=P + (k + 63) // 64 + 8)
            live[x] = True
            if t == T_ - 1:
                lam = np.where(pos, lj, li)
                if mode == 'l2':
                    const = 0.5 * np.sum(lam * np.sum(V64[ob] ** 2, axis=1)) + 0.5 * float(F32(lb)) * np.sum(b64[ob] ** 2)
                else:
                    const = np.sum(lam * np.sum(np.abs(V64[ob]), axis=1)) + float(F32(lb)) * np.sum(np.abs(b64[ob]))
                loss[:, x] = np.array(o['loss']) - const
            for name, ms in (('V', 'msV'), ('b', 'msb')):
                st[name][n_items], st[ms][n_items] = o[name].val[n_items], o[ms].val[n_items]
                unc[name][n_items] = np.maximum(o[name].hi - o[name].val, o[name].val - o[name].lo)[n_items]
                unc[ms][n_items] = np.maximum(o[ms].hi - o[ms].val, o[ms].val - o[ms].lo)[n_items]
        for q, name in ((0, 'V'), (3, 'b')):
            res[q][x] = st[name][n_items]
            res[q + 1][x], res[q + 2][x] = st[name][n_items] - unc[name][n_items], st[name][n_items] + unc[name][n_items]
    return (Box(res[0], res[1], res[2], np.repeat(live[:, None], k, axis=1)), Box(res[3], res[4], res[5], live.copy()), tuple(loss))


# ---------------------------------------------------------------------------------------------------------------- fusion
def fusion_step64(W, D, lr, lambda_w):
    """K16: one call of tests/_fusion_oracle.sgd_step on the batch's score differences D [B, M] (fp32) -> Box of W', (cost, lo, hi)"""
    W64, D64 = np.asarray(W, dtype=np.float64), np.asarray(D, dtype=np.float64)
    lr, lam = float(F32(lr)), float(F32(lambda_w))
    B, M = D64.shape
    x = D64 @ W64
    dx = C['x'] * U32 * (M + 4) * (np.abs(D64) @ np.abs(W64))
    s = _sig(x)
    ds = np.minimum(s, 1 - s) * np.expm1(dx) + s * C['s'] * U32
    g = -(s[:, None] * D64).sum(axis=0) + lam * W64
    mag = (s[:, None] * np.abs(D64)).sum(axis=0) + lam * np.abs(W64)
    dg = (ds[:, None] * np.abs(D64)).sum(axis=0) + U32 * mag + U32 * (B + 3) * mag
    (val, lo, hi), _ = _rms(W64, None, g, dg, lr, 'sgd')
    cost = np.sum(_soft(x)) + 0.5 * lam * np.sum(W64 * W64)
    dc = np.sum(s * np.expm1(dx) + C['l'] * _ulp32(x)) + (B + M + 8) * U32 * cost
    return Box(val, lo, hi, np.ones(M, dtype=bool)), (cost, cost - dc, cost + dc)


# ---------------------------------------------------------------------------------------------------------------- VBPR
def vbpr_step64(state, feat, ub, ib, jb, hp):
    """one mini-batch of oracle/ref_np.vbpr_step in float64 -> dict of Box for ure, uce, ire, irb, cem, icb and their ms_ twins,
    'loss' -> (value, lo, hi), 'alpha', 'beta'.  The same construction as bpr_step64 with S_a = sum_b sigma_ab and T_b = sum_a
    sigma_ab as coefficients (dS = sum dsigma_ab + u (B + 2) S); sum|feat . cem| enters dx."""
    lu, li, lj, lb, le, lr = _hp64(hp, ('lu', 'li', 'lj', 'lb', 'le', 'lr'))
    mode = hp.get('mode', 'l2')
    S = {n: state[n].astype(np.float64) for n in ('ure', 'uce', 'ire', 'irb', 'cem', 'icb')}
    Ms = {n: state['ms_' + n].astype(np.float64) for n in S}
    f = feat.astype(np.float64)
    ub, ib, jb = (np.asarray(a, dtype=np.int64) for a in (ub, ib, jb))
    B, kh, d = len(ub), S['ure'].shape[1], f.shape[1]
    ur, uc, ir, jr, bi, bj = S['ure'][ub], S['uce'][ub], S['ire'][ib], S['ire'][jb], S['irb'][ib], S['irb'][jb]
    ic, jc = f[ib], f[jb]
    nnz = max(int((feat != 0).sum(axis=1).max()), 1)
    ice, jce = ic @ S['cem'], jc @ S['cem']
    a_ice, a_jce = np.abs(ic) @ np.abs(S['cem']), np.abs(jc) @ np.abs(S['cem'])
    beta = np.sum(ur * ir + uc * ice, axis=1) - np.sum(ur * jr + uc * jce, axis=1)
    a_beta = np.sum(np.abs(ur) * (np.abs(ir) + np.abs(jr)) + np.abs(uc) * (a_ice + a_jce), axis=1)
    d_beta = C['x'] * U32 * (2 * kh + 2 * nnz + 4) * a_beta
    dfeat = ic - jc
    alpha = bi - bj + dfeat @ S['icb']
    a_alpha = np.abs(bi) + np.abs(bj) + (np.abs(ic) + np.abs(jc)) @ np.abs(S['icb'])
    d_alpha = C['x'] * U32 * (2 * nnz + 4) * a_alpha
    x = alpha[:, None] + beta[None, :]
    dx = d_alpha[:, None] + d_beta[None, :] + C['x'] * U32 * (np.abs(alpha)[:, None] + np.abs(beta)[None, :])
    sg = _sig(x)
    dsg = np.minimum(sg, 1 - sg) * np.expm1(dx) + sg * C['s'] * U32
    sa, dsa = sg.sum(axis=1), dsg.sum(axis=1)              # coefficient of alpha_a
    sb, dsb = sg.sum(axis=0), dsg.sum(axis=0)              # coefficient of beta_b
    dsa = dsa + U32 * (B + 2) * sa
    dsb = dsb + U32 * (B + 2) * sb
    s_, ds_ = sb[:, None], dsb[:, None]
    out = {}

    def terms(coef, coef_mag, coef_err, P, lam):
        r, ar, er = _reg(P, lam, mode)
        mag = s_ * coef_mag
        return r, mag + ar, coef_mag * ds_ + U32 * mag + (s_ + ds_) * coef_err + er

    e_ice = C['x'] * U32 * (nnz + 2) * (a_ice + a_jce)       # error of fl(ice - jce)
    rows_u = np.unique(ub)
    r, a, e = terms(ir - jr, np.abs(ir) + np.abs(jr), 0.0, ur, lu)
    (G, A, D), n = _seg(ub, rows_u, -s_ * (ir - jr) + r, a, e)
    _apply(out, 'ure', 'ms_ure', S['ure'], Ms['ure'], rows_u, G, D + U32 * (n[:, None] + 2) * A, lr, 'rmsprop')
    r, a, e = terms(ice - jce, a_ice + a_jce, e_ice, uc, lu)
    (G, A, D), n = _seg(ub, rows_u, -s_ * (ice - jce) + r, a, e)
    _apply(out, 'uce', 'ms_uce', S['uce'], Ms['uce'], rows_u, G, D + U32 * (n[:, None] + 2) * A, lr, 'rmsprop')
    items = np.concatenate([ib, jb])
    rows_i = np.unique(items)
    rI, aI, eI = terms(ur, np.abs(ur), 0.0, ir, li)
    rJ, aJ, eJ = terms(ur, np.abs(ur), 0.0, jr, lj)
    (G, A, D), n = _seg(items, rows_i, np.concatenate([-s_ * ur + rI, s_ * ur + rJ]), np.concatenate([aI, aJ]), np.concatenate([eI, eJ]))
    _apply(out, 'ire', 'ms_ire', S['ire'], Ms['ire'], rows_i, G, D + U32 * (n[:, None] + 2) * A, lr, 'rmsprop')
    rI, aI, _ = _reg(bi, lb, mode)
    rJ, aJ, _ = _reg(bj, lb, mode)
    (G, A, D), n = _seg(items, rows_i, np.concatenate([-sa + rI, sa + rJ]), np.concatenate([sa + aI, sa + aJ]),
                        np.concatenate([dsa + U32 * (sa + aI), dsa + U32 * (sa + aJ)]))
    _apply(out, 'irb', 'ms_irb', S['irb'], Ms['irb'], rows_i, G, D + U32 * (n + 2) * A, lr, 'rmsprop')
    # dense: cem [d, kh] = sum_t (f_i - f_j)[t, c] * (-T_t uc[t, :]) + le reg; icb [d] = sum_t (f_i - f_j)[t, c] * (-S_t) + lb reg
    r, ar, er = _reg(S['cem'], le, mode)
    af = np.abs(ic) + np.abs(jc)
    g = dfeat.T @ (-s_ * uc) + r
    mag = af.T @ (s_ * np.abs(uc)) + ar
    occ = (af != 0).sum(axis=0)[:, None]
    dg = af.T @ (ds_ * np.abs(uc)) + U32 * (2 * occ + 4) * mag + er
    all_cem = np.arange(d)
    _apply(out, 'cem', 'ms_cem', S['cem'], Ms['cem'], all_cem, g, dg, lr, 'rmsprop')
    r, ar, er = _reg(S['icb'], lb, mode)
    g = dfeat.T @ (-sa) + r
    mag = af.T @ sa + ar
    dg = af.T @ dsa + U32 * (2 * occ[:, 0] + 4) * mag + er
    _apply(out, 'icb', 'ms_icb', S['icb'], Ms['icb'], all_cem, g, dg, lr, 'rmsprop')
    if mode == 'l2':
        pen = (0.5 * le * np.sum(S['cem'] ** 2) + 0.5 * np.sum((ur * ur + uc * uc) * lu + ir * ir * li + jr * jr * lj)
               + 0.5 * lb * (np.sum(bi * bi + bj * bj) + np.sum(S['icb'] ** 2)))
    else:
        pen = (le * np.sum(np.abs(S['cem'])) + np.sum((np.abs(ur) + np.abs(uc)) * lu + np.abs(ir) * li + np.abs(jr) * lj)
               + lb * (np.sum(np.abs(bi) + np.abs(bj)) + np.sum(np.abs(S['icb']))))
    val = np.sum(_soft(x)) + pen
    dl = np.sum(sg * np.expm1(dx) + C['l'] * _ulp32(x)) + (B + 72 + (d * kh) ** 0.5) * U32 * val
    out['loss'] = (val, val - dl, val + dl)
    out['alpha'], out['beta'] = alpha, beta
    return out


# ---------------------------------------------------------------------------------------------------------------- the cases
HP = dict(lu=2.5e-3, li=2.5e-3, lj=2.5e-4, lb=1e-3, lr=0.05)


def toy(n_users, n_items, seed, max_deg=12):
    """the training rows of tests/test_gpu_bpr.py / test_gpu_flow.py"""
    rng = np.random.Generator(np.random.PCG64(seed))
    tr = {}
    for u in rng.permutation(n_users)[: max(1, n_users - n_users // 8)]:
        tr[int(u)] = [int(x) for x in rng.integers(0, n_items, int(rng.integers(1, max_deg)))]
    return tr, list(tr.keys())


def triplets(tr, tr_users, n_users, n_items, seed, B):
    """K1's stream restated (oracle/plan_np.py): the ids of batch 0"""
    from oracle import plan_np as P
    row_ptr, pos, srt = P.build_csr(tr, n_users)
    return P.sample_triplets(tr_users, row_ptr, pos, srt, n_items, seed, 0, B)

N_USERS, N_ITEMS = 400, 120
# (k, B, mode, opt): the shapes of tests/test_gpu_step_regimes.py for K2 (tkr_bpr_run) ...
BPR_CASES = [(16, 256, 'l2', 'rmsprop'), (16, 256, 'l1', 'rmsprop'), (128, 256, 'l2', 'rmsprop'), (128, 256, 'l1', 'rmsprop'),
             (300, 256, 'l2', 'rmsprop'), (300, 256, 'l1', 'rmsprop'), (512, 256, 'l2', 'rmsprop'), (512, 256, 'l1', 'rmsprop'),
             (128, 2048, 'l2', 'rmsprop'), (128, 2048, 'l1', 'rmsprop'), (600, 256, 'l2', 'rmsprop'), (600, 256, 'l1', 'rmsprop'),
             (300, 2048, 'l2', 'rmsprop'), (300, 2048, 'l1', 'rmsprop'), (128, 256, 'l2', 'sgd')]
# ... and for K2f / K2o
FLOW_CASES = [(k, 256, mode, 'rmsprop') for k in (16, 128, 256) for mode in ('l2', 'l1')]


def state_kw(k):
    """the recipe as measured, but for k = 600: x is a sum of 1,200 terms there, and with factors of N(0, 0.5^2) 2.7 % of the elements
    of U have an interval wider than 10 x the step tolerance (fewer x16 rows do not change that: 2.8 %); with N(0, 0.2^2) 98 % are
    within it and |x| still reaches 60"""
    return dict(sd=0.2) if k >= 600 else {}


_CACHE = {}


def bpr_case(k, B, mode, opt, plant=True):
    """-> dict(state, tr, tr_users, u, i, j, hp, out): the regime state (with one planted ms = 0, g = 0 element), K1's ids of batch 0
    with seed 42, and the float64 step with its intervals -- computed once per case and shared; nothing of it may be changed"""
    key = (k, B, mode, opt, plant)
    if key not in _CACHE:
        tr, tr_users = toy(N_USERS, N_ITEMS, seed=k + B)
        u, i, j = triplets(tr, tr_users, N_USERS, N_ITEMS, 42, B)
        st = trained_state(N_USERS, N_ITEMS, k, np.random.Generator(np.random.PCG64(k)), **state_kw(k))
        if plant:
            once = np.flatnonzero(np.bincount(u, minlength=N_USERS)[u] == 1)
            if len(once):
                t = int(once[0])
                plant_zero_gradient(st, u[t], i[t], j[t])
        hp = dict(HP, mode=mode, opt=opt)
        _CACHE[key] = dict(state=st, tr=tr, tr_users=tr_users, u=u, i=i, j=j, hp=hp, out=bpr_step64(st, u, i, j, hp))
    return _CACHE[key]


# K3: (k, d, B, mode, dense features)
VBPR_USERS, VBPR_ITEMS = 300, 90
VBPR_HP = dict(lu=2.5e-3, li=2.5e-3, lj=2.5e-4, lb=1e-3, le=1e-3, lr=0.02)
VBPR_CASES = [(16, 40, 64, 'l2', True), (128, 700, 256, 'l2', False), (50, 333, 128, 'l1', False), (600, 333, 128, 'l2', False),
              (64, 300, 2048, 'l2', False)]
VBPR_NAMES = ('ure', 'uce', 'ire', 'irb', 'cem', 'icb')


def vbpr_toy(n_users, n_items, seed):
    """the training rows of tests/test_gpu_vbpr.py"""
    rng = np.random.Generator(np.random.PCG64(seed))
    tr = {int(u): [int(x) for x in rng.integers(0, n_items, int(rng.integers(1, 10)))] for u in rng.permutation(n_users)[: n_users - 5]}
    return tr, list(tr.keys())


def vbpr_case(k, d, B, mode, dense, **kw):
    """as bpr_case: row-normalised features (tf-idf-like sparsity unless ``dense``), K1's ids of batch 0 with seed 5"""
    key = ('vbpr', k, d, B, mode, dense, tuple(sorted(kw.items())))
    if key not in _CACHE:
        n_users, n_items = VBPR_USERS, VBPR_ITEMS
        tr, tr_users = vbpr_toy(n_users, n_items, seed=k + d)
        rng = np.random.Generator(np.random.PCG64(d))
        feat = np.abs(rng.standard_normal((n_items, d))).astype(F32)
        if not dense:
            feat *= rng.random((n_items, d)) < 0.1
        feat = (feat / np.maximum(np.linalg.norm(feat, axis=1, keepdims=True), 1e-6)).astype(F32)
        u, i, j = triplets(tr, tr_users, n_users, n_items, 5, B)
        st = scale_vbpr_state(trained_vbpr_state(n_users, n_items, k, d, feat, rng, **kw), feat, u, i, j)
        hp = dict(VBPR_HP, mode=mode)
        _CACHE[key] = dict(state=st, feat=feat, tr=tr, tr_users=tr_users, u=u, i=i, j=j, hp=hp, out=vbpr_step64(st, feat, u, i, j, hp))
    return _CACHE[key]


# K9 / K10: (k, steps, mode); 16 triplets a step
FOLD_CASES = [(128, 1, 'l2'), (128, 5, 'l2'), (128, 1, 'l1'), (128, 5, 'l1'), (600, 1, 'l2'), (600, 5, 'l1')]
FOLD_P, FOLD_SEED, FOLD_LR = 16, 11, 0.05


def fold_kw(side, k, T):
    """One step: the recipe (k = 600: factors of N(0, 0.15^2), as state_kw).  Five steps: the step map of a row is expansive in this
    regime -- d(update)/d(row) ~ lr sigma' |p|^2 per triplet, 16 triplets, |p|^2 = k / 2 with the recipe's factors -- so the interval
    of step t widens that of step t + 1 several times over and is vacuous after five.  The five-step states take the saturation from
    the biases instead (N(0, 6^2): |x| to 30) and factors small enough that 98 % of the intervals stay within 10 x the step
    tolerance (measured on the CPU; the item side sees the x 16 user rows as its p and needs smaller ones)."""
    if T == 1:
        return dict(sd=0.15) if k >= 600 else {}
    sd = {('user', 128): 0.1, ('user', 600): 0.05, ('item', 128): 0.05, ('item', 600): 0.03}[(side, k)]
    return dict(sd=sd, sb=6.0)


def fold_user_case(k, T, mode):
    """K9: 24 histories over 500 items; V, b and the start vectors (rows x 4 and x 16, exact zeros of both signs) from the regime
    state; the draw of tests/_foldin_oracle.py"""
    key = ('k9', k, T, mode)
    if key not in _CACHE:
        import _foldin_oracle as FO
        rng = np.random.Generator(np.random.PCG64(1000 + k))
        n_items, m = 500, 24
        hist = [np.sort(rng.choice(n_items, d, replace=False)).astype(np.int32) for d in [1, 2, 37, 499] + [int(x) for x in rng.integers(1, 60, m - 4)]]
        ptr, cols = FO.csr(hist)
        st = trained_state(m, n_items, k, rng, **fold_kw('user', k, T))
        trip = FO.draw(ptr, cols, n_items, FOLD_SEED, T, FOLD_P)
        box, loss = fold_user64(st['V'], st['b'], st['U'], trip, HP['lu'], FOLD_LR, mode)
        _CACHE[key] = dict(V=st['V'], b=st['b'], U0=st['U'], ptr=ptr, cols=cols, trip=trip, box=box, loss=loss)
    return _CACHE[key]


def fold_item_case(k, T, mode):
    """K10: the 300 users x 200 items and eight new items (1 .. 300 likers, one without any) of tests/_item_foldin_oracle.shapes;
    U, V, b from the regime state, the new rows' start from its recipe for item rows"""
    key = ('k10', k, T, mode)
    if key not in _CACHE:
        import _item_foldin_oracle as IO
        uptr, ucols, _, lptr, lrows, likers = IO.shapes()
        rng = np.random.Generator(np.random.PCG64(2000 + k))
        kw = fold_kw('item', k, T)
        st = trained_state(IO.N_USERS, IO.N_ITEMS, k, rng, **kw)
        m = len(likers)
        V0 = _factor(rng, m, k, True, kw.get('sd', 0.5))
        b0 = rng.standard_normal(m).astype(F32)
        b0[1] = 0.0
        thresh = IO.role_thresh(uptr, lptr, lrows, IO.N_ITEMS)
        trip, _ = IO.draw(uptr, ucols, lptr, lrows, thresh, IO.N_ITEMS, FOLD_SEED, T, FOLD_P)
        Vb, bb, loss = fold_item64(st['U'], st['V'], st['b'], V0, b0, trip, HP['li'], HP['lj'], HP['lb'], FOLD_LR, mode)
        _CACHE[key] = dict(U=st['U'], V=st['V'], b=st['b'], V0=V0, b0=b0, uptr=uptr, ucols=ucols, lptr=lptr, lrows=lrows, thresh=thresh,
                           trip=trip, Vbox=Vb, bbox=bb, loss=loss)
    return _CACHE[key]


# K16: (M, B)
FUSION_CASES = [(3, 1000), (8, 1000)]
FUSION_LR, FUSION_LAMBDA = 0.05, 1e-3


def fusion_case(M, B):
    """score differences D [B, M] and weights W ~ N(0, 8^2), D scaled so that x = D W spans +-100; some rows of D all zero.  (With W ~ N(0, 1) the same x needs |D| eight times larger, the gradient is a sum of 1,000 terms of that size, and the
    bound of an fp32 sum in ANY order leaves a third of the weights with an interval wider than 10 x the step tolerance.)"""
    key = ('k16', M, B)
    if key not in _CACHE:
        rng = np.random.Generator(np.random.PCG64(3000 + M))
        W = (rng.standard_normal(M) * 8).astype(F32)
        D = (rng.standard_normal((B, M)) * 10 ** rng.uniform(-2, 0, (B, 1))).astype(F32)
        D = (D * F32(100.0 / np.abs(D.astype(np.float64) @ W).max())).astype(F32)
        D[::37] = 0.0
        box, cost = fusion_step64(W, D, FUSION_LR, FUSION_LAMBDA)
        _CACHE[key] = dict(W=W, D=D, box=box, cost=cost)
    return _CACHE[key]
