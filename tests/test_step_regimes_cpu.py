"""The interval oracle of tests/_regime_oracle.py checked on the CPU, without a GPU:

* the fp32 oracles (oracle/ref_np.bpr_step / vbpr_step, tests/_foldin_oracle.py, _item_foldin_oracle.py, _fusion_oracle.py) use at
  most HALF of every interval, on every element of every shape that tests/test_gpu_step_regimes.py runs;
* the intervals are not vacuous: on every table at least 98 % of the touched elements have an interval no wider than 10 x the
  project's step tolerance (1e-5 + 2e-4 |P|; K3: 2e-5 + 3e-4 |P|);
* the check FAILS for seven mutations of an fp32 NumPy step -- the mistakes the regime exists to catch."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _regime_oracle as O
from oracle import ref_np as R

F32 = np.float32
TABLES = ('U', 'V', 'b', 'msU', 'msV', 'msb')


def _shares(out, got, names, record, tag):
    worst = {}
    for n in names:
        sh = O.share(out[n], got[n])
        worst[n] = float(sh[out[n].touched].max())
        rest = ~out[n].touched
        assert np.array_equal(np.asarray(got[n])[rest].view(np.int32), np.asarray(out[n].val[rest], dtype=F32).view(np.int32)), n
        record[n] = max(record.get(n, 0.0), worst[n])
    print(tag, ' '.join('%s %.3f' % kv for kv in worst.items()))
    return worst


def _wide_share(box, atol, rtol):
    h, p = box.half()[box.touched], np.abs(box.val[box.touched])
    return float((h > 10 * (atol + rtol * p)).mean())


BPR_RECORD = {}


@pytest.mark.parametrize('k,B,mode,opt', O.BPR_CASES + O.FLOW_CASES)
def test_fp32_oracle_uses_half_of_the_bpr_intervals(k, B, mode, opt):
    c = O.bpr_case(k, B, mode, opt)
    ref = {n: v.copy() for n, v in c['state'].items()}
    loss = R.bpr_step(ref, c['u'], c['i'], c['j'], c['hp'])
    names = TABLES[:3] if opt == 'sgd' else TABLES
    worst = _shares(c['out'], ref, names, BPR_RECORD, 'k=%d B=%d %s %s:' % (k, B, mode, opt))
    assert max(worst.values()) <= 0.5
    val, lo, hi = c['out']['loss']
    assert np.isfinite(loss) and abs(float(loss) - val) <= 0.5 * (hi - val)
    # the regime is the regime: saturated triplets of both signs, slots at zero, zeros in the tables
    x = c['out']['x']
    assert np.abs(x).max() > 30 and (x > 17).any() and (x < -17).any()
    assert (c['state']['msU'] == 0).any() and (c['state']['U'] == 0).any() and np.signbit(c['state']['U'][c['state']['U'] == 0]).any()


@pytest.mark.parametrize('k,B,mode,opt', O.BPR_CASES + O.FLOW_CASES)
def test_bpr_intervals_are_not_vacuous(k, B, mode, opt):
    out = O.bpr_case(k, B, mode, opt)['out']
    for n in ('U', 'V', 'b'):
        assert _wide_share(out[n], 1e-5, 2e-4) <= 0.02, n
    val, lo, hi = out['loss']
    assert hi - val <= 2e-3 * val                        # (the other step tests compare the loss at 1e-4 .. 1e-3 relative)


VBPR_RECORD, FOLD_RECORD, FUSION_RECORD = {}, {}, {}


@pytest.mark.parametrize('case', O.VBPR_CASES)
def test_fp32_oracle_uses_half_of_the_vbpr_intervals_and_they_are_not_vacuous(case):
    c = O.vbpr_case(*case)
    ref = {n: v.copy() for n, v in c['state'].items()}
    loss = R.vbpr_step(ref, c['feat'], c['u'], c['i'], c['j'], c['hp'])
    names = tuple(n for base in O.VBPR_NAMES for n in (base, 'ms_' + base))
    worst = _shares(c['out'], ref, names, VBPR_RECORD, 'K3 %s:' % (case,))
    assert max(worst.values()) <= 0.5
    val, lo, hi = c['out']['loss']
    assert np.isfinite(loss) and abs(float(loss) - val) <= 0.5 * (hi - val) and hi - val <= 2e-3 * val
    for n in O.VBPR_NAMES:
        assert _wide_share(c['out'][n], 2e-5, 3e-4) <= 0.02, n
    # alpha and beta inside the documented +-80, both signs, and pairs whose e^alpha e^beta overflows / underflows in fp32
    a, b = c['out']['alpha'], c['out']['beta']
    assert max(np.abs(a).max(), np.abs(b).max()) < 80 and min(a.max(), -a.min(), b.max(), -b.min()) > 40
    assert a.max() + b.max() > 89 and a.min() + b.min() < -89
    assert (c['state']['ms_cem'] == 0).any() and (c['state']['cem'] == 0).any() and (c['state']['icb'] == 0).any()


@pytest.mark.parametrize('k,T,mode', O.FOLD_CASES)
def test_fp32_oracle_uses_half_of_the_fold_in_intervals_and_they_are_not_vacuous(k, T, mode):
    import _foldin_oracle as FO
    import _item_foldin_oracle as IO
    c = O.fold_user_case(k, T, mode)
    U32, l32 = FO.fold_in(c['V'], c['b'], c['ptr'], c['cols'], c['trip'], O.HP['lu'], O.FOLD_LR, mode, U0=c['U0'])
    worst = _shares(dict(U=c['box']), dict(U=U32), ('U',), FOLD_RECORD, 'K9 k=%d T=%d %s:' % (k, T, mode))
    val, lo, hi = c['loss']
    assert worst['U'] <= 0.5 and (np.abs(l32 - val) <= 0.5 * (hi - val)).all() and (hi - val <= 5e-3 * np.abs(val) + 1e-5).all()
    assert _wide_share(c['box'], 1e-5, 2e-4) <= 0.02
    assert (c['U0'] == 0).any() and np.signbit(c['U0'][c['U0'] == 0]).any()
    c = O.fold_item_case(k, T, mode)
    V32, b32, l32 = IO.fold_in_items(c['U'], c['V'], c['b'], c['trip'], O.HP['li'], O.HP['lj'], O.HP['lb'], O.FOLD_LR, mode, V0=c['V0'], b0=c['b0'])
    rec = {}
    worst = _shares(dict(V=c['Vbox'], b=c['bbox']), dict(V=V32, b=b32), ('V', 'b'), rec, 'K10 k=%d T=%d %s:' % (k, T, mode))
    FOLD_RECORD['Vn'], FOLD_RECORD['bn'] = max(FOLD_RECORD.get('Vn', 0), rec['V']), max(FOLD_RECORD.get('bn', 0), rec['b'])
    val, lo, hi = c['loss']
    live = c['bbox'].touched
    assert max(worst.values()) <= 0.5 and (np.abs(l32 - val) <= 0.5 * (hi - val))[live].all()
    assert _wide_share(c['Vbox'], 1e-5, 2e-4) <= 0.02 and _wide_share(c['bbox'], 1e-5, 2e-4) <= 0.02


@pytest.mark.parametrize('M,B', O.FUSION_CASES)
def test_fp32_oracle_uses_half_of_the_fusion_intervals_and_they_are_not_vacuous(M, B):
    import _fusion_oracle as FU
    c = O.fusion_case(M, B)
    W32, cost = FU.sgd_step(c['W'].copy(), c['D'], F32(O.FUSION_LR), F32(O.FUSION_LAMBDA))
    assert W32.dtype == F32
    worst = _shares(dict(W=c['box']), dict(W=W32), ('W',), FUSION_RECORD, 'K16 M=%d:' % M)
    val, lo, hi = c['cost']
    assert worst['W'] <= 0.5 and abs(float(cost) - val) <= 0.5 * (hi - val) and hi - val <= 2e-3 * val
    assert _wide_share(c['box'], 1e-5, 2e-4) <= 0.02
    x = c['D'].astype(np.float64) @ c['W']
    assert x.max() > 50 and x.min() < -50 and np.abs(x).max() >= 99


def test_recorded_shares_are_the_measured_ones():
    """tests/_regime_oracle.MEASURED (quoted in its docstring and in DESIGN.md section 2) holds the largest share per table that the
    fp32 oracles used over all cases; a change of the oracle or of a case that moves one is a reason to look at the constants again"""
    for case in O.BPR_CASES + O.FLOW_CASES:
        test_fp32_oracle_uses_half_of_the_bpr_intervals(*case)
    for case in O.VBPR_CASES:
        test_fp32_oracle_uses_half_of_the_vbpr_intervals_and_they_are_not_vacuous(case)
    for case in O.FOLD_CASES:
        test_fp32_oracle_uses_half_of_the_fold_in_intervals_and_they_are_not_vacuous(*case)
    for case in O.FUSION_CASES:
        test_fp32_oracle_uses_half_of_the_fusion_intervals_and_they_are_not_vacuous(*case)
    print({g: {n: round(v, 3) for n, v in rec.items()} for g, rec in (('bpr', BPR_RECORD), ('vbpr', VBPR_RECORD), ('fold', FOLD_RECORD),
                                                                       ('fusion', FUSION_RECORD))})
    for group, rec in (('bpr', BPR_RECORD), ('vbpr', VBPR_RECORD), ('fold', FOLD_RECORD), ('fusion', FUSION_RECORD)):
        for n, v in rec.items():
            assert v <= O.MEASURED[group][n] + 0.02 <= 0.52, (group, n, v)      # (0.02: another NumPy build's exp / log1p may round another way)


# ------------------------------------------------------------------------------------------------------------- mutations
def _sig32(x, mut):
    x = x.astype(F32)
    if mut == 'sigma_one_minus':                          # sigma(-x) as 1 - 1 / (1 + exp(-x)): 0 from x = 17 on
        with np.errstate(over='ignore'):
            return (F32(1) - F32(1) / (F32(1) + np.exp(-x).astype(F32))).astype(F32)
    e = np.exp(-np.abs(x)).astype(F32)
    return np.where(x >= 0, e / (F32(1) + e), F32(1) / (F32(1) + e)).astype(F32)


def _soft32(x, mut):
    x = x.astype(F32)
    if mut == 'softplus_naive':
        with np.errstate(over='ignore'):
            return np.log(F32(1) + np.exp(-x).astype(F32)).astype(F32)
    return (np.maximum(-x, F32(0)) + np.log1p(np.exp(-np.abs(x)))).astype(F32)


def _sign32(v, mut):
    return np.where(v == 0, F32(1), np.sign(v)).astype(F32) if mut == 'sign_zero_is_one' else np.sign(v)


def _rms32(P, ms, rows, g, lr, mut):
    g = g.astype(F32)
    a, b_ = (R.RHO, F32(1) - R.RHO) if mut != 'rho_swapped' else (F32(1) - R.RHO, R.RHO)
    new = (a * ms[rows] + b_ * g * g).astype(F32)
    used = ms[rows].copy() if mut == 'old_slot' else new
    ms[rows] = new
    with np.errstate(invalid='ignore', divide='ignore'):
        if mut == 'eps_outside':
            den = (np.sqrt(used) + R.EPS).astype(F32)
        elif mut == 'eps_dropped':
            den = np.sqrt(used).astype(F32)
        else:
            den = np.sqrt(used + R.EPS).astype(F32)
        P[rows] = (P[rows] - F32(lr) * g / den).astype(F32)


def bpr_step32(state, ub, ib, jb, hp, mut=None):
    """oracle/ref_np.bpr_step (RMSProp) written out once more in fp32 NumPy, with one mistake switched on by ``mut``; mut = None is
    bit for bit ref_np.bpr_step (asserted below)"""
    U, V, b = state['U'], state['V'], state['b']
    lu, li, lj, lb = (F32(hp[n]) for n in ('lu', 'li', 'lj', 'lb'))
    ub, ib, jb = (np.asarray(a, dtype=np.int64) for a in (ub, ib, jb))
    ue, ie, je, bi, bj = U[ub], V[ib], V[jb], b[ib], b[jb]
    x = (bi - bj + np.sum(ue * ie, axis=1, dtype=F32) - np.sum(ue * je, axis=1, dtype=F32)).astype(F32)
    s = _sig32(x, mut)[:, None]
    if hp['mode'] == 'l2':
        loss = (np.sum(_soft32(x, mut), dtype=F32) + F32(0.5) * np.sum(ue * ue * lu + ie * ie * li + je * je * lj, dtype=F32)
                + F32(0.5) * np.sum(bi * bi + bj * bj, dtype=F32) * lb)
        ru, ri, rj, rbi, rbj = lu * ue, li * ie, lj * je, lb * bi, lb * bj
    else:
        loss = (np.sum(_soft32(x, mut), dtype=F32) + np.sum(np.abs(ue) * lu + np.abs(ie) * li + np.abs(je) * lj, dtype=F32)
                + np.sum(np.abs(bi) + np.abs(bj), dtype=F32) * lb)
        ru, ri, rj = lu * _sign32(ue, mut), li * _sign32(ie, mut), lj * _sign32(je, mut)
        rbi, rbj = lb * _sign32(bi, mut), lb * _sign32(bj, mut)
    gU = (-s * (ie - je) + ru).astype(F32)
    items = np.concatenate([ib, jb])
    rows_u, sum_u = R._segment_sum(ub, gU)
    rows_v, sum_v = R._segment_sum(items, np.concatenate([(-s * ue + ri).astype(F32), (s * ue + rj).astype(F32)]))
    rows_b, sum_b = R._segment_sum(items, np.concatenate([(-s[:, 0] + rbi).astype(F32), (s[:, 0] + rbj).astype(F32)]))
    _rms32(U, state['msU'], rows_u, sum_u, hp['lr'], mut)
    _rms32(V, state['msV'], rows_v, sum_v, hp['lr'], mut)
    _rms32(b, state['msb'], rows_b, sum_b, hp['lr'], mut)
    return F32(loss)


def _inside(out, got, loss):
    """the check of the GPU tests: every element finite and inside its interval, the loss inside its interval"""
    ok = all(bool((O.share(out[n], got[n]) <= 1.0).all()) for n in TABLES)
    return ok and bool(np.isfinite(loss)) and out['loss'][1] <= float(loss) <= out['loss'][2]


MUTATIONS = ['eps_outside', 'eps_dropped', 'sign_zero_is_one', 'softplus_naive', 'sigma_one_minus', 'rho_swapped', 'old_slot']


@pytest.mark.parametrize('mode', ['l2', 'l1'])
def test_the_unmutated_step_is_ref_np_and_passes(mode):
    c = O.bpr_case(128, 256, mode, 'rmsprop')
    a = {n: v.copy() for n, v in c['state'].items()}
    b = {n: v.copy() for n, v in c['state'].items()}
    la, lb = bpr_step32(a, c['u'], c['i'], c['j'], c['hp']), R.bpr_step(b, c['u'], c['i'], c['j'], c['hp'])
    assert la == lb
    for n in TABLES:
        np.testing.assert_array_equal(a[n], b[n])
    assert _inside(c['out'], a, la)


@pytest.mark.parametrize('mut', MUTATIONS)
def test_the_interval_check_fails_for_a_mutated_step(mut):
    mode = 'l1' if mut == 'sign_zero_is_one' else 'l2'
    c = O.bpr_case(128, 256, mode, 'rmsprop')
    got = {n: v.copy() for n, v in c['state'].items()}
    loss = bpr_step32(got, c['u'], c['i'], c['j'], c['hp'], mut)
    assert not _inside(c['out'], got, loss)
    if mut == 'eps_dropped':                              # ... and it shows as NaN at ms = 0, g = 0 (the planted element)
        assert np.isnan(got['U']).any()
    if mut == 'softplus_naive':
        assert not np.isfinite(loss)
    if mut == 'sigma_one_minus':                          # the tables alone give it away, not only the loss
        assert not all(bool((O.share(c['out'][n], got[n]) <= 1.0).all()) for n in TABLES)
