"""-m gpu: the training-step kernels in the TRAINED regime -- |x| from 0 to > 100 (saturated sigmoids of both signs), RMSProp slots
from 1e-14 to 1 with exact zeros, exact +0.0 / -0.0 in the tables -- against the float64 oracle of tests/_regime_oracle.py, which
returns an INTERVAL per element (the constants of the interval are fixed there, from the fp32 oracles; tests/test_step_regimes_cpu.py).

Every case: ONE batch from the regime state on K1's own ids; every result finite and inside its interval (no element excluded);
the rows that were not drawn bit-unchanged, slots included; the loss inside its interval.

Which case reaches which kernel:

* K2 ``tkr_bpr_run`` (csrc/bpr_step.hip), l2 and l1 -- k = 16: partly filled lanes; k = 128; k = 300: k % 64 != 0, the clamped loads;
  k = 512 at B = 256; k = 128 at B = 2048: the large-batch workgroups; ``bpr_wide_kernel``: k = 600 at B = 256 and k = 300 at
  B = 2048; opt = sgd at k = 128 (test_k2_*).
* K2f (csrc/bpr_flow.hip, flow_task.h: fast_sigmoid_neg, rsq) with 2 and 4 buffers per item row, K2o (csrc/bpr_own.hip) on the
  device's owner count ('o') and on 8 owners ('o8'): k = 16, 128, 256 at B = 256, l2 and l1, with the bookkeeping checks of
  tests/test_gpu_flow.py::_check (test_k2f_k2o_*).
* K3 (csrc/vbpr_step.hip, vbpr_cols.hip, vbpr_rows.h, vbpr_wide.hip: pair_exp / pair_sigmoid / pair_softplus_neg) -- (k, d, B) =
  (16, 40, 64) dense features, (128, 700, 256) sparse, (50, 333, 128) l1, both views; TKR_VBPR_COLS=0 once (the four-launch walk);
  k = 600: vbpr_wide.hip; B = 2048: the blocked pair sums; dense RMSProp on cem / icb with slots from the recipe (test_k3_*).
* K9 / K10 (csrc/fold_rows.h) -- item table and biases from the regime state, the row's own slot where the kernel starts it; one
  step and five steps; k = 128 (registers) and k = 600 (LDS); l1 with zeros in the start vector (test_k9_*, test_k10_*).
* K16 ``tkr_fusion_sgd`` (csrc/fusion.hip) -- M = 3 and 8, one batch of 1,000, D scaled so that x spans +-100 (test_k16_*).

Each test prints the largest share of an interval its kernel used; DESIGN.md section 2 quotes the MI355X run."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _regime_oracle as O
from test_gpu_bpr import _current, _run_plan, _state_struct, _tables
from test_gpu_flow import _Flow, _check, _owners, _plan

pytestmark = pytest.mark.gpu

F32 = np.float32
NU, NI = O.N_USERS, O.N_ITEMS


@pytest.fixture(scope='module')
def hip():
    import tkr_hip
    assert torch.cuda.is_available(), 'GPU tests need a MI355X'
    tkr_hip.lib()
    return tkr_hip


def _bits(a):
    return np.ascontiguousarray(a, dtype=F32).view(np.int32)


def _judge(tag, out, got, names, loss=None):
    """every element finite and inside its interval; untouched elements bit-equal to the state; the loss inside its interval"""
    worst = {}
    for n in names:
        g = np.asarray(got[n])
        assert np.isfinite(g).all(), '%s: %s has non-finite elements' % (tag, n)
        box = out[n]
        sh = O.share(box, g)
        worst[n] = float(sh[box.touched].max()) if box.touched.any() else 0.0
        rest = ~box.touched
        assert np.array_equal(_bits(g)[rest], _bits(box.val)[rest]), '%s: untouched elements of %s changed' % (tag, n)
    if loss is not None:
        val, lo, hi = out['loss']
        assert np.isfinite(loss), tag
        worst['loss'] = abs(float(loss) - val) / (hi - val)
    print('%s: share of the interval used: %s' % (tag, ' '.join('%s %.3f' % kv for kv in worst.items())))
    bad = {n: v for n, v in worst.items() if not v <= 1.0}
    assert not bad, '%s: outside the interval: %s' % (tag, bad)
    return worst


def _ids_are_k1s(c, exp):
    for name, got in zip(('u', 'i', 'j'), exp[:3]):
        np.testing.assert_array_equal(np.asarray(got).reshape(-1)[:len(c[name])], c[name], err_msg=name)


# ------------------------------------------------------------------------------------------------------------------ K2
@pytest.mark.parametrize('k,B,mode,opt', O.BPR_CASES)
def test_k2_step_in_the_trained_regime(hip, k, B, mode, opt):
    c = O.bpr_case(k, B, mode, opt)
    st, hp = c['state'], c['hp']
    T = _tables(st, NU, NI, k)
    for n in ('msU', 'msV', 'msb'):
        T[n][0] = torch.from_numpy(st[n]).cuda()
    before = {n: T[n].clone() for n in T}
    _, exp, plan = _run_plan(hip, c['tr'], c['tr_users'], NU, NI, seed=42, first=0, nb=1, B=B)
    _ids_are_k1s(c, exp)
    S = _state_struct(hip, T, NU, NI, k, hp)
    if opt == 'sgd':
        S.msU = S.msV = S.msb = None
    loss = torch.zeros(1, device='cuda')
    hip.bpr_run(S, plan, B, 1, loss)
    torch.cuda.synchronize()
    ucnt, icnt = np.zeros(NU, np.int32), np.zeros(NI, np.int32)
    ucnt[np.unique(c['u'])] = 1
    icnt[np.unique(np.concatenate([c['i'], c['j']]))] = 1
    names = ('U', 'V', 'b') if opt == 'sgd' else ('U', 'V', 'b', 'msU', 'msV', 'msb')
    got = {n: _current(T, n, ucnt if n.endswith('U') else icnt) for n in names}
    _judge('K2 k=%d B=%d %s %s' % (k, B, mode, opt), c['out'], got, names, float(loss[0]))
    # both buffers of a row that was not drawn, and the read buffer of a row that was, are as they were
    for n in T:
        if opt == 'sgd' and n.startswith('ms'):
            assert torch.equal(T[n].view(torch.int32), before[n].view(torch.int32))
            continue
        cnt = torch.from_numpy(ucnt if n.endswith('U') else icnt).cuda()
        assert torch.equal(T[n].view(torch.int32)[:, cnt == 0], before[n].view(torch.int32)[:, cnt == 0]), n
        assert torch.equal(T[n].view(torch.int32)[0], before[n].view(torch.int32)[0]), n


# ------------------------------------------------------------------------------------------------------------ K2f, K2o
@pytest.mark.parametrize('kernel,bufs', [('f', 2), ('f', 4), ('o', 2), ('o8', 4)])
@pytest.mark.parametrize('k,B,mode,opt', O.FLOW_CASES)
def test_k2f_k2o_step_in_the_trained_regime(hip, k, B, mode, opt, kernel, bufs):
    c = O.bpr_case(k, B, mode, opt)
    st, hp = c['state'], c['hp']
    F = _Flow(hip, st, NU, NI, k, hp, bufs=bufs)               # (takes ref['ms*'] from the state)
    plan, exp, _, _ = _plan(hip, c['tr'], c['tr_users'], NU, NI, 42, 0, 1, B, owners=_owners(hip, kernel, NI, k))
    _ids_are_k1s(c, exp)
    loss = torch.zeros(1, device='cuda')
    F.run(plan, B, 1, loss, kernel=kernel)
    status, _ = F.status()
    assert status == 0
    ucnt, icnt = np.zeros(NU, np.int32), np.zeros(NI, np.int32)
    uocc, iocc = np.bincount(c['u'], minlength=NU), np.bincount(np.concatenate([c['i'], c['j']]), minlength=NI)
    ucnt[uocc > 0] = 1
    icnt[iocc > 0] = 1
    got = F.current(ucnt, icnt)
    names = ('U', 'V', 'b', 'msU', 'msV', 'msb')
    _judge('K2%s bufs=%d k=%d %s' % (kernel, bufs, k, mode), c['out'], got, names, float(loss[0]))
    # the bookkeeping checks of test_gpu_flow.py::_check, with the oracle's values standing in for its reference (the fixed
    # tolerance of _check is not the instrument here: elements whose interval is wider than it exist, and are judged above)
    ref = {n: got[n] for n in names}
    _check(F, ref, ucnt, icnt, uocc.astype(np.int64), iocc.astype(np.int64))


# ------------------------------------------------------------------------------------------------------------------ K3
def _k3(case, view, tag):
    from single import _engine
    from oracle import plan_np as P
    k, d, B, mode, dense = case
    kh = k // 2
    c = O.vbpr_case(*case)
    st, feat, hp = c['state'], c['feat'], c['hp']
    dev = torch.device('cuda')
    eng = _engine.VbprEngine(O.VBPR_USERS, O.VBPR_ITEMS, k, d, feat, hp, dev, seed=5, sparse=(view == 'sparse'))
    assert (eng.sparse is not None) == (view == 'sparse')
    eng.set_users(U=np.concatenate([st['ure'], st['uce']], axis=1), msU=np.concatenate([st['ms_ure'], st['ms_uce']], axis=1))
    eng.set_items(I=st['ire'], irb=st['irb'], msI=st['ms_ire'], msirb=st['ms_irb'])
    eng.set_dense(cem=st['cem'], icb=st['icb'], mscem=st['ms_cem'], msicb=st['ms_icb'])
    row_ptr, pos, srt = P.build_csr(c['tr'], O.VBPR_USERS)
    csr = _engine.TrainingCSR.from_arrays(row_ptr, pos, np.asarray(c['tr_users'], np.int32), dev)
    import warnings
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')                               # (k = 600: the one warning of the generic form)
        loss = eng.run_batches(csr, 1, B).cpu().numpy()
    torch.cuda.synchronize()
    for name in ('u', 'i', 'j'):
        np.testing.assert_array_equal(getattr(eng.plan, name).cpu().numpy()[:B], c[name], err_msg=name)
    Uc, msU = (t.cpu().numpy() for t in eng.get('U'))
    Ic, msI = (t.cpu().numpy() for t in eng.get('I'))
    bc, msb = (t.cpu().numpy() for t in eng.get('irb'))
    got = dict(ure=Uc[:, :kh], uce=Uc[:, kh:], ms_ure=msU[:, :kh], ms_uce=msU[:, kh:], ire=Ic, ms_ire=msI, irb=bc.reshape(-1), ms_irb=msb.reshape(-1),
               cem=eng.cem.cpu().numpy(), icb=eng.icb.cpu().numpy().reshape(-1), ms_cem=eng.mscem.cpu().numpy(),
               ms_icb=eng.msicb.cpu().numpy().reshape(-1))
    names = tuple(n for base in O.VBPR_NAMES for n in (base, 'ms_' + base))
    a, b = c['out']['alpha'], c['out']['beta']
    assert max(np.abs(a).max(), np.abs(b).max()) < 80 and (a[:, None] + b[None, :]).max() > 89 and (a[:, None] + b[None, :]).min() < -89
    return eng, _judge('K3 %s %s %s' % (case, view, tag), c['out'], got, names, float(loss[0]))


@pytest.mark.parametrize('view', ['dense', 'sparse'])
@pytest.mark.parametrize('case', O.VBPR_CASES[:3])
def test_k3_step_in_the_trained_regime(case, view):
    _k3(case, view, '')


def test_k3_four_launch_walk_in_the_trained_regime(monkeypatch):
    monkeypatch.setenv('TKR_VBPR_COLS', '0')
    eng, _ = _k3(O.VBPR_CASES[1], 'sparse', 'TKR_VBPR_COLS=0')
    assert not eng.wants_cols(256)


def test_k3_wide_form_in_the_trained_regime():
    eng, _ = _k3(O.VBPR_CASES[3], 'sparse', 'vbpr_wide')
    assert eng.kh > 128


def test_k3_blocked_pair_sums_in_the_trained_regime():
    eng, _ = _k3(O.VBPR_CASES[4], 'sparse', 'B=2048')
    assert not eng.wants_cols(2048)


# ------------------------------------------------------------------------------------------------------------- K9, K10
def _dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to('cuda')


@pytest.mark.parametrize('k,T,mode', O.FOLD_CASES)
def test_k9_user_fold_in_from_the_trained_regime(hip, k, T, mode):
    c = O.fold_user_case(k, T, mode)
    import warnings
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')                               # (k = 600: the one warning of the generic form)
        U, loss, trip = hip.fold_in(_dev(c['V']), _dev(c['b']), _dev(c['ptr']), _dev(c['cols']), lu=O.HP['lu'], lr=O.FOLD_LR, mode=mode, steps=T,
                                    triplets=O.FOLD_P, seed=O.FOLD_SEED, U0=_dev(c['U0']), want_loss=True, want_triplets=True)
    np.testing.assert_array_equal(trip.cpu().numpy(), c['trip'])
    assert (c['U0'] == 0).any() and np.signbit(c['U0'][c['U0'] == 0]).any()
    tag = 'K9 k=%d T=%d %s' % (k, T, mode)
    _judge(tag, dict(U=c['box']), dict(U=U.cpu().numpy()), ('U',))
    loss = loss.cpu().numpy().astype(np.float64)
    val, lo, hi = c['loss']
    assert np.isfinite(loss).all()
    used = np.abs(loss - val) / (hi - val)
    print('%s: share of the loss intervals used: %.3f' % (tag, used.max()))
    assert (used <= 1.0).all()


@pytest.mark.parametrize('k,T,mode', O.FOLD_CASES)
def test_k10_item_fold_in_from_the_trained_regime(hip, k, T, mode):
    c = O.fold_item_case(k, T, mode)
    import warnings
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        Vn, bn, loss, trip = hip.fold_in_items(_dev(c['U']), _dev(c['V']), _dev(c['b']), _dev(c['uptr']), _dev(c['ucols']), _dev(c['lptr']),
                                               _dev(c['lrows']), c['thresh'], li=O.HP['li'], lj=O.HP['lj'], lb=O.HP['lb'], lr=O.FOLD_LR, mode=mode,
                                               steps=T, triplets=O.FOLD_P, seed=O.FOLD_SEED, V0=_dev(c['V0']), b0=_dev(c['b0']),
                                               want_loss=True, want_triplets=True)
    np.testing.assert_array_equal(trip.cpu().numpy(), c['trip'])
    tag = 'K10 k=%d T=%d %s' % (k, T, mode)
    _judge(tag, dict(V=c['Vbox'], b=c['bbox']), dict(V=Vn.cpu().numpy(), b=bn.cpu().numpy()), ('V', 'b'))
    loss = loss.cpu().numpy().astype(np.float64)
    val, lo, hi = c['loss']
    live = c['bbox'].touched
    assert np.isfinite(loss).all() and live.any()
    used = np.abs(loss - val)[live] / (hi - val)[live]
    print('%s: share of the loss intervals used: %.3f' % (tag, used.max()))
    assert (used <= 1.0).all()


# ----------------------------------------------------------------------------------------------------------------- K16
@pytest.mark.parametrize('M,B', O.FUSION_CASES)
def test_k16_fusion_sgd_in_the_trained_regime(hip, M, B):
    c = O.fusion_case(M, B)
    x = c['D'].astype(np.float64) @ c['W']
    assert x.max() > 50 and x.min() < -50 and np.abs(x).max() >= 99
    W = _dev(c['W'].copy())
    W, loss = hip.fusion_sgd(_dev(c['D']), B, 1, O.FUSION_LR, O.FUSION_LAMBDA, W, want_loss=True)
    torch.cuda.synchronize()
    out = dict(W=c['box'], loss=c['cost'])
    _judge('K16 M=%d' % M, out, dict(W=W.cpu().numpy()), ('W',), float(loss[0]))
