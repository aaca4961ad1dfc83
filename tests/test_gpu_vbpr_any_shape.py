"""VBPR at the shapes the column-plan step does not take (single/vbpr.py:18,76 set no limits): k // 2 > 128 with feature rows of more
than 1024 nonzeros, batches above 1024 or column counters beyond the LDS -- the generic form of the five-launch sparse view
(csrc/vbpr_wide.hip G1-G4) -- and batches above 65,536, where K1's wave records no longer carry a triplet's index in their 16-bit
halves (vbpr_rows.h read_rec takes it from occt).  Parity against oracle/ref_np.vbpr_step through VbprEngine, as
tests/test_gpu_vbpr.py::test_vbpr_step_parity does."""
import os
import pickle
import warnings

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import plan_np as P
from oracle import ref_np as R

F32 = R.F32
TOL = dict(rtol=3e-4, atol=2e-5)
# batches above 1024 on a few hundred rows: every S_t / T_t is a sum of B sigmoids and every item row sums dozens of occurrences, in
# another fp32 order than the oracle's (tests/test_gpu_vbpr.py::test_vbpr_four_launch_sparse_view_still_right: 1.4e-3 measured at 2048)
TOL_BIG = dict(rtol=3e-3, atol=1e-4)


def _toy(n_users, n_items, seed):
    rng = np.random.Generator(np.random.PCG64(seed))
    tr = {int(u): [int(x) for x in rng.integers(0, n_items, int(rng.integers(1, 10)))] for u in rng.permutation(n_users)[: n_users - 5]}
    return tr, list(tr.keys())


def _feat(n_items, d, seed, density=1.0, per_row=None):
    rng = np.random.Generator(np.random.PCG64(seed))
    if per_row is not None:                                          # a fixed number of nonzeros per row (a wide tf-idf vocabulary)
        feat = np.zeros((n_items, d), np.float32)
        for r in range(n_items):
            feat[r, rng.choice(d, per_row, replace=False)] = rng.random(per_row) + 0.1
    else:
        feat = np.abs(rng.standard_normal((n_items, d))).astype(np.float32)
        if density < 1.0:
            feat *= rng.random((n_items, d)) < density
    return (feat / np.maximum(np.linalg.norm(feat, axis=1, keepdims=True), 1e-6)).astype(np.float32)


def _setup(n_users, n_items, k, d, feat, hp, sparse=None, seed=5):
    from single import _engine
    dev = torch.device('cuda')
    kh = k // 2
    eng = _engine.VbprEngine(n_users, n_items, k, d, feat, hp, dev, seed=seed, sparse=sparse)
    rng = np.random.Generator(np.random.PCG64(d + k))
    eng.set_dense(cem=(rng.standard_normal((d, kh)) * 0.05).astype(np.float32), icb=(rng.standard_normal(d) * 0.05).astype(np.float32))
    eng.set_items(irb=(rng.standard_normal(n_items) * 0.01).astype(np.float32))
    U0 = eng.get('U')[0].cpu().numpy()
    ref = dict(ure=U0[:, :kh].copy(), uce=U0[:, kh:].copy(), ire=eng.get('I')[0].cpu().numpy(), irb=eng.get('irb')[0].cpu().numpy(),
               cem=eng.cem.cpu().numpy(), icb=eng.icb.cpu().numpy())
    for n in list(ref):
        ref['ms_' + n] = np.ones_like(ref[n])
    return eng, ref


def _run(eng, tr, tr_users, n_users, nb, B):
    from single import _engine
    row_ptr, pos, srt = P.build_csr(tr, n_users)
    csr = _engine.TrainingCSR.from_arrays(row_ptr, pos, np.asarray(tr_users, np.int32), eng.device)
    with warnings.catch_warnings(record=True) as seen:
        warnings.simplefilter('always')
        loss = eng.run_batches(csr, nb, B).cpu().numpy()
    torch.cuda.synchronize()
    u, i, j = P.sample_triplets(tr_users, row_ptr, pos, srt, eng.n_items, 5, 0, nb * B)
    np.testing.assert_array_equal(eng.plan.u.cpu().numpy()[: nb * B], u)     # K1's triplets: the oracle's stream
    return loss, (u, i, j), [str(w.message) for w in seen]


def _check_tables(eng, ref, tol, ms_tol=None):
    kh = eng.kh
    if ms_tol is None:                                               # the slots hold g^2: twice the relative error of g
        ms_tol = dict(rtol=1e-3 if tol is TOL else 2 * tol['rtol'], atol=1e-6)
    Uc, msU = (t.cpu().numpy() for t in eng.get('U'))
    np.testing.assert_allclose(Uc[:, :kh], ref['ure'], err_msg='ure', **tol)
    np.testing.assert_allclose(Uc[:, kh:], ref['uce'], err_msg='uce', **tol)
    np.testing.assert_allclose(msU[:, :kh], ref['ms_ure'], **ms_tol)
    np.testing.assert_allclose(eng.get('I')[0].cpu().numpy(), ref['ire'], err_msg='ire', **tol)
    np.testing.assert_allclose(eng.get('irb')[0].cpu().numpy(), ref['irb'], err_msg='irb', **tol)
    np.testing.assert_allclose(eng.cem.cpu().numpy(), ref['cem'], err_msg='cem', **tol)
    np.testing.assert_allclose(eng.icb.cpu().numpy(), ref['icb'], err_msg='icb', **tol)
    np.testing.assert_allclose(eng.mscem.cpu().numpy(), ref['ms_cem'], **ms_tol)


class _NoParities:
    """a plan buffer seen without K1's per-triplet parities: tkr_vbpr_run then scores the triplets per user occurrence (G2)"""

    def __init__(self, plan):
        self._plan = plan

    def __getattr__(self, name):
        if name == 'tpar':
            raise AttributeError(name)
        return getattr(self._plan, name)


@pytest.mark.parametrize('k,d,B,nb,mode,feat_kw,fused', [
    (300, 1500, 256, 3, 'l2', dict(), True),                         # dense rows: 1500 nonzeros, no column plan at any batch size
    (300, 1500, 256, 3, 'l1', dict(), True),
    (300, 1500, 256, 2, 'l2', dict(), False),                        # ... scored per user occurrence
    (300, 700, 2048, 2, 'l2', dict(density=0.1), True),              # batch above the column plan's 1024
    (302, 700, 1500, 2, 'l2', dict(density=0.1), True),              # kh = 151 (odd), batch 1500
    (280, 50000, 256, 2, 'l2', dict(per_row=30), True),              # the column plan's counters need more than 160 KB of LDS
])
def test_vbpr_generic_sparse_view_parity(k, d, B, nb, mode, feat_kw, fused, monkeypatch):
    """k // 2 > 128 where the column plan does not apply: the generic form of the sparse view against the oracle, one warning"""
    import tkr_hip
    n_users, n_items = 300, 90
    tr, tr_users = _toy(n_users, n_items, seed=k + d)
    feat = _feat(n_items, d, seed=d, **feat_kw)
    hp = dict(lu=2.5e-3, li=2.5e-3, lj=2.5e-4, lb=1e-3, le=1e-3, lr=0.02, mode=mode)
    eng, ref = _setup(n_users, n_items, k, d, feat, hp)
    assert eng.sparse is not None and not eng.wants_cols(B)
    if not fused:
        real = tkr_hip.vbpr_run
        monkeypatch.setattr(tkr_hip, 'vbpr_run', lambda state, plan, *a, **kw: real(state, _NoParities(plan), *a, **kw))
    loss, (u, i, j), msgs = _run(eng, tr, tr_users, n_users, nb, B)
    assert sum('generic form' in m for m in msgs) == 1
    ref_loss = [R.vbpr_step(ref, feat, u[b * B:(b + 1) * B], i[b * B:(b + 1) * B], j[b * B:(b + 1) * B], hp) for b in range(nb)]
    tol = TOL if B <= 1024 else TOL_BIG
    _check_tables(eng, ref, tol)
    np.testing.assert_allclose(loss, np.array(ref_loss), rtol=2e-4 if B <= 1024 else tol['rtol'])


# ---- batches above 65,536 ------------------------------------------------------------------------------------------------------
def _pair_sums(alpha, beta, rows=1024):
    """S_a = sum_b sigma(-(alpha_a + beta_b)), T_b = sum_a sigma(-(alpha_a + beta_b)) and the pair loss sum_ab log(1 + exp(-(alpha_a +
    beta_b))) of vbpr.py:61,64 in fp64 row blocks (the oracle's [B, B] matrix would be 19.6 GB at B = 70,000)"""
    dev = torch.device('cuda')
    a = torch.from_numpy(alpha.astype(np.float64)).to(dev)
    b = torch.from_numpy(beta.astype(np.float64)).to(dev)
    S = torch.empty_like(a)
    T = torch.zeros_like(b)
    pair = torch.zeros((), dtype=torch.float64, device=dev)
    for r0 in range(0, a.numel(), rows):
        x = a[r0:r0 + rows, None] + b[None, :]
        sg = torch.sigmoid(-x)
        S[r0:r0 + rows] = sg.sum(1)
        T += sg.sum(0)
        pair += torch.nn.functional.softplus(-x).sum()
    return S.cpu().numpy().astype(F32), T.cpu().numpy().astype(F32), float(pair)


def _vbpr_step_blocked(state, feat, ub, ib, jb, hp):
    """oracle/ref_np.vbpr_step with the pair sums and the pair loss from _pair_sums; every other line as the oracle states it"""
    ure, uce, ire, irb, cem, icb = (state[n] for n in ('ure', 'uce', 'ire', 'irb', 'cem', 'icb'))
    lu, li, lj, lb, le = (F32(hp[k]) for k in ('lu', 'li', 'lj', 'lb', 'le'))
    ub = np.asarray(ub, dtype=np.int64); ib = np.asarray(ib, dtype=np.int64); jb = np.asarray(jb, dtype=np.int64)
    ur, uc, ir, jr = ure[ub], uce[ub], ire[ib], ire[jb]
    bi, bj = irb[ib], irb[jb]
    ic, jc = feat[ib], feat[jb]
    ice = (ic @ cem).astype(F32)
    jce = (jc @ cem).astype(F32)
    x_ui = np.sum(ur * ir + uc * ice, axis=1, dtype=F32)
    x_uj = np.sum(ur * jr + uc * jce, axis=1, dtype=F32)
    dfeat = (ic - jc).astype(F32)
    alpha = (bi - bj + dfeat @ icb).astype(F32)
    beta = (x_ui - x_uj).astype(F32)
    sa, s, pair = _pair_sums(alpha, beta)
    sa, s = sa[:, None], s[:, None]
    if hp.get('mode', 'l2') == 'l2':
        loss = (F32(pair) + F32(0.5) * np.sum(cem * cem, dtype=F32) * le
                + F32(0.5) * np.sum((ur * ur + uc * uc) * lu + ir * ir * li + jr * jr * lj, dtype=F32)
                + F32(0.5) * (np.sum(bi * bi + bj * bj, dtype=F32) + np.sum(icb * icb, dtype=F32)) * lb)
        r_ur, r_uc, r_ir, r_jr = lu * ur, lu * uc, li * ir, lj * jr
        r_bi, r_bj, r_cem, r_icb = lb * bi, lb * bj, le * cem, lb * icb
    else:
        loss = (F32(pair) + np.sum(np.abs(cem), dtype=F32) * le
                + np.sum((np.abs(ur) + np.abs(uc)) * lu + np.abs(ir) * li + np.abs(jr) * lj, dtype=F32)
                + (np.sum(np.abs(bi) + np.abs(bj), dtype=F32) + np.sum(np.abs(icb), dtype=F32)) * lb)
        r_ur, r_uc, r_ir, r_jr = lu * np.sign(ur), lu * np.sign(uc), li * np.sign(ir), lj * np.sign(jr)
        r_bi, r_bj, r_cem, r_icb = lb * np.sign(bi), lb * np.sign(bj), le * np.sign(cem), lb * np.sign(icb)
    g_ur = (-s * (ir - jr) + r_ur).astype(F32)
    g_uc = (-s * (ice - jce) + r_uc).astype(F32)
    g_ir = (-s * ur + r_ir).astype(F32)
    g_jr = (s * ur + r_jr).astype(F32)
    g_bi = (-sa[:, 0] + r_bi).astype(F32)
    g_bj = (sa[:, 0] + r_bj).astype(F32)
    d_ice = (-s * uc).astype(F32)
    g_cem = (ic.T @ d_ice + jc.T @ (-d_ice) + r_cem).astype(F32)
    g_icb = (dfeat.T @ (-sa[:, 0]) + r_icb).astype(F32)
    lr = hp['lr']
    rows_u, sum_ur = R._segment_sum(ub, g_ur)
    _, sum_uc = R._segment_sum(ub, g_uc)
    items = np.concatenate([ib, jb])
    rows_i, sum_ir = R._segment_sum(items, np.concatenate([g_ir, g_jr]))
    _, sum_b = R._segment_sum(items, np.concatenate([g_bi, g_bj]))
    R._rmsprop_rows(ure, state['ms_ure'], rows_u, sum_ur, lr)
    R._rmsprop_rows(uce, state['ms_uce'], rows_u, sum_uc, lr)
    R._rmsprop_rows(ire, state['ms_ire'], rows_i, sum_ir, lr)
    R._rmsprop_rows(irb, state['ms_irb'], rows_i, sum_b, lr)
    for name, g in (('cem', g_cem), ('icb', g_icb)):
        ms = state['ms_' + name]
        ms[...] = (ms + (g * g - ms) * (F32(1) - R.RHO)).astype(F32)
        state[name][...] = (state[name] - F32(lr) * g / np.sqrt(ms + R.EPS)).astype(F32)
    return F32(loss)


def test_blocked_pair_sums_restate_the_oracle():
    """the restatement above equals ref_np.vbpr_step where the oracle can still form its [B, B] matrix"""
    n_users, n_items, k, d, B = 300, 90, 20, 40, 512
    tr, tr_users = _toy(n_users, n_items, seed=3)
    row_ptr, pos, srt = P.build_csr(tr, n_users)
    u, i, j = P.sample_triplets(tr_users, row_ptr, pos, srt, n_items, 5, 0, B)
    feat = _feat(n_items, d, seed=4, density=0.3)
    rng = np.random.Generator(np.random.PCG64(1))
    st = R.init_vbpr_state(n_users, n_items, k, d, rng)
    st['cem'] = (rng.standard_normal(st['cem'].shape) * 0.05).astype(F32)
    a, b = ({n: v.copy() for n, v in st.items()} for _ in range(2))
    hp = dict(lu=2.5e-3, li=2.5e-3, lj=2.5e-4, lb=1e-3, le=1e-3, lr=0.02, mode='l2')
    la = R.vbpr_step(a, feat, u, i, j, hp)
    lb = _vbpr_step_blocked(b, feat, u, i, j, hp)
    assert abs(float(la) - float(lb)) <= 1e-5 * abs(float(la))
    for n in a:                                                      # (fp64 pair sums here, fp32 ones there: 6e-6 apart at most)
        np.testing.assert_allclose(b[n], a[n], err_msg=n, **TOL)


@pytest.mark.parametrize('k,view', [(16, 'sparse'), (16, 'dense'), (300, 'sparse')])
def test_vbpr_batch_above_65536(k, view):
    """one batch of 70,000 on 600 users x 300 items (every item occurs ~470 times: heavy teams, occurrences past the four a record
    carries): the register form (k = 16, both views of feat) and the generic form (k = 300), one B^2 warning"""
    n_users, n_items, d, B = 600, 300, 40, 70000
    tr, tr_users = _toy(n_users, n_items, seed=11)
    feat = _feat(n_items, d, seed=12, density=0.3)
    # lr = the class default (1e-4): every update is at most lr * sqrt(10), so the fp32 order of the 70,000-term pair sums (vs fp64
    # here) stays below the table tolerance; the step still moves the tables by ~1e-4, five times the atol
    hp = dict(lu=2.5e-3, li=2.5e-3, lj=2.5e-4, lb=1e-3, le=1e-3, lr=1e-4, mode='l2')
    eng, ref = _setup(n_users, n_items, k, d, feat, hp, sparse=(view == 'sparse'))
    before = eng.get('I')[0].cpu().numpy()
    loss, (u, i, j), msgs = _run(eng, tr, tr_users, n_users, 1, B)
    assert sum('B^2' in m for m in msgs) == 1
    ref_loss = _vbpr_step_blocked(ref, feat, u, i, j, hp)
    # the slots hold 0.9 + 0.1 g^2 where g sums 70,000 triplets' terms of up to ~1e4 in another fp32 order: measured 1.6e-3 relative
    # (k = 16) and 7e-3 absolute on a slot of 1.2 (k = 300: g ~ 1 after cancellation, off by ~1e-5 of its terms); the tables meet TOL,
    # at lr = 1e-4 the normalised update barely depends on that error
    _check_tables(eng, ref, TOL, ms_tol=dict(rtol=5e-3, atol=2e-2))
    assert np.abs(eng.get('I')[0].cpu().numpy() - before).max() > 5e-5
    # the loss sums 4.9e9 pair terms of ~0.69: each of the B pair waves adds ~1,100 terms per lane in order (then a DPP tree), the
    # waves meet in 64 slots by atomics (~1,100 adds each) -- two levels of naive fp32 summation, <= 2 * 1,100 * 2^-24 = 1.3e-4
    # relative in the worst case, plus ~3e-7 per term from the hardware log (tkr_common.h pair_softplus_neg)
    np.testing.assert_allclose(loss, [ref_loss], rtol=5e-4)


# ---- through the class and run to run ----------------------------------------------------------------------------------------
def test_vbpr_class_wide_k_dense_features(tmp_path):
    """VBPR(k=300, d=2048) with dense content features (rows of 2048 nonzeros: no column plan) at batch_size=2048: one epoch through
    the generic form, one warning; the folded export is vbpr.py:124-126 of the engine's tables"""
    import synth
    from single import VBPR
    r = synth.make_ratings(200, 80, 20, seed=9, mu=3.0, sigma=0.5, min_r=5, max_r=40, om_per_user=3)
    data = str(tmp_path / 'data')
    synth.write_dataset(data, r)
    d, k = 2048, 300
    rng = np.random.Generator(np.random.PCG64(7))
    feats = np.abs(rng.standard_normal((100, d))).astype(np.float32)
    feats /= np.linalg.norm(feats, axis=1, keepdims=True)
    pickle.dump(feats, open(tmp_path / 'meta.pkl', 'wb'))
    m = VBPR(k=k, d=d, lambda_e=1e-3, lr=0.02)
    m.load_training_data(os.path.join(data, 'uid'), os.path.join(data, 'vid'), os.path.join(data, 'f0tr.txt'))
    m.load_content_data(str(tmp_path / 'meta.pkl'), os.path.join(data, 'vid'))
    with warnings.catch_warnings(record=True) as seen:
        warnings.simplefilter('always')
        m.train(epochs=1, batch_size=2048, epoch_sample_limit=2048 * 3, seed=3, verbose=False)
    assert sum('generic form' in str(w.message) for w in seen) == 1
    e = m._eng
    assert e.sparse is not None and not e.wants_cols(2048)
    kh = k // 2
    U = e.get('U')[0].cpu().numpy()
    st = dict(ure=U[:, :kh], uce=U[:, kh:], ire=e.get('I')[0].cpu().numpy(), irb=e.get('irb')[0].cpu().numpy(),
              cem=e.cem.cpu().numpy(), icb=e.icb.cpu().numpy())
    assert np.abs(st['cem'] - 2.0 / (d * k)).max() > 0                 # it trained
    fue, fie, fib = R.vbpr_fold(st, m.feat)
    np.testing.assert_allclose(m.fue, fue, rtol=3e-4, atol=2e-5)
    np.testing.assert_allclose(m.fie, fie, rtol=3e-4, atol=2e-5)
    np.testing.assert_allclose(m.fib, fib, rtol=3e-4, atol=2e-5)


def test_vbpr_generic_sparse_view_is_deterministic():
    """the same seed twice: bit-identical tables (fixed summation orders everywhere, no float atomics on parameters)"""
    n_users, n_items, k, d, B, nb = 300, 90, 300, 700, 2048, 2
    tr, tr_users = _toy(n_users, n_items, seed=21)
    feat = _feat(n_items, d, seed=22, density=0.1)
    hp = dict(lu=2.5e-3, li=2.5e-3, lj=2.5e-4, lb=1e-3, le=1e-3, lr=0.02, mode='l2')
    outs = []
    for _ in range(2):
        eng, _ref = _setup(n_users, n_items, k, d, feat, hp)
        _run(eng, tr, tr_users, n_users, nb, B)
        outs.append([eng.get('U')[0].cpu().numpy(), eng.get('I')[0].cpu().numpy(), eng.get('irb')[0].cpu().numpy(), eng.cem.cpu().numpy(),
                     eng.icb.cpu().numpy()])
    for a, b in zip(*outs):
        np.testing.assert_array_equal(a, b)
