"""K9 (tkr_bpr_foldin, csrc/foldin.hip), foldin.py, BPR.fold_in and recommend.py on the GPU, against tests/_foldin_oracle.py.
The draw is integer and compared exactly; the vectors at the project's step tolerance (rtol 2e-4, atol 1e-5, as smoke())."""
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _foldin_oracle as O

from oracle import ref_np as R

import tkr_hip

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RTOL, ATOL = 2e-4, 1e-5


def _dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to('cuda')


def _fold(V, b, ptr, cols, **kw):
    U0 = kw.pop('U0', None)
    out = tkr_hip.fold_in(_dev(V), _dev(b), _dev(ptr), _dev(cols), U0=_dev(U0), **kw)
    out = out if isinstance(out, tuple) else (out,)
    return tuple(t.cpu().numpy() for t in out)


def _histories(rng, n_items, degrees):
    return [np.sort(rng.choice(n_items, d, replace=False)).astype(np.int32) for d in degrees]


def test_draw_equals_oracle_exactly():
    """degrees 1, 2, 37 and 1,000, a user who rated all but one item, first_row != 0 (small, and above 2^32 / steps / triplets so that
    the second counter word moves), and a call split in two blocks = the call in one"""
    rng = np.random.Generator(np.random.PCG64(41))
    n_items, k, T, Pn = 1200, 16, 5, 16
    degrees = [1, 2, 37, 1000, n_items - 1, 37, 0, n_items, 5, 300] + [int(x) for x in rng.integers(1, 80, 54)]
    hist = _histories(rng, n_items, degrees)
    ptr, cols = O.csr(hist)
    V = (rng.standard_normal((n_items, k)) * 0.1).astype(np.float32)
    hp = dict(lu=2.5e-3, lr=0.05, steps=T, triplets=Pn)
    for seed, first in ((7, 0), (7, 12345), ((1 << 63) + 99, (1 << 40) + 3)):
        U, trip = _fold(V, None, ptr, cols, seed=seed, first_row=first, want_triplets=True, **hp)
        want = O.draw(ptr, cols, n_items, seed, T, Pn, first_row=first)
        np.testing.assert_array_equal(trip, want, err_msg=str((seed, first)))
        assert np.all(trip[6] == -1) and np.all(trip[7] == -1) and np.all(trip[4, :, :, 1] == np.setdiff1d(np.arange(n_items), hist[4])[0])
        cut = 23
        Ua, ta = _fold(V, None, ptr[:cut + 1], cols[:ptr[cut]], seed=seed, first_row=first, want_triplets=True, **hp)
        Ub, tb = _fold(V, None, ptr[cut:] - ptr[cut], cols[ptr[cut]:], seed=seed, first_row=first + cut, want_triplets=True, **hp)
        np.testing.assert_array_equal(np.concatenate([ta, tb]), trip)
        np.testing.assert_array_equal(np.concatenate([Ua, Ub]), U)             # bitwise: a user does not see who shares its call
    for Pn in (1, 3, 64):
        _, trip = _fold(V, None, ptr, cols, seed=3, lu=2.5e-3, lr=0.05, steps=2, triplets=Pn, want_triplets=True)
        np.testing.assert_array_equal(trip, O.draw(ptr, cols, n_items, 3, 2, Pn))


@pytest.mark.parametrize('Pn', [1, 16, 64])
@pytest.mark.parametrize('k', [4, 50, 128, 200, 512, 600])
def test_short_run_matches_oracle(k, Pn):
    """at most 16 updates of a row (the depth of the existing step tests): T = 16, 8, 4 for P = 1, 16, 64; l2 and l1, with and without
    item biases, from zero vectors and from given ones.  k = 4 .. 512: the register forms (k = 128, 512 the vector rows), 600: LDS."""
    rng = np.random.Generator(np.random.PCG64(100 * k + Pn))
    n_items, T = 500, {1: 16, 16: 8, 64: 4}[Pn]
    hist = _histories(rng, n_items, [1, 2, 37, 0, n_items, 499] + [int(x) for x in rng.integers(1, 60, 34)])
    ptr, cols = O.csr(hist)
    m = len(hist)
    V = (rng.standard_normal((n_items, k)) * 0.1).astype(np.float32)
    bias = (rng.standard_normal(n_items) * 0.1).astype(np.float32)
    start = (rng.standard_normal((m, k)) * 0.1).astype(np.float32)
    trip = O.draw(ptr, cols, n_items, 11, T, Pn)
    import warnings
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')                               # (k = 600: the one warning of the generic form)
        for mode in ('l2', 'l1'):
            for b in (None, bias):
                for U0 in (None, start):
                    U, loss, got_trip = _fold(V, b, ptr, cols, lu=2.5e-3, lr=0.05, mode=mode, steps=T, triplets=Pn, seed=11, U0=U0, want_loss=True,
                                              want_triplets=True)
                    np.testing.assert_array_equal(got_trip, trip)
                    wantU, want_loss = O.fold_in(V, b, ptr, cols, trip, 2.5e-3, 0.05, mode, U0=U0)
                    what = str((k, Pn, mode, b is not None, U0 is not None))
                    print(what, 'max |U - oracle| = %.3g, max |loss - oracle| = %.3g' % (np.abs(U - wantU).max(), np.abs(loss - want_loss).max()))
                    np.testing.assert_allclose(U, wantU, rtol=RTOL, atol=ATOL, err_msg=what)
                    np.testing.assert_allclose(loss, want_loss, rtol=RTOL, atol=ATOL, err_msg=what)
                    for x in (3, 4):                                  # empty / full-catalogue history: the start vector, untouched
                        np.testing.assert_array_equal(U[x], np.zeros(k, np.float32) if U0 is None else U0[x])
                        assert loss[x] == 0
                    assert np.abs(U[0]).max() > 1e-3


@pytest.mark.parametrize('k', [50, 128])
def test_default_depth_within_measured_tolerance(k):
    """T = 50, P = 16.  The tolerance is measured: d = the largest elementwise distance between the oracle in fp32 and in fp64 on the
    same triplets; the kernel must lie within max(project tolerance, 4 d) of the fp64 result (4: a wave sums in another order
    than NumPy).  Measured on MI355X: see DESIGN.md section 4, K9."""
    rng = np.random.Generator(np.random.PCG64(k))
    n_items, m, T, Pn = 2000, 64, 50, 16
    hist = _histories(rng, n_items, [int(x) for x in rng.integers(5, 70, m)])
    ptr, cols = O.csr(hist)
    V = (rng.standard_normal((n_items, k)) * 0.1).astype(np.float32)
    bias = (rng.standard_normal(n_items) * 0.1).astype(np.float32)
    U, trip = _fold(V, bias, ptr, cols, lu=2.5e-3, lr=0.05, steps=T, triplets=Pn, seed=5, want_triplets=True)
    np.testing.assert_array_equal(trip, O.draw(ptr, cols, n_items, 5, T, Pn))
    U32, _ = O.fold_in(V, bias, ptr, cols, trip, 2.5e-3, 0.05)
    U64, _ = O.fold_in_direct(V, bias, ptr, cols, trip, 2.5e-3, 0.05, dtype=np.float64)
    d = float(np.abs(U32.astype(np.float64) - U64).max())
    dist = np.abs(U.astype(np.float64) - U64)
    bound = np.maximum(ATOL + RTOL * np.abs(U64), 4 * d)
    print('k = %d: d(fp32 oracle, fp64 oracle) = %.3g, kernel to fp64 = %.3g, max |U| = %.3g, tightest bound used = %.3g'
          % (k, d, float(dist.max()), float(np.abs(U64).max()), float(bound.min())))
    assert np.all(dist <= bound), float((dist - bound).max())


@pytest.mark.parametrize('k', [128, 600])
def test_split_by_first_row_and_two_runs_are_bitwise_equal(k):
    """the vector rows (k = 128: workgroups of four waves, the last one partly filled) and the LDS form (k = 600: one wave a
    workgroup): a call split at row 23 equals the call in one, and a second run the first, bitwise -- a wave carries nothing from
    one row to the next and a user does not see who shares its call"""
    rng = np.random.Generator(np.random.PCG64(k))
    n_items, cut = 1200, 23
    hist = _histories(rng, n_items, [int(x) for x in rng.integers(1, 81, 60)])
    ptr, cols = O.csr(hist)
    V = (rng.standard_normal((n_items, k)) * 0.1).astype(np.float32)
    bias = (rng.standard_normal(n_items) * 0.1).astype(np.float32)
    kw = dict(lu=2.5e-3, lr=0.05, steps=5, triplets=16, seed=9, want_loss=True, want_triplets=True)
    import warnings
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')                               # (k = 600: the one warning of the generic form)
        whole = _fold(V, bias, ptr, cols, first_row=12345, **kw)
        again = _fold(V, bias, ptr, cols, first_row=12345, **kw)
        head = _fold(V, bias, ptr[:cut + 1], cols[:ptr[cut]], first_row=12345, **kw)
        tail = _fold(V, bias, ptr[cut:] - ptr[cut], cols[ptr[cut]:], first_row=12345 + cut, **kw)
    assert len(whole) == 3 and np.abs(whole[0]).max() > 1e-3 and whole[1].all() and (whole[2] >= 0).all()
    for a, c, h, t in zip(whole, again, head, tail):
        np.testing.assert_array_equal(a, c)
        np.testing.assert_array_equal(a, np.concatenate([h, t]))


EDGE_CHILD = r'''
import sys
sys.path[:0] = [%r, %r]
import numpy as np, torch, tkr_hip
n_items, k = 70, %d
V = torch.randn((n_items, k), device='cuda')
ptr = torch.tensor([0, 0, n_items, n_items, 2 * n_items], dtype=torch.int64, device='cuda')
cols = torch.arange(n_items, dtype=torch.int32, device='cuda').repeat(2)
U0 = torch.randn((4, k), device='cuda')
for start in (None, U0):
    U, loss, trip = tkr_hip.fold_in(V, None, ptr, cols, lu=2.5e-3, lr=0.05, steps=50, triplets=16, seed=1, U0=start, want_loss=True, want_triplets=True)
    torch.cuda.synchronize()
    assert torch.equal(U, torch.zeros_like(U) if start is None else U0) and not loss.any() and bool((trip == -1).all())
U = tkr_hip.fold_in(V, None, torch.zeros(4, dtype=torch.int64, device='cuda'), torch.zeros(0, dtype=torch.int32, device='cuda'), lu=0.1, lr=0.1, steps=3, triplets=64, seed=1)
assert U.shape == (3, k) and not U.any()
print('edge ok')
'''


@pytest.mark.parametrize('k', [16, 600])
def test_edge_rows_keep_start_vector_and_never_hang(k):
    """histories that are empty or cover the whole catalogue (no triplet exists: decided before any draw, so the cyclic fallback never
    runs on them), in a child process under its own time limit"""
    out = subprocess.run([sys.executable, '-W', 'ignore', '-c', EDGE_CHILD % (ROOT, os.path.join(ROOT, 'top-k-rec_amd'), k)], capture_output=True, text=True,
                         timeout=120)
    assert out.returncode == 0 and 'edge ok' in out.stdout, out.stdout[-2000:] + out.stderr[-2000:]


def test_wrapper_refuses_bad_arguments():
    V = torch.zeros((10, 4), device='cuda')
    ptr = torch.tensor([0, 1], dtype=torch.int64, device='cuda')
    for cols, Pn in (([3], 0), ([3], 65), ([10], 4), ([-1], 4)):
        with pytest.raises((ValueError, AssertionError)):
            tkr_hip.fold_in(V, None, ptr, torch.tensor(cols, dtype=torch.int32, device='cuda'), lu=0.1, lr=0.1, steps=1, triplets=Pn, seed=0)
    with pytest.raises(AssertionError):                               # a row pointer that decreases: refused before any launch
        tkr_hip.fold_in(V, None, torch.tensor([0, 2, 1, 3], dtype=torch.int64, device='cuda'), torch.tensor([1, 2, 3], dtype=torch.int32, device='cuda'),
                        lu=0.1, lr=0.1, steps=1, triplets=4, seed=0)


def _g4(golden_dir):
    d = os.path.join(golden_dir, 'g4')
    return os.path.join(d, 'data'), os.path.join(d, 'model')


def _parse_lines(path):
    out = []
    for ln in open(path).read().strip().split('\n'):
        f = ln.split(',')
        out.append((f[0], [t.split(':')[0] for t in f[1:]], [float(t.split(':')[1]) for t in f[1:]]))
    return out


def _expected_lists(umat, vmat, bias, rated_cols, total):
    s = R.mfma_chain_scores(umat, vmat, bias)
    return s, [R.filtered_topk(s[x], rated_cols[x], total, canonical=True) for x in range(len(umat))]


def test_recommend_cli_on_golden_g4(golden_dir, tmp_path):
    """every user of G4: the ids of each line are ref_np.filtered_topk(canonical) on fue . fie^T with every item of the user's history
    line masked, the scores those of the product within what '%f' prints"""
    import recommend
    data, model = _g4(golden_dir)
    uids, vids = R.read_id_list(os.path.join(data, 'uid')), R.read_id_list(os.path.join(data, 'vid'))
    ivt = {i: v for v, i in vids.items()}
    rated = R.read_history(os.path.join(data, 'f0tr.txt'))
    umat = R.read_embed_text(os.path.join(model, 'final-U.dat'), uids)
    vmat = R.read_embed_text(os.path.join(model, 'final-V.dat'), vids)
    users = list(uids)
    rated_cols = [{vids[v] for v in rated.get(u, ()) if v in vids} for u in users]
    s, want = _expected_lists(umat[[uids[u] for u in users]], vmat, None, rated_cols, 30)
    out = tmp_path / 'rec.txt'
    lines = recommend.main(['-d', data, '-m', model, '-f', '0', '-t', '30', '-o', str(out)])
    got = _parse_lines(str(out))
    assert len(got) == len(users) == len(lines) and open(str(out)).read() == '\n'.join(lines) + '\n'
    masked = 0
    for x, (u, ids, scores) in enumerate(got):
        assert u == users[x] and ids == [ivt[c] for c in want[x]], u
        assert not set(ids) & rated.get(u, set())
        masked += len(rated_cols[x])
        np.testing.assert_allclose(scores, s[x][want[x]], rtol=1e-6, atol=1.1e-6)
    assert masked > 0
    # a user list: those users, in its order, a repeated user twice; -t above one K4 launch
    some = tmp_path / 'some'
    some.write_text('%s\n%s\n%s\n' % (users[5], users[2], users[5]))
    recommend.main(['-d', data, '-m', model, '-t', '40', '-o', str(out), '-u', str(some)])
    got = _parse_lines(str(out))
    _, want40 = _expected_lists(umat[[uids[u] for u in users]], vmat, None, rated_cols, 40)
    assert [g[0] for g in got] == [users[5], users[2], users[5]]
    for g, x in zip(got, (5, 2, 5)):
        assert g[1] == [ivt[c] for c in want40[x]]


def test_recommend_cli_folds_in_new_users(golden_dir, tmp_path):
    """the last three users of G4's uid file are taken out of a copy of it and presented as new: their lines are the canonical lists of
    the vectors K9 folds in for them, and those vectors agree with the oracle's -- rounded to exact small-integer factors (as smoke()
    does for K4) kernel and oracle give identical lists"""
    import foldin
    import recommend
    data, model = _g4(golden_dir)
    work = tmp_path / 'data'
    shutil.copytree(data, str(work))
    tokens = open(os.path.join(data, 'uid')).read().split()
    new = tokens[-3:]
    (work / 'uid').write_text('\n'.join(tokens[:-3]) + '\n')
    (tmp_path / 'new_uid').write_text('\n'.join(new) + '\n')
    vids = R.read_id_list(os.path.join(data, 'vid'))
    ivt = {i: v for v, i in vids.items()}
    vmat = R.read_embed_text(os.path.join(model, 'final-V.dat'), vids)
    rated = R.read_history(os.path.join(data, 'f0tr.txt'))
    pairs = R.read_positive_pairs(os.path.join(data, 'f0tr.txt'), {u: i for i, u in enumerate(new)}, vids)
    hist = [sorted({vids[i] for u, i in pairs if u == tok}) for tok in new]
    assert all(len(h) > 0 for h in hist)
    hp = dict(lu=2.5e-3, lr=0.05, steps=50, triplets=16, seed=3)
    out = tmp_path / 'rec.txt'
    recommend.main(['-d', str(work), '-m', model, '-t', '10', '-o', str(out), '--new-uid', str(tmp_path / 'new_uid'), '--new-history',
                    os.path.join(data, 'f0tr.txt'), '--seed', '3'])
    got = _parse_lines(str(out))
    assert [g[0] for g in got] == tokens[:-3] + new
    U = foldin.fold_in(vmat, None, hist, **hp)                        # K9 is bitwise repeatable: the vectors the CLI ranked
    rated_cols = [{vids[v] for v in rated[u] if v in vids} for u in new]
    s, want = _expected_lists(U, vmat, None, rated_cols, 10)
    for x, g in enumerate(got[-3:]):
        assert g[1] == [ivt[c] for c in want[x]] and not set(g[1]) & rated[new[x]]
        np.testing.assert_allclose(g[2], s[x][want[x]], rtol=1e-6, atol=1.1e-6)
    ptr, cols = O.csr(hist)
    Uo, _ = O.fold_in(vmat, None, ptr, cols, O.draw(ptr, cols, len(vmat), 3, 50, 16), 2.5e-3, 0.05)
    print('max |U - oracle| = %.3g at max |U| = %.3g' % (np.abs(U - Uo).max(), np.abs(Uo).max()))
    qV = np.round(vmat * 512).astype(np.float32) / 64
    qU, qUo = (np.round(a * 64).astype(np.float32) / 64 for a in (U, Uo))
    dev = torch.device('cuda')
    rptr, rcols = O.csr([sorted(c) for c in rated_cols])
    mask, pitch = tkr_hip.build_rated_mask(_dev(rptr), _dev(rcols), 3, len(vmat))
    ids = tkr_hip.score_topk(_dev(qU), _dev(qV), 10, mask=mask, mask_pitch=pitch).cpu().numpy()
    so = np.dot(qUo, qV.T)
    for x in range(3):
        assert ids[x].tolist() == R.filtered_topk(so[x], rated_cols[x], 10, canonical=True), x


def test_bpr_fold_in_on_vbpr_shaped_factors(tmp_path):
    """a VBPR model's exported factors: fie = [ire | feat . cem], fib = irb + feat . icb (vbpr.py:124-126).  VBPR inherits
    BPR.fold_in unchanged; the vectors are the oracle's on the same histories.  start='model' refreshes users of the model."""
    from single.vbpr import VBPR
    rng = np.random.Generator(np.random.PCG64(8))
    n_items, k, d = 90, 12, 30
    feat = rng.random((n_items, d)).astype(np.float32)
    cem = (rng.standard_normal((d, k // 2)) * 0.05).astype(np.float32)
    model = VBPR(k=k, d=d, lr=0.05)
    model.uids = {'a%d' % q: q for q in range(4)}
    model.iids = {'i%d' % q: q for q in range(n_items)}
    model.n_users, model.n_items = 4, n_items
    model.fue = (rng.standard_normal((4, k)) * 0.1).astype(np.float32)
    model.fie = np.concatenate([(rng.standard_normal((n_items, k // 2)) * 0.1).astype(np.float32), feat @ cem], axis=1)
    model.fib = (rng.standard_normal(n_items) * 0.1 + feat @ (rng.standard_normal(d) * 0.01)).astype(np.float32).reshape(-1, 1)
    hist = _histories(rng, n_items, [7, 1, 20])
    new = ['n0', 'n1', 'n2']
    (tmp_path / 'uid').write_text('\n'.join(new) + '\n')
    with open(str(tmp_path / 'tr.txt'), 'w') as fh:
        for tok, h in zip(new, hist):                                 # like 0 entries and unknown items are not positives
            fh.write(tok + ',' + ','.join('i%d:1' % c for c in h[::-1]) + ',i%d:0,zzz:1\n' % int(np.setdiff1d(np.arange(n_items), h)[0]))
    uids, U = model.fold_in(str(tmp_path / 'uid'), str(tmp_path / 'tr.txt'), steps=8, triplets=16, seed=4)
    assert uids == {'n0': 0, 'n1': 1, 'n2': 2} and U.shape == (3, k) and U.dtype == np.float32
    ptr, cols = O.csr(hist)
    trip = O.draw(ptr, cols, n_items, 4, 8, 16)
    want, _ = O.fold_in(model.fie, model.fib, ptr, cols, trip, model.lu, model.lr, model.mode)
    np.testing.assert_allclose(U, want, rtol=RTOL, atol=ATOL)
    with pytest.raises(ValueError):                                   # known users are not new
        (tmp_path / 'old').write_text('a1\n')
        model.fold_in(str(tmp_path / 'old'), str(tmp_path / 'tr.txt'))
    (tmp_path / 'old').write_text('a2\na0\n')
    with open(str(tmp_path / 'tr2.txt'), 'w') as fh:
        fh.write('a0,' + ','.join('i%d:1' % c for c in hist[0]) + '\na2,' + ','.join('i%d:1' % c for c in hist[2]) + '\n')
    uids, U = model.fold_in(str(tmp_path / 'old'), str(tmp_path / 'tr2.txt'), steps=8, triplets=16, seed=4, start='model', lr=0.01, lambda_u=0.01)
    p2, c2 = O.csr([hist[2], hist[0]])
    want, _ = O.fold_in(model.fie, model.fib, p2, c2, O.draw(p2, c2, n_items, 4, 8, 16), 0.01, 0.01, U0=model.fue[[2, 0]])
    assert uids == {'a2': 0, 'a0': 1}
    np.testing.assert_allclose(U, want, rtol=RTOL, atol=ATOL)
