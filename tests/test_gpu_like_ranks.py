"""K8 (tkr_like_ranks, csrc/like_ranks.hip), evaluate.py -M and the two-rank run of it, on the GPU.  rank_out is integer and
deterministic: every comparison with the oracle is exact."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _rank_oracle as O

import tkr_hip

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ALL = ['acc', 'auc', 'mrr', 'ndcg', 'map']


def _csr(rows):
    ptr = np.zeros(len(rows) + 1, np.int64)
    np.cumsum([len(x) for x in rows], out=ptr[1:])
    cols = np.concatenate([np.asarray(x, np.int32) for x in rows] + [np.zeros(0, np.int32)]).astype(np.int32)
    return ptr, cols


def _dev(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _like_ranks(U, V, likes, dev, bias=None, user_idx=None, rated=None):
    lptr, lcols = _csr(likes)
    mask, pitch = None, 0
    if rated is not None:
        rptr, rcols = _csr(rated)
        mask, pitch = tkr_hip.build_rated_mask(_dev(rptr, dev), _dev(rcols, dev), len(likes), V.shape[0])
    got = tkr_hip.like_ranks(_dev(U, dev), _dev(V, dev), _dev(lptr, dev), _dev(lcols, dev), bias=None if bias is None else _dev(bias, dev),
                             user_idx=None if user_idx is None else _dev(user_idx, dev), mask=mask, mask_pitch=pitch)
    return got.cpu().numpy(), lptr


@pytest.mark.parametrize('n_cols', [90, 700, 4099])
@pytest.mark.parametrize('k', [4, 8, 50, 128, 200, 256, 300])
def test_exact_arithmetic_with_ties_matches_oracle(k, n_cols):
    """factors m * 2^-6 with small integer m: every order of summation gives the same bits, and ties are frequent.  Rows holding 1,
    33, 64, 65 and 500 likes (all columns where the catalogue has fewer), some of them rated; a user block whose likes do not fit
    the kernel's LDS at once (20 rows of 500); with and without bias, mask and user_idx."""
    dev = torch.device('cuda')
    rng = np.random.Generator(np.random.PCG64(1000 * k + n_cols))
    n_rows = 300
    U_all = rng.integers(-3, 4, (n_rows + 9, k)).astype(np.float32) / 64
    V = rng.integers(-3, 4, (n_cols, k)).astype(np.float32) / 64
    V[n_cols // 2] = V[n_cols // 3]                                  # planted: two columns tie for EVERY user
    b = rng.integers(-2, 3, n_cols).astype(np.float32) / 4096
    b[n_cols // 2] = b[n_cols // 3]
    idx = rng.permutation(n_rows + 9)[:n_rows].astype(np.int32)
    counts = [1, 33, 64, 65, 500] + [500] * 20 + [int(x) for x in rng.integers(0, 13, n_rows - 25)]
    likes = [np.sort(rng.choice(n_cols, min(c, n_cols), replace=False)).astype(np.int32) for c in counts]
    likes[30] = np.union1d(likes[30], [n_cols // 3, n_cols // 2]).astype(np.int32)      # both ends of the planted tie are liked
    rated = [np.sort(rng.choice(n_cols, int(rng.integers(0, n_cols // 2)), replace=False)).astype(np.int32) for _ in range(n_rows)]
    rated[30] = np.setdiff1d(rated[30], [n_cols // 3, n_cols // 2]).astype(np.int32)
    for with_bias, with_mask, with_idx in ((False, False, False), (True, True, True), (True, False, False), (False, True, True)):
        U = U_all if with_idx else U_all[:n_rows]
        rows = idx if with_idx else np.arange(n_rows)
        s = (U_all[rows].astype(np.float64) @ V.astype(np.float64).T + (b.astype(np.float64) if with_bias else 0.0)).astype(np.float32)
        assert np.array_equal(s.astype(np.float64), U_all[rows].astype(np.float64) @ V.astype(np.float64).T + (b if with_bias else 0.0))
        got, lptr = _like_ranks(U, V, likes, dev, bias=b if with_bias else None, user_idx=idx if with_idx else None,
                                rated=rated if with_mask else None)
        want = np.concatenate([O.like_ranks_np(s[r], rated[r] if with_mask else (), likes[r]) for r in range(n_rows)])
        np.testing.assert_array_equal(got, want, err_msg=str((with_bias, with_mask, with_idx)))
        if with_mask:
            assert np.any(want < 0)
        e = int(lptr[30]) + int(np.searchsorted(likes[30], n_cols // 3))
        assert got[e] > got[int(lptr[30]) + int(np.searchsorted(likes[30], n_cols // 2))]           # ties: the higher column first


def test_consistent_with_topk_lists_on_generic_factors():
    """N(0, 0.01^2) factors rounded like '%f': a like at position p of K4's top-32 list has rank p; a like outside the list has
    rank >= 32, or -1 exactly when it is rated.  Under both arithmetic modes of K4 (same lists by contract)."""
    dev = torch.device('cuda')
    rng = np.random.Generator(np.random.PCG64(77))
    n_rows, n_cols, k, K = 3000, 10380, 128, 32
    U = np.round(rng.standard_normal((n_rows, k)) * 0.01, 6).astype(np.float32)
    V = np.round(rng.standard_normal((n_cols, k)) * 0.01, 6).astype(np.float32)
    # likes drawn where they matter: a few of the best columns of the row (approximate scores pick them), the rest anywhere
    approx = U @ V.T
    best = np.argsort(-approx, axis=1)[:, :40]
    likes, rated = [], []
    for r in range(n_rows):
        near = rng.choice(best[r], int(rng.integers(0, 6)), replace=False)
        far = rng.choice(n_cols, int(rng.integers(1, 12)), replace=False)
        likes.append(np.unique(np.r_[near, far]).astype(np.int32))
        rated.append(np.unique(np.r_[rng.choice(best[r], 5, replace=False), rng.choice(n_cols, 200, replace=False)]).astype(np.int32))
    lptr, lcols = _csr(likes)
    rptr, rcols = _csr(rated)
    Ud, Vd = _dev(U, dev), _dev(V, dev)
    mask, pitch = tkr_hip.build_rated_mask(_dev(rptr, dev), _dev(rcols, dev), n_rows, n_cols)
    ranks = tkr_hip.like_ranks(Ud, Vd, _dev(lptr, dev), _dev(lcols, dev), mask=mask, mask_pitch=pitch).cpu().numpy()
    line = np.repeat(np.arange(n_rows), np.diff(lptr))
    is_rated = np.zeros((n_rows, n_cols), dtype=bool)
    is_rated[np.repeat(np.arange(n_rows), np.diff(rptr)), rcols] = True
    like_rated = is_rated[line, lcols]
    assert like_rated.any() and not like_rated.all()
    try:
        for mode in ('refine', 'fp32'):
            tkr_hip.set_topk_math(mode)
            ids = tkr_hip.score_topk(Ud, Vd, K, mask=mask, mask_pitch=pitch).cpu().numpy()
            where = np.full((n_rows, n_cols), -1, dtype=np.int16)
            where[np.repeat(np.arange(n_rows), K), ids.reshape(-1)] = np.tile(np.arange(K), n_rows)
            p = where[line, lcols]
            listed = p >= 0
            print('%s: %d of %d likes are in a top-%d list, %d rated' % (mode, int(listed.sum()), len(p), K, int(like_rated.sum())))
            assert listed.sum() > 1000
            np.testing.assert_array_equal(ranks[listed], p[listed])
            np.testing.assert_array_equal(ranks[~listed] == -1, like_rated[~listed])
            assert np.all(ranks[~listed & ~like_rated] >= K)
            assert not np.any(listed & like_rated)
    finally:
        tkr_hip.set_topk_math(tkr_hip.TOPK_MATH_DEFAULT)


def _golden_runs(golden_dir):
    """(data, model, scenarios, step, total, expected reference stdout) of every committed CLI run of G4-G7"""
    runs = []
    for g, scs in (('g4', ['im', 'om']), ('g5', ['im', 'om']), ('g6', ['all'])):
        d = os.path.join(golden_dir, g)
        exp = json.load(open(os.path.join(d, 'expected.json')))
        runs.append((os.path.join(d, 'data'), os.path.join(d, 'model'), scs, 5, 30, exp['stdout']))
    d = os.path.join(golden_dir, 'g7')
    for run in json.load(open(os.path.join(d, 'expected.json')))['runs']:
        runs.append((os.path.join(d, 'data'), os.path.join(d, 'model'), ['sm'], run['step'], run['total'], run['stdout']))
    return runs


def test_cli_metrics_on_goldens(golden_dir, capsys):
    import evaluate as E
    from oracle import ref_np as R
    for data, model, scs, step, total, ref_stdout in _golden_runs(golden_dir):
        args = ['-d', data, '-m', model, '-s', str(step), '-t', str(total), '-sl'] + scs
        capsys.readouterr()
        plain = E.main(args)
        assert capsys.readouterr().out.strip().split('\n') == ref_stdout == plain          # without -M: unchanged
        got = E.main(args + ['-M'] + ALL)
        assert capsys.readouterr().out.strip().split('\n') == got
        assert got[:len(scs)] == ref_stdout
        want = O.metric_lines(data, model, 0, step, total, scs, ALL)
        assert got[len(scs):] == want, (data, step, total)
        for i, sc in enumerate(scs):                                  # S.acc is the plain line
            assert got[len(scs) + i * len(ALL)] == sc + '.acc' + ref_stdout[i][len(sc):]
        # a depth K4 reaches in ten passes: one rank pass
        deep = E.main(['-d', data, '-m', model, '-s', '50', '-t', '300', '-sl'] + scs + ['-M', 'acc'])
        assert deep[:len(scs)] == R.evaluate_cli(data, model, 0, 50, 300, scenarios=tuple(scs))
        assert [l.replace('.acc', '', 1) for l in deep[len(scs):]] == deep[:len(scs)]
    some = E.main(['-d', data, '-m', model, '-sl', 'sm', '-M', 'mrr', 'auc'])
    assert [l.split(',')[0] for l in some] == ['sm', 'sm.mrr', 'sm.auc']


def _run_cli_ranks(args, world, port, tmp_path):
    """evaluate.py under torch.distributed.run: `world` ranks on the one visible GPU (gloo) -> rank 0's stdout lines"""
    env = dict(os.environ, TKR_SINGLE_DEVICE='1', TKR_DIST_BACKEND='gloo', MASTER_ADDR='127.0.0.1', TKR_NO_CACHE='1')
    out = subprocess.run([sys.executable, '-m', 'torch.distributed.run', '--nnodes=1', '--nproc-per-node=%d' % world,
                          '--master-addr', '127.0.0.1', '--master-port', str(port),
                          os.path.join(ROOT, 'top-k-rec_amd', 'evaluate.py')] + args,
                         capture_output=True, text=True, timeout=280, env=env, cwd=str(tmp_path))
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-3000:]
    return [l for l in out.stdout.strip().split('\n') if ',' in l and not l.startswith('[')]


def test_two_ranks_on_one_gpu_agree_with_one_process(golden_dir, tmp_path):
    """the sums and counts of two shards, all-reduced: within 1e-6 of the single-process lines (printing rounds to 1e-6; the order
    of the fp64 sums differs by ~n * 2^-53)"""
    import evaluate as E
    for g, scs in (('g4', ['im', 'om']), ('g6', ['all'])):
        d = os.path.join(golden_dir, g)
        args = ['-d', os.path.join(d, 'data'), '-m', os.path.join(d, 'model'), '-sl'] + scs + ['-M'] + ALL
        one = E.main(args)
        two = _run_cli_ranks(args, 2, 29661, tmp_path)
        assert [l.split(',')[0] for l in two] == [l.split(',')[0] for l in one]
        for a, b in zip(one, two):
            va, vb = ([float(x) for x in l.split(',')[1:]] for l in (a, b))
            assert len(va) == len(vb) and all(abs(x - y) <= 1e-6 for x, y in zip(va, vb)), (a, b)


def test_bad_arguments_are_refused_before_any_device_access():
    lib = tkr_hip.lib()
    fn = lib.tkr_like_ranks
    fn.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_int32, C.c_void_p,
                   C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p]
    try:
        p = 4096                                                     # never dereferenced: every call below fails its checks
        good = dict(U=p, idx=None, n_rows=4, Vt=p, bias=None, n_cols=50, k=8, mask=None, pitch=0, lptr=p, lcols=p, out=p, ws=p,
                    ws_bytes=1 << 20, stream=None)
        bad = [dict(U=None), dict(Vt=None), dict(lptr=None), dict(lcols=None), dict(out=None), dict(ws=None), dict(n_rows=0),
               dict(n_cols=0), dict(n_cols=1 << 27), dict(k=0), dict(mask=p, pitch=3), dict(ws_bytes=0), dict(ws_bytes=16)]
        for change in bad:
            a = dict(good, **change)
            assert fn(*a.values()) == -1, change                     # TKR_E_INVAL
    finally:
        fn.argtypes = None
    need = lib.tkr_like_ranks_workspace_bytes
    assert need(C.c_int32(10), C.c_int32(50), C.c_int32(8), C.c_int64(1000)) >= 1000 * 20
    assert need(C.c_int32(0), C.c_int32(50), C.c_int32(8), C.c_int64(1000)) == 0
