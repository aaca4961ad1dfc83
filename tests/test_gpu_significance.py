"""K18 on the GPU: the line table bit for bit against the per-line loops of tests/_significance_oracle.py, what it refuses, the resample
sums against long-double sums over the oracle's draw, and evaluate.py --bootstrap / --compare against the oracle pipeline."""
import os
import shutil
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _rank_oracle as RO
import _significance_oracle as O

import rankmetrics
import significance
import tkr_hip

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'


def planted(step, total, n_cols, n_lines=400, seed=3):
    """ranks no K8 produced: every shape of line the kernel distinguishes.  P is cut to the line's unrated columns where n_cols is small"""
    rng = np.random.Generator(np.random.PCG64(seed))
    interval = total // step
    edges = sorted({x for b in range(interval) for x in (step * (b + 1) - 1, step * (b + 1))})
    ranks, like_ptr, rated_ptr = [], [0], [0]
    for r in range(n_lines):
        rated = int(rng.integers(0, n_cols // 2)) if r % 3 else 0
        tail = [-1] * int(rng.integers(0, 3))                          # rated likes beside the ranked ones
        kind = r % 20
        if kind < 7:                                                   # P = 0, 1, 2, 63, 64, 65, 500: below, at and above one wave's lanes
            P = min((0, 1, 2, 63, 64, 65, 500)[kind], n_cols - rated)
            line = rng.choice(n_cols - rated, P, replace=False).tolist()
            tail = tail or ([-1] if P == 0 else [])
        elif kind == 7:                                                # every like is rated
            line, tail = [], [-1, -1, -1]
        elif kind == 8:                                                # N = 0: every unrated column is a like
            rated = n_cols - 5
            line = [0, 1, 2, 3, 4]
        elif kind == 9:                                                # ranks on both sides of every cut-off
            line = [x for x in edges if x < n_cols - rated]
        elif kind == 10:                                               # the best possible ranks
            line = list(range(min(17, n_cols - rated)))
        elif kind == 11:                                               # the worst possible ranks
            cap = n_cols - rated
            line = list(range(max(cap - 17, 0), cap))
        elif kind == 12:                                               # a line without a like at all
            line, tail = [], []
        else:
            line = rng.choice(n_cols - rated, int(rng.integers(0, min(n_cols - rated, 40) + 1)), replace=False).tolist()
        line = line + tail
        rng.shuffle(line)
        ranks += line
        like_ptr.append(len(ranks))
        rated_ptr.append(rated_ptr[-1] + rated)
    return np.array(ranks, dtype=np.int32), np.array(like_ptr, dtype=np.int64), np.array(rated_ptr, dtype=np.int64)


def device_table(ranks, like_ptr, rated_ptr, n_cols, step, total):
    args = [torch.from_numpy(np.ascontiguousarray(a)).to(DEV) for a in (ranks.astype(np.int32), like_ptr, rated_ptr)]
    return significance.line_table(*args, n_cols, step, total)


def assert_same_bits(got, want):
    assert got.dtype == want.dtype == np.float64 and got.shape == want.shape
    assert np.array_equal(got.view(np.uint64), want.view(np.uint64)), np.argwhere(got.view(np.uint64) != want.view(np.uint64))[:5]


@pytest.mark.parametrize('step,total,n_cols', [(5, 30, 90), (7, 30, 4099), (1, 1, 90), (32, 1024, 4099), (5, 3, 90)])
def test_table_is_bit_exact_on_planted_ranks(step, total, n_cols):
    ranks, like_ptr, rated_ptr = planted(step, total, n_cols)
    want = O.line_table(ranks, like_ptr, rated_ptr, n_cols, step, total)
    got = device_table(ranks, like_ptr, rated_ptr, n_cols, step, total)
    assert got.shape == (400, 3 * (total // step) + 5)
    assert_same_bits(got.cpu().numpy(), want)
    assert_same_bits(device_table(ranks, like_ptr, rated_ptr, n_cols, step, total).cpu().numpy(), got.cpu().numpy())


@pytest.mark.parametrize('step,total,n_cols', [(1, 100, 300), (5, 30, 300000), (5, 30, 500000), (5, 30, tkr_hip.LINE_MAX_COLS)])
def test_table_at_every_launch_shape(step, total, n_cols):
    """more cut-offs than lanes (lane b takes b, b + 64, ...), and bitmaps of which four, two and one fit a workgroup"""
    ranks, like_ptr, rated_ptr = planted(step, total, n_cols, n_lines=23, seed=8)
    ranks[like_ptr[1]] = n_cols - 1 - (rated_ptr[2] - rated_ptr[1])  # the last bit of the bitmap that may be set (line 1: P = 1)
    want = O.line_table(ranks, like_ptr, rated_ptr, n_cols, step, total)
    assert_same_bits(device_table(ranks, like_ptr, rated_ptr, n_cols, step, total).cpu().numpy(), want)
    with pytest.raises(tkr_hip.TkrError, match='supported'):
        device_table(ranks, like_ptr, rated_ptr, tkr_hip.LINE_MAX_COLS + 1, step, total)
    with pytest.raises(tkr_hip.TkrError, match='supported'):
        device_table(ranks, like_ptr, rated_ptr, n_cols, 5, 1025)


def _g4(golden_dir, scenario):
    import evaluate as E
    import textio
    d = os.path.join(golden_dir, 'g4')
    data, model = os.path.join(d, 'data'), os.path.join(d, 'model')
    uids, vids = E.read_ids(os.path.join(data, 'uid')), E.read_ids(os.path.join(data, 'vid'))
    umat = torch.from_numpy(E.read_matrix(os.path.join(model, 'final-U.dat'), uids)).to(DEV)
    vmat = E.read_matrix(os.path.join(model, 'final-V.dat'), vids)
    sc = E.load_scenario(data, 0, scenario, uids, textio.IdMap(uids))
    return E, sc, E.like_ranks_loaded(umat, vmat, None, vids, sc, torch.device(DEV))


def test_table_from_k8_ranks_on_g4(golden_dir):
    for scenario in ('im', 'om'):
        E, sc, ranks = _g4(golden_dir, scenario)
        lptr, rptr = (torch.from_numpy(a).to(DEV) for a in (sc.like_ptr, sc.rated_ptr))
        X = significance.line_table(ranks, lptr, rptr, len(sc.teids), 5, 30).cpu().numpy()
        host = ranks.cpu().numpy()
        assert_same_bits(X, O.line_table(host, sc.like_ptr, sc.rated_ptr, len(sc.teids), 5, 30))
        sums = rankmetrics.rank_sums(host, sc.like_ptr, sc.rated_ptr, len(sc.teids), 5, 30)
        col, bound = X.sum(0), len(X) * 2.0 ** -52 * np.abs(X).sum(0)
        np.testing.assert_array_equal(col[:6], sums['acc'][0])
        assert col[6] == sums['acc'][1] and col[8] == sums['auc'][1] and col[10] == sums['mrr'][1] == sums['ndcg'][1] == sums['map'][1]
        assert abs(col[7] - sums['auc'][0]) <= bound[7] and abs(col[9] - sums['mrr'][0]) <= bound[9]
        assert np.all(np.abs(col[11:17] - sums['ndcg'][0]) <= bound[11:17]) and np.all(np.abs(col[17:] - sums['map'][0]) <= bound[17:])


def test_refused_inputs_raise_and_the_next_call_works():
    good = dict(ranks=np.array([0, 3, -1, 2, 40, 70], dtype=np.int32), like_ptr=np.array([0, 3, 6], dtype=np.int64),
                rated_ptr=np.array([0, 2, 10], dtype=np.int64), n_cols=90, step=5, total=30)
    want = O.line_table(**good)
    cases = [(dict(ranks=[0, 3, -2, 2, 40, 70]), 'below -1'), (dict(ranks=[0, 3, -1, 2, 40, -2 ** 31]), 'below -1'),
             (dict(ranks=[0, 88, -1, 2, 40, 70]), 'unrated'),           # line 0 has 88 unrated columns: ranks 0 .. 87
             (dict(ranks=[0, 3, -1, 2, 40, 82]), 'unrated'), (dict(ranks=[0, 3, -1, 2, 40, 2 ** 31 - 1]), 'unrated'),
             (dict(ranks=[3, 3, -1, 2, 40, 70]), 'twice'),
             (dict(ranks=[0, 3, -1, 70, 40, 70]), 'twice'),             # both beyond `total`: no cut-off ever looks at them
             (dict(like_ptr=[1, 3, 6]), 'ascend'), (dict(like_ptr=[0, 4, 3]), 'ascend'), (dict(like_ptr=[0, 3, 7]), 'ascend'),
             (dict(like_ptr=[0, -3, 6]), 'ascend'), (dict(like_ptr=[0, 2 ** 40, 6]), 'ascend'),
             (dict(rated_ptr=[0, 5, 3]), 'ascend'), (dict(rated_ptr=[2, 4, 12]), 'ascend'), (dict(rated_ptr=[0, 91, 100]), 'ascend')]
    for change, word in cases:
        a = dict(good, **{k: np.array(v, dtype=good[k].dtype) for k, v in change.items()})
        with pytest.raises(O.Refused):
            O.line_table(**a)
        with pytest.raises(tkr_hip.TkrError, match=word):
            device_table(**a)
        assert_same_bits(device_table(**good).cpu().numpy(), want)
    # the status word names the first line that was refused
    with pytest.raises(tkr_hip.TkrError, match='line 1 '):
        device_table(**dict(good, ranks=np.array([0, 3, -1, 2, 2, 70], dtype=np.int32)))


def boot_table(n, C, seed):
    """integer-valued columns in front (sums exact in float64), then floats of both signs over fifteen orders of magnitude"""
    rng = np.random.Generator(np.random.PCG64(seed))
    n_int = 7 if C >= 14 else (C + 1) // 2
    X = np.empty((n, C), dtype=np.float64)
    X[:, :n_int] = rng.integers(0, 1 << 20, (n, n_int))
    X[:, n_int:] = rng.choice([-1.0, 1.0], (n, C - n_int)) * 10.0 ** rng.uniform(-9, 6, (n, C - n_int))
    return X, n_int


@pytest.mark.parametrize('n,C,R', [(1, 1, 1), (2, 5, 3), (63, 23, 3), (64, 23, 3), (65, 23, 3), (4097, 46, 257), (100003, 64, 5)])
def test_bootstrap_sums_against_the_oracle(n, C, R):
    """The draw's block counter is t >> 1 < 2^30 for every legal n: its high word (c1) is 0 at any size a test can reach, and at any
    legal size at all; the kernel and the oracle both still form it from the 64-bit counter."""
    X, n_int = boot_table(n, C, 1000 * C + R)
    seed = 5 + (7 << 32)
    Xd = torch.from_numpy(X).to(DEV)
    got = significance.bootstrap_sums(Xd, R, seed)
    assert got.shape == (R, C) and got.dtype == torch.float64
    again = significance.bootstrap_sums(Xd, R, seed).cpu().numpy()
    plain = tkr_hip.bootstrap_sums(Xd, R, seed, pad=False).cpu().numpy()      # the table's own row pitch: the same summation tree
    got = got.cpu().numpy()
    assert np.array_equal(got.view(np.uint64), again.view(np.uint64)) and np.array_equal(got.view(np.uint64), plain.view(np.uint64))
    want, mag = O.bootstrap_sums(X, R, seed, want_abs=True)
    assert np.array_equal(got[:, :n_int], want[:, :n_int].astype(np.float64))
    err = np.abs(got.astype(np.longdouble) - want)
    assert np.all(err <= n * 2.0 ** -52 * mag), float((err / np.maximum(mag, 1e-300)).max())
    low = significance.bootstrap_sums(Xd, R, 5).cpu().numpy()          # the seed's high word is part of the key
    if n >= 63:                                                       # (two draws of one or two lines may well agree)
        assert not np.array_equal(low[:, :n_int], got[:, :n_int])
    assert np.array_equal(low[:, :n_int], O.bootstrap_sums(X, R, 5)[:, :n_int].astype(np.float64))


def _named(lines):
    return {l.split(',')[0]: [float(x) for x in l.split(',')[1:]] for l in lines}


def _oracle_table(data, model, scenario, step, total):
    scores, lines = RO.load_lines(data, model, 0, scenario)
    ranks, like_ptr, rated_ptr = RO.csr_ranks(scores, lines)
    return O.line_table(ranks, like_ptr, rated_ptr, scores.shape[1], step, total)


def test_cli_bootstrap_and_compare_on_g4(golden_dir, tmp_path, capsys):
    import evaluate as E
    import textio
    d = os.path.join(golden_dir, 'g4')
    data, model = os.path.join(d, 'data'), os.path.join(d, 'model')
    metrics, scs, R, seed = ['acc', 'auc', 'ndcg'], ['im', 'om'], 200, 1
    base = ['-d', data, '-m', model, '-sl'] + scs + ['-M'] + metrics
    boot = ['--bootstrap', str(R), '--boot-seed', str(seed)]
    capsys.readouterr()
    plain = E.main(base)
    assert capsys.readouterr().out.strip().split('\n') == plain
    got = E.main(base + boot)
    assert capsys.readouterr().out.strip().split('\n') == got
    assert got[:len(plain)] == plain                                  # the leading lines: byte for byte
    tables = {sc: _oracle_table(data, model, sc, 5, 30) for sc in scs}
    want = [x for sc in scs for x in O.cli_lines(sc, tables[sc], None, 6, metrics, R, seed, 0.95)]
    new = got[len(plain):]
    assert [l.split(',')[0] for l in new] == [name for name, _ in want]
    for line, (name, vals) in zip(new, want):
        mine = [float(x) for x in line.split(',')[1:]]
        assert len(mine) == len(vals) and all(abs(a - b) <= 1e-6 for a, b in zip(mine, vals)), (line, vals)
        assert all(len(x.split('.')[1]) == 6 for x in line.split(',')[1:])
    by = _named(got)
    for sc in scs:
        for m in metrics:
            for lo, point, hi in zip(by['%s.%s.lo' % (sc, m)], by['%s.%s' % (sc, m)], by['%s.%s.hi' % (sc, m)]):
                assert lo <= point <= hi, (sc, m)
            assert any(lo < hi for lo, hi in zip(by['%s.%s.lo' % (sc, m)], by['%s.%s.hi' % (sc, m)])), (sc, m)
    # the same model twice: B's values are A's, every difference is 0, p = 1
    same = E.main(base + boot + ['--compare', model])
    capsys.readouterr()
    by = _named(same)
    assert same[:len(plain)] == plain and len(same) == len(plain) + 7 * len(scs) * len(metrics)
    for sc in scs:
        for m in metrics:
            assert by['%s.vs.%s' % (sc, m)] == by['%s.%s' % (sc, m)]
            for key in ('diff.%s', 'diff.%s.lo', 'diff.%s.hi'):
                assert by['%s.%s' % (sc, key % m)] == [0.0] * len(by['%s.%s' % (sc, m)])
            assert by['%s.diff.%s.p' % (sc, m)] == [1.0] * len(by['%s.%s' % (sc, m)])
    # a perturbed copy of the model
    other = tmp_path / 'model_b'
    shutil.copytree(model, other)
    V = textio.read_matrix(os.path.join(model, 'final-V.dat'), where='host')
    noise = np.random.Generator(np.random.PCG64(4)).standard_normal(V.shape).astype(np.float32)
    textio.write_matrix(str(other / 'final-V.dat'), (V + 0.15 * noise).astype(np.float32), where='host')
    got = E.main(base + boot + ['--compare', str(other)])
    capsys.readouterr()
    assert got[:len(plain)] == plain
    want = [x for sc in scs for x in O.cli_lines(sc, tables[sc], _oracle_table(data, str(other), sc, 5, 30), 6, metrics, R, seed, 0.95)]
    new = got[len(plain):]
    assert [l.split(',')[0] for l in new] == [name for name, _ in want]
    for line, (name, vals) in zip(new, want):
        mine = [float(x) for x in line.split(',')[1:]]
        assert len(mine) == len(vals) and all(abs(a - b) <= 1e-6 for a, b in zip(mine, vals)), (line, vals)
    by = _named(got)
    assert any(v != 0.0 for v in by['im.diff.ndcg']) and all(0.0 < p <= 1.0 for p in by['im.diff.ndcg.p'])
