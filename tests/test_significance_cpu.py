"""K18 (tkr_line_metrics, tkr_bootstrap_sums, significance.py, evaluate.py --bootstrap) without a GPU: the oracle's table against
rankmetrics.rank_sums, the ABI and its argument checks, the interval and the p-value on hand-written cases, what the command line
refuses, and a few literal draw indices."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _rank_oracle as RO
import _significance_oracle as O

import rankmetrics
import significance

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN_CASES = [('g4', 'im'), ('g4', 'om'), ('g5', 'im'), ('g5', 'om'), ('g6', 'all'), ('g7', 'sm')]
V_, I32, I64, U64 = C.c_void_p, C.c_int32, C.c_int64, C.c_uint64
LINE_ARGTYPES = [V_, I64, V_, V_, I64, I32, I32, I32, V_, V_, V_, V_, V_]
BOOT_ARGTYPES = [V_, I64, I32, I64, I32, U64, V_, V_, I64, V_]


def synthetic_ranks(seed, n_lines, n_cols, max_likes):
    """distinct ranks below the line's unrated count, some likes rated (-1), some lines without a ranked like"""
    rng = np.random.Generator(np.random.PCG64(seed))
    ranks, like_ptr, rated_ptr = [], [0], [0]
    for r in range(n_lines):
        rated = int(rng.integers(0, n_cols // 2))
        cap = n_cols - rated
        P = 0 if r % 11 == 3 else int(rng.integers(1, min(max_likes, cap) + 1))
        line = rng.choice(cap, P, replace=False).tolist() + [-1] * int(rng.integers(0, 3))
        rng.shuffle(line)
        if not line:
            line = [-1]
        ranks += line
        like_ptr.append(len(ranks))
        rated_ptr.append(rated_ptr[-1] + rated)
    return np.array(ranks, dtype=np.int64), np.array(like_ptr, dtype=np.int64), np.array(rated_ptr, dtype=np.int64)


def check_table_against_rank_sums(X, ranks, like_ptr, rated_ptr, n_cols, step, total):
    """integer columns equal; every float column sum within n_lines * 2^-52 * sum |x| of rank_sums' (the bound for reordering a
    float64 sum)"""
    sums = rankmetrics.rank_sums(ranks, like_ptr, rated_ptr, n_cols, step, total)
    i, n = total // step, X.shape[0]
    col = X.sum(0)
    np.testing.assert_array_equal(col[:i], sums['acc'][0])
    assert col[i] == sums['acc'][1] and col[i + 2] == sums['auc'][1]
    assert col[i + 4] == sums['mrr'][1] == sums['ndcg'][1] == sums['map'][1]
    bound = n * 2.0 ** -52 * np.abs(X).sum(0)
    assert abs(col[i + 1] - sums['auc'][0]) <= bound[i + 1]
    assert abs(col[i + 3] - sums['mrr'][0]) <= bound[i + 3]
    assert np.all(np.abs(col[i + 5:2 * i + 5] - sums['ndcg'][0]) <= bound[i + 5:2 * i + 5])
    assert np.all(np.abs(col[2 * i + 5:] - sums['map'][0]) <= bound[2 * i + 5:])


@pytest.mark.parametrize('step,total', [(5, 30), (7, 30), (1, 1), (3, 7)])
def test_oracle_table_against_rank_sums_on_synthetic_ranks(step, total):
    ranks, like_ptr, rated_ptr = synthetic_ranks(5, 120, 90, 40)
    X = O.line_table(ranks, like_ptr, rated_ptr, 90, step, total)
    assert X.shape == (120, 3 * (total // step) + 5) == (120, significance.n_columns(total // step))
    check_table_against_rank_sums(X, ranks, like_ptr, rated_ptr, 90, step, total)


@pytest.mark.parametrize('case', GOLDEN_CASES)
def test_oracle_table_against_rank_sums_on_goldens(golden_dir, case):
    d = os.path.join(golden_dir, case[0])
    scores, lines = RO.load_lines(os.path.join(d, 'data'), os.path.join(d, 'model'), 0, case[1])
    ranks, like_ptr, rated_ptr = RO.csr_ranks(scores, lines)
    for step, total in ((5, 30), (7, 64)):
        X = O.line_table(ranks, like_ptr, rated_ptr, scores.shape[1], step, total)
        check_table_against_rank_sums(X, ranks, like_ptr, rated_ptr, scores.shape[1], step, total)
        got = significance.values(X.sum(0), total // step)
        want = rankmetrics.finish(rankmetrics.rank_sums(ranks, like_ptr, rated_ptr, scores.shape[1], step, total))
        for m in rankmetrics.METRICS:
            np.testing.assert_allclose(got[m], want[m], rtol=1e-12, atol=0)


def test_oracle_refuses_what_the_kernel_refuses():
    good = dict(ranks=[0, 3, -1, 2], like_ptr=[0, 3, 4], rated_ptr=[0, 2, 2], n_cols=6, step=2, total=4)
    O.line_table(**good)
    for change in (dict(ranks=[0, 3, -2, 2]), dict(ranks=[0, 4, -1, 2]), dict(ranks=[0, 0, -1, 2]), dict(like_ptr=[1, 3, 4]),
                   dict(like_ptr=[0, 3, 2]), dict(rated_ptr=[0, 2, 1]), dict(like_ptr=[0, 3, 5])):
        with pytest.raises(O.Refused):
            O.line_table(**dict(good, **change))


def test_header_binding_and_library_agree_and_check_their_arguments():
    import tkr_hip
    header = open(os.path.join(ROOT, 'include', 'tkr.h')).read()
    declared = re.findall(r'^int(?:32_t|64_t)? (tkr_\w+)\(', header, flags=re.M)
    lib = C.CDLL(tkr_hip.LIB_PATH)
    for name in ('tkr_line_metrics', 'tkr_bootstrap_sums'):
        assert name in declared and name in tkr_hip.EXPORTS and hasattr(lib, name)
    for macro, value in (('TKR_LINE_MAX_TOTAL', tkr_hip.LINE_MAX_TOTAL), ('TKR_LINE_MAX_COLS', tkr_hip.LINE_MAX_COLS),
                         ('TKR_BOOT_MAX_COLUMNS', tkr_hip.BOOT_MAX_COLUMNS), ('TKR_BOOT_CHUNK', tkr_hip.BOOT_CHUNK)):
        assert re.search(r'#define %s %d\b' % (macro, value), header), macro
    assert tkr_hip.LINE_MAX_TOTAL == 1024 and tkr_hip.BOOT_MAX_COLUMNS == 64
    assert lib.tkr_version() == tkr_hip.VERSION
    p = 4096                                                          # never dereferenced: every call below fails its checks
    fn = lib.tkr_line_metrics
    fn.restype, fn.argtypes = C.c_int, LINE_ARGTYPES
    good = dict(ranks=p, n_likes=10, lptr=p, rptr=p, n_lines=3, n_cols=90, step=5, total=30, gain=p, ideal=p, X=p, status=p, stream=None)
    assert len(good) == len(LINE_ARGTYPES)
    for change in (dict(ranks=None), dict(lptr=None), dict(rptr=None), dict(gain=None), dict(ideal=None), dict(X=None), dict(status=None),
                   dict(n_likes=-1), dict(n_lines=0), dict(n_cols=0), dict(step=0), dict(total=0), dict(X=p + 4), dict(status=p + 4)):
        assert fn(*dict(good, **change).values()) == -1, change
    assert fn(*dict(good, total=1025).values()) == -2                 # TKR_E_UNSUPPORTED
    assert fn(*dict(good, n_cols=tkr_hip.LINE_MAX_COLS + 1).values()) == -2
    assert fn(*dict(good, total=1025, X=None).values()) == -1         # what is invalid is invalid at any size
    fn = lib.tkr_bootstrap_sums
    fn.restype, fn.argtypes = C.c_int, BOOT_ARGTYPES
    good = dict(X=p, n=1000, C=23, pitch=32, R=10, seed=1, out=p, ws=p, ws_bytes=10 * 23 * 8, stream=None)
    assert len(good) == len(BOOT_ARGTYPES)
    for change in (dict(X=None), dict(out=None), dict(ws=None), dict(C=0), dict(C=65), dict(C=-1), dict(pitch=22), dict(pitch=0), dict(C=64), dict(n=0), dict(n=-1), dict(n=2 ** 31),
                   dict(R=0), dict(R=-1), dict(ws_bytes=10 * 23 * 8 - 1), dict(n=8193), dict(out=p + 4)):
        assert fn(*dict(good, **change).values()) == -1, change
    assert [tkr_hip.boot_pitch(c) for c in (1, 8, 9, 16, 17, 23, 32, 33, 46, 48, 49, 64)] == [8, 8, 16, 16, 32, 32, 32, 48, 48, 48, 64, 64]


def test_wrappers_refuse_on_the_host():
    """tensor properties are looked at before the library is asked: CPU tensors never reach a kernel"""
    import torch
    import tkr_hip
    with pytest.raises(tkr_hip.TkrError, match='GPU'):
        tkr_hip.bootstrap_sums(torch.zeros((5, 4), dtype=torch.float64), 3, 0)
    with pytest.raises(tkr_hip.TkrError, match='float64'):
        tkr_hip.bootstrap_sums(torch.zeros((5, 4)), 3, 0)
    with pytest.raises(tkr_hip.TkrError, match='GPU'):
        significance.line_table(torch.zeros(3, dtype=torch.int32), torch.zeros(2, dtype=torch.int64), torch.zeros(2, dtype=torch.int64), 9, 1, 3)


def test_interval_and_p_value_known_answers():
    v = np.arange(1.0, 21.0)                                          # R = 20: j = floor(0.025 * 20) = 0, floor(0.05 * 20) = 1, floor(0.25 * 20) = 5
    assert significance.interval_of(v, 0.95) == (1.0, 20.0)
    assert significance.interval_of(v, 0.90) == (2.0, 19.0)
    assert significance.interval_of(v, 0.50) == (6.0, 15.0)
    assert significance.interval_of(np.arange(200.0), 0.95) == (5.0, 194.0)
    assert significance.interval_of([7.0], 0.95) == (7.0, 7.0)
    for level in (0.0, 1.0, -0.5):
        with pytest.raises(ValueError):
            significance.interval_of(v, level)
    # R = 9: all positive -> 2 * min(1 / 10, 10 / 10) = 0.2;  two of nine <= 0 -> 2 * 3 / 10;  all zero -> min(1, 2) = 1;  four below,
    # five above -> 2 * min(5 / 10, 6 / 10) = 1
    assert significance.p_value([1.0] * 9) == pytest.approx(0.2, abs=1e-15)
    assert significance.p_value([-1.0] * 9) == pytest.approx(0.2, abs=1e-15)
    assert significance.p_value([-1.0, 0.0] + [1.0] * 7) == pytest.approx(0.6, abs=1e-15)
    assert significance.p_value([0.0] * 9) == 1.0
    assert significance.p_value([-1.0] * 4 + [1.0] * 5) == 1.0
    assert significance.p_value([3.0] * 999) == pytest.approx(0.002, abs=1e-15)


def test_values_report_and_zero_denominators():
    interval = 2
    names = significance.columns(interval)
    assert len(names) == significance.n_columns(interval) == 11 and len(set(names)) == 11
    assert names[interval] == 'likes' and names[interval + 2] == 'auc.n' and names[interval + 4] == 'rr.n'
    #        hits    likes auc n   rr  n   ndcg      ap
    point = [3, 5,   10,   1.5, 2, 2.0, 4, 1.0, 3.0, 0.5, 2.5]
    got = significance.values(point, interval)
    assert {m: list(v) for m, v in got.items()} == {'acc': [0.3, 0.5], 'auc': [0.75], 'mrr': [0.5], 'ndcg': [0.25, 0.75], 'map': [0.125, 0.625]}
    assert list(significance.values(point, interval, ('mrr',))) == ['mrr']
    reps = np.array([point, [2, 4, 8, 1.0, 2, 1.0, 4, 2.0, 2.0, 1.0, 1.0], [4, 4, 8, 2.0, 2, 4.0, 4, 4.0, 4.0, 2.0, 2.0]])
    got = significance.values(reps, interval)
    np.testing.assert_array_equal(got['acc'], [[0.3, 0.5], [0.25, 0.5], [0.5, 0.5]])
    np.testing.assert_array_equal(got['mrr'], [[0.5], [0.25], [1.0]])
    # identical columns side by side: the difference is 0 in every replicate -> interval (0, 0), p = 1
    both = np.concatenate([reps, reps], axis=1)
    rep = significance.report(np.concatenate([point, point]), both, interval, rankmetrics.METRICS, 0.95, 2)
    for m in rankmetrics.METRICS:
        width = 2 if m in rankmetrics.PER_BUCKET else 1
        assert rep[m]['diff'] == rep[m]['diff.lo'] == rep[m]['diff.hi'] == [0.0] * width and rep[m]['diff.p'] == [1.0] * width
        assert rep[m]['vs'] == list(significance.values(point, interval)[m])
    assert rep['acc']['lo'] == [0.25, 0.5] and rep['acc']['hi'] == [0.5, 0.5] and rep['mrr']['lo'] == [0.25] and rep['mrr']['hi'] == [1.0]
    assert set(significance.report(point, reps, interval, ('auc',), 0.95)['auc']) == {'lo', 'hi'}
    # a zero denominator in the point estimate or in ANY replicate
    for column, metric in ((interval, 'acc'), (interval + 2, 'auc'), (interval + 4, 'mrr'), (interval + 4, 'ndcg'), (interval + 4, 'map')):
        broken = reps.copy()
        broken[1, column] = 0.0
        with pytest.raises(ZeroDivisionError, match=metric):
            significance.values(broken, interval, (metric,))
        with pytest.raises(ZeroDivisionError, match=metric):
            significance.values(broken[1], interval, (metric,))
        with pytest.raises(ZeroDivisionError, match=metric):
            significance.report(point, broken, interval, (metric,), 0.95)
        if metric != 'auc':
            significance.values(broken, interval, ('auc',))            # the other metrics are not touched
    with pytest.raises(ValueError):
        significance.values(point[:-1], interval)


def test_command_line_refuses_bad_bootstrap_arguments(golden_dir, monkeypatch):
    """parser.error, before anything asks for a GPU or reads a file"""
    import evaluate
    d = os.path.join(golden_dir, 'g4')
    ev = ['-d', os.path.join(d, 'data'), '-m', os.path.join(d, 'model'), '-t', '30', '-sl', 'im']
    model = os.path.join(d, 'model')
    bad = (['--bootstrap', '100'], ['--bootstrap', '100', '-M', 'ild'], ['--bootstrap', '100', '-M', 'hr', '--negatives', '5'],
           ['--compare', model], ['--compare', model, '-M', 'acc'], ['-M', 'acc', '--bootstrap', '0'], ['-M', 'acc', '--bootstrap', '-3'],
           ['-M', 'acc', '--bootstrap', 'many'], ['-M', 'acc', '--bootstrap', '10', '--level', '0'],
           ['-M', 'acc', '--bootstrap', '10', '--level', '1'], ['-M', 'acc', '--bootstrap', '10', '--level', '1.5'],
           ['-M', 'acc', '--bootstrap', '10', '--level', 'nan'], ['-M', 'acc', '--bootstrap', '10', '--boot-seed', '-1'],
           ['-M', 'acc', '--bootstrap', '10', '--boot-seed', str(2 ** 64)])
    for extra in bad:
        with pytest.raises(SystemExit) as stop:
            evaluate.main(ev + extra)
        assert stop.value.code == 2, extra
    monkeypatch.setenv('WORLD_SIZE', '2')                             # a multi-rank launcher: not sharded
    for extra in (['-M', 'acc', '--bootstrap', '10'], ['-M', 'auc', '--bootstrap', '10', '--compare', model]):
        with pytest.raises(SystemExit) as stop:
            evaluate.main(ev + extra)
        assert stop.value.code == 2, extra


def test_draw_indices_are_pinned():
    """the stream definition as literal numbers (oracle/plan_np.py's Philox and mulhi64, stream word 3): PINNED below"""
    assert O.draw(1000, 0, 0)[:6].tolist() == PINNED[0]
    assert O.draw(1000, 7, 1)[:6].tolist() == PINNED[1]
    assert O.draw(480189, 999, (5 << 32) | 9)[-4:].tolist() == PINNED[2]
    assert O.draw(1000, 2, 2 ** 63)[:3].tolist() == PINNED[3]
    assert not np.array_equal(O.draw(1001, 4, 11)[:1000], O.draw(1000, 4, 11))            # n enters every index
    assert not np.array_equal(O.draw(1000, 0, 1), O.draw(1000, 0, 1 + (1 << 32)))         # the seed's high word is used
    idx = O.draw(100003, 1, 3)
    assert idx.min() >= 0 and idx.max() < 100003 and len(idx) == 100003


PINNED = [[841, 774, 225, 117, 266, 935], [947, 708, 983, 215, 314, 802], [400861, 471080, 432790, 362984], [97, 122, 91]]
