"""K15 (csrc/group_dev.hip) without a GPU: the ABI and its refusals, the wrappers' refusals, the where / TKR_GROUP rule, the host path of
load_scenario against a plain restatement, and that restatement (tests/_group_oracle.py) against evaluate._group."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _group_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ('tkr_group_count_dev', 'tkr_group_emit_dev', 'tkr_last_line_of_user_dev', 'tkr_compact_rows_count_dev', 'tkr_compact_rows_emit_dev')
SCENARIOS = [('g4', 'im'), ('g4', 'om'), ('g5', 'im'), ('g5', 'om'), ('g6', 'all'), ('g6', 'im'), ('g6', 'om'), ('g7', 'sm')]
NAMES = ('users', 'like_ptr', 'like_cols', 'rated_ptr', 'rated_cols', 'seen_ptr', 'seen_cols')


def test_header_binding_and_library_agree():
    import tkr_hip
    header = open(os.path.join(ROOT, 'include', 'tkr.h')).read()
    declared = re.findall(r'^int(?:32_t|64_t)? (tkr_\w+)\(', header, flags=re.M)
    lib = C.CDLL(tkr_hip.LIB_PATH)
    for name in NEW:
        assert name in declared and name in tkr_hip.EXPORTS and hasattr(lib, name)
    assert int(re.search(r'#define TKR_GROUP_WAVE_COLS (\d+)', header).group(1)) == tkr_hip.GROUP_WAVE_COLS
    assert int(re.search(r'#define TKR_GROUP_MAX_COLS (\d+)', header).group(1)) == tkr_hip.GROUP_MAX_COLS
    # one wave's bitmap: 32 waves of a CU within its 160 KB; one workgroup's bitmap: within the 160 KB
    assert tkr_hip.GROUP_WAVE_COLS // 8 * 32 <= 160 * 1024 and tkr_hip.GROUP_MAX_COLS // 8 <= 160 * 1024 < tkr_hip.GROUP_MAX_COLS // 8 + 1024
    assert issubclass(tkr_hip.DeviceGroupTooLarge, tkr_hip.TkrError)
    for fn in (tkr_hip.group_segments, tkr_hip.last_line_of_user, tkr_hip.scenario_lines):
        assert callable(fn)


def _source(p, n_seg, n_entries, like=True, seg_of_row=True):
    import tkr_hip
    return tkr_hip.GroupSource(p, p, p if like else None, p if seg_of_row else None, n_seg, n_entries)


def test_entry_points_check_their_arguments_before_any_device_access():
    import tkr_hip
    lib = C.CDLL(tkr_hip.LIB_PATH)
    p = 4096                                                          # never dereferenced: every call below fails its checks
    count, emit = lib.tkr_group_count_dev, lib.tkr_group_emit_dev
    count.argtypes = [C.c_void_p, C.c_int32, C.c_int64, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p]
    emit.argtypes = [C.c_void_p, C.c_int32, C.c_int64, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p]
    assert count(None, 0, 0, 0, 0, None, None, None) == -1
    assert emit(None, 0, 0, 0, 0, None, None, 0, None, None) == -1
    one = (tkr_hip.GroupSource * 1)(_source(p, 10, 100))
    good = dict(src=C.cast(one, C.c_void_p), n_src=1, n_rows=10, n_cols=50, like_only=1, ptr=p, totals=p, stream=None)
    for change in (dict(src=None), dict(n_src=0), dict(n_src=3), dict(n_rows=0), dict(n_rows=-1), dict(n_cols=0), dict(n_cols=-5), dict(ptr=None),
                   dict(totals=None), dict(ptr=p + 4)):
        assert count(*dict(good, **change).values()) == -1, change
    for bad in (_source(None, 10, 100), tkr_hip.GroupSource(p, None, p, p, 10, 100), _source(p, 10, 100, like=False),
                _source(p, 9, 100, seg_of_row=False), _source(p, -1, 100), _source(p, 10, -1)):
        arr = (tkr_hip.GroupSource * 1)(bad)
        assert count(*dict(good, src=C.cast(arr, C.c_void_p)).values()) == -1
    # more columns than one workgroup's LDS holds: unsupported, still without touching the device
    assert count(*dict(good, n_cols=tkr_hip.GROUP_MAX_COLS + 1).values()) == -2
    good_e = dict(src=C.cast(one, C.c_void_p), n_src=1, n_rows=10, n_cols=50, like_only=0, ptr=p, cols=p, n_out=7, status=p, stream=None)
    for change in (dict(src=None), dict(n_rows=0), dict(n_cols=0), dict(ptr=None), dict(cols=None), dict(n_out=-1), dict(status=None)):
        assert emit(*dict(good_e, **change).values()) == -1, change
    assert emit(*dict(good_e, n_cols=tkr_hip.GROUP_MAX_COLS + 1).values()) == -2
    last = lib.tkr_last_line_of_user_dev
    last.argtypes = [C.c_void_p, C.c_int64, C.c_int64, C.c_void_p, C.c_void_p]
    for args in ((None, 5, 5, p), (p, 0, 5, p), (p, 5, 0, p), (p, 5, 5, None), (p, -1, 5, p)):
        assert last(*args, None) == -1, args
    cc, ce = lib.tkr_compact_rows_count_dev, lib.tkr_compact_rows_emit_dev
    cc.argtypes = [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p]
    ce.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    for args in ((None, 5, p), (p, 0, p), (p, 5, None)):
        assert cc(*args, None) == -1, args
    for args in ((None, p, 5, 2, p, p, p), (p, None, 5, 2, p, p, p), (p, p, 0, 0, p, p, p), (p, p, 5, 6, p, p, p), (p, p, 5, -1, p, p, p),
                 (p, p, 5, 2, None, p, p), (p, p, 5, 2, p, None, p), (p, p, 5, 2, p, p, None)):
        assert ce(*args, None) == -1, args


def test_wrappers_refuse_dtype_layout_and_device_before_any_device_access():
    import tkr_hip
    seg_ptr, item, like = torch.tensor([0, 2, 3]), torch.tensor([1, 2, 3], dtype=torch.int32), torch.tensor([1, 0, 1], dtype=torch.int32)
    G = tkr_hip.group_segments
    with pytest.raises(TypeError, match='seg_ptr must be torch.int64'):
        G([(seg_ptr.int(), item, like, None)], 2, 10)
    with pytest.raises(TypeError, match='must be a tensor'):
        G([([0, 2, 3], item, like, None)], 2, 10)
    with pytest.raises(TypeError, match='a source is'):
        G([(seg_ptr, item)], 2, 10)
    with pytest.raises(ValueError, match='one or two sources'):
        G([], 2, 10)
    with pytest.raises(ValueError, match='must be contiguous'):
        G([(torch.zeros(6, dtype=torch.int64)[::2], item, like, None)], 2, 10)
    with pytest.raises(ValueError, match='must live on the GPU'):      # host tensors: refused, never handed to the library
        G([(seg_ptr, item, like, None)], 2, 10)
    with pytest.raises(ValueError, match='n_cols >= 1'):
        G([(seg_ptr, item, like, None)], 2, 0)
    with pytest.raises(TypeError, match='line_user must be torch.int32'):
        tkr_hip.last_line_of_user(torch.zeros(4, dtype=torch.int64), 3)
    with pytest.raises(ValueError, match='must live on the GPU'):
        tkr_hip.last_line_of_user(torch.zeros(4, dtype=torch.int32), 3)
    with pytest.raises(TypeError, match='ptr must be torch.int64'):
        tkr_hip.scenario_lines(torch.zeros(4, dtype=torch.int32))
    with pytest.raises(ValueError, match='must live on the GPU'):
        tkr_hip.scenario_lines(torch.zeros(4, dtype=torch.int64))


def test_where_and_environment_are_validated(monkeypatch, golden_dir):
    import evaluate
    import recommend
    import textio
    assert textio.GROUP_WHERE == ('host', 'device', 'auto') and textio.group_counts.keys() == {'host', 'device'}
    with pytest.raises(ValueError, match='where / TKR_GROUP must be one of host, device, auto'):
        textio._group_where('gpu')
    monkeypatch.setenv('TKR_GROUP', 'nowhere')
    with pytest.raises(ValueError, match="where / TKR_GROUP must be one of host, device, auto, got 'nowhere'"):
        textio._group_where(None)
    data = os.path.join(golden_dir, 'g4', 'data')
    with pytest.raises(ValueError, match='TKR_GROUP'):
        evaluate.load_scenario(data, 0, 'im', evaluate.read_ids(os.path.join(data, 'uid')))
    with pytest.raises(ValueError, match='TKR_GROUP'):
        recommend.candidate_lines(os.path.join(data, 'f0tr.txt'), {}, {}, 5, where='everywhere')
    monkeypatch.setenv('TKR_GROUP', 'host')
    assert textio._group_where(None) == 'host' and textio._group_where('auto') == 'auto'
    monkeypatch.delenv('TKR_GROUP')
    assert textio._group_where(None) == 'auto'
    monkeypatch.setenv('TKR_GROUP_DEVICE_FROM', '123')
    assert textio._group_device_from() == 123
    monkeypatch.delenv('TKR_GROUP_DEVICE_FROM')
    assert textio._group_device_from() == textio.GROUP_DEVICE_FROM


def test_auto_without_a_gpu_groups_on_the_host_and_device_raises(golden_dir, monkeypatch):
    import evaluate
    import textio
    import tkr_hip
    monkeypatch.setattr(torch.cuda, 'is_available', lambda: False)      # what the rule does on a machine without a GPU
    monkeypatch.setenv('TKR_GROUP_DEVICE_FROM', '1')
    data = os.path.join(golden_dir, 'g4', 'data')
    uids = evaluate.read_ids(os.path.join(data, 'uid'))
    before = dict(textio.group_counts)
    evaluate.load_scenario(data, 0, 'im', uids, where='auto')
    evaluate.load_scenario(data, 0, 'om', uids)
    assert textio.group_counts == {'host': before['host'] + 2, 'device': before['device']}
    with pytest.raises(tkr_hip.TkrError, match='no MI355X is visible'):
        evaluate.load_scenario(data, 0, 'im', uids, where='device')


@pytest.mark.parametrize('g,scenario', SCENARIOS)
def test_host_path_equals_the_restatement_on_the_golden_sets(golden_dir, g, scenario):
    import evaluate
    import textio
    data = os.path.join(golden_dir, g, 'data')
    uids = evaluate.read_ids(os.path.join(data, 'uid'))
    teids = evaluate.read_ids(os.path.join(data, 'f0te.%s.idl' % scenario))
    sc = evaluate.load_scenario(data, 0, scenario, uids, where='host')
    T = textio.parse_ratings(os.path.join(data, 'f0te.%s.txt' % scenario), uids, teids, where='host')
    H = textio.parse_ratings(os.path.join(data, 'f0tr.txt'), uids, teids, where='host')
    for name, want in zip(NAMES, O.scenario(T, H)):
        got = getattr(sc, name)
        assert got.dtype == want.dtype and got.shape == want.shape and np.array_equal(got, want), name
    assert sc.tcount == int(sc.like_ptr[-1]) and getattr(sc, 'dev', None) is None


@pytest.mark.parametrize('seed', range(6))
def test_oracle_equals_group_on_grouped_rows(seed):
    """the yardstick of the GPU tests is pinned to evaluate._group: identity rows, gathered rows with repeats, and a union of two"""
    import evaluate
    rng = np.random.Generator(np.random.PCG64(seed))
    n_cols = int(rng.choice([1, 7, 33, 500]))
    n_seg, n_rows = 30, 45
    a, b = O.random_source(rng, n_seg, n_cols), O.random_source(rng, n_seg, n_cols)
    for like_only in (False, True):
        for sources in ([a + (None,)], [a + (rng.integers(-1, n_seg, n_rows),)], [a + (rng.integers(-1, n_seg, n_rows),), b + (rng.integers(-1, n_seg, n_rows),)]):
            rows_n = n_seg if sources[0][3] is None else n_rows
            rr, cc = [], []
            for seg_ptr, item, like, seg_of_row in sources:
                for r in range(rows_n):
                    g = r if seg_of_row is None else int(seg_of_row[r])
                    if g < 0:
                        continue
                    e = np.arange(seg_ptr[g], seg_ptr[g + 1])
                    keep = (item[e] >= 0) & ((like[e] == 1) | (not like_only))
                    rr.append(np.full(int(keep.sum()), r, dtype=np.int64))
                    cc.append(item[e][keep].astype(np.int64))
            want = evaluate._group(np.concatenate(rr), np.concatenate(cc), rows_n, n_cols)
            got = O.group_segments(sources, rows_n, like_only)
            for x, y in zip(got, want):
                assert x.dtype == y.dtype and np.array_equal(x, y)


def test_oracle_helpers_on_hand_worked_input():
    assert O.last_line_of_user(np.array([2, -1, 0, 2, -1, 2, 7], dtype=np.int32), 4).tolist() == [2, -1, 5, -1]
    rows, ptr = O.scenario_lines(np.array([0, 0, 3, 3, 4, 4], dtype=np.int64))
    assert rows.tolist() == [1, 3] and ptr.tolist() == [0, 3, 4] and rows.dtype == ptr.dtype == np.int64


def test_recommend_parser_knows_group(golden_dir, tmp_path, capsys):
    import recommend
    d = os.path.join(golden_dir, 'g4')
    with pytest.raises(SystemExit):
        recommend.main(['-d', os.path.join(d, 'data'), '-m', os.path.join(d, 'model'), '-o', str(tmp_path / 'o.txt'), '--group', 'gpu'])
    assert '--group' in capsys.readouterr().err
