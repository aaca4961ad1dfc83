"""K15 on the GPU (csrc/group_dev.hip): tkr_hip.group_segments, last_line_of_user and scenario_lines against the plain restatement of
tests/_group_oracle.py, and the device path of evaluate.load_scenario / recommend.rank / recommend.candidate_lines against the host path.
Every comparison is exact: values, dtype and shape."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _group_oracle as O

pytestmark = pytest.mark.gpu

SCENARIOS = [('g4', 'im'), ('g4', 'om'), ('g5', 'im'), ('g5', 'om'), ('g6', 'all'), ('g6', 'im'), ('g6', 'om'), ('g7', 'sm')]
NAMES = ('users', 'like_ptr', 'like_cols', 'rated_ptr', 'rated_cols', 'seen_ptr', 'seen_cols')


def _dev(x):
    return None if x is None else torch.from_numpy(np.ascontiguousarray(x)).cuda()


def _same(got, want, what=''):
    got = got.cpu().numpy() if isinstance(got, torch.Tensor) else got
    assert got.dtype == want.dtype and got.shape == want.shape and np.array_equal(got, want), what


def _check(sources, n_rows, n_cols, like_only):
    import tkr_hip
    ptr, cols = tkr_hip.group_segments([tuple(_dev(np.asarray(a, dtype=np.int64) if k in (0, 3) and a is not None else a) for k, a in enumerate(s))
                                        for s in sources], n_rows, n_cols, like_only=like_only)
    want_ptr, want_cols = O.group_segments(sources, n_rows, like_only)
    _same(ptr, want_ptr, 'ptr')
    _same(cols, want_cols, 'cols')


def test_rows_of_every_length_in_one_call():
    """0 ... 5,000 entries per row, 14 rows (not a multiple of the 4 rows of a workgroup); a row of unknown items only, a row that is one
    column 300 times, a row that holds columns 0 and n_cols - 1"""
    rng = np.random.Generator(np.random.PCG64(1))
    n_cols = 1000
    lengths = [0, 1, 2, 63, 64, 65, 127, 128, 129, 1000, 5000, 70, 300, 2]
    seg_ptr, item, like = O.random_source(rng, len(lengths), n_cols, lengths)
    item[seg_ptr[11]:seg_ptr[12]] = -1
    item[seg_ptr[12]:seg_ptr[13]] = 417
    item[seg_ptr[13]:seg_ptr[14]] = (0, n_cols - 1)
    like[seg_ptr[12]:seg_ptr[14]] = 1
    for like_only in (False, True):
        _check([(seg_ptr, item, like, None)], len(lengths), n_cols, like_only)
    _check([(seg_ptr, item, None, None)], len(lengths), n_cols, False)      # no like array at all


def _cols_cases():
    import tkr_hip
    W, M = tkr_hip.GROUP_WAVE_COLS, tkr_hip.GROUP_MAX_COLS
    return [1, 31, 32, 33, 63, 64, 65, 1000, W - 1, W, W + 1, M]


@pytest.mark.parametrize('case', range(12))
def test_column_counts_at_every_word_and_team_boundary(case):
    """two sources with overlapping sets; seg_of_row with repeats, out of order, -1 in one source or in both; like values -1, 0, 1, 2"""
    n_cols = _cols_cases()[case]
    rng = np.random.Generator(np.random.PCG64(100 + case))
    n_seg, n_rows = 9, 13
    a = O.random_source(rng, n_seg, n_cols, rng.integers(0, 200, n_seg))
    b = O.random_source(rng, n_seg, n_cols, rng.integers(0, 200, n_seg))
    a[1][:2] = (0, n_cols - 1)
    a[2][:2] = 1
    b[1][int(b[0][n_seg]) - 1] = n_cols - 1
    ra = np.array([3, 3, 8, -1, 0, 5, -1, 7, 1, 3, -1, 2, 0], dtype=np.int64)
    rb = np.array([2, -1, 8, -1, 4, 4, 1, -1, 0, 6, -1, 8, 0], dtype=np.int64)
    for like_only in (False, True):
        _check([a + (ra,), b + (rb,)], n_rows, n_cols, like_only)
    _check([a + (None,)], n_seg, n_cols, True)
    _check([a + (ra,)], n_rows, n_cols, False)


def test_no_row_one_row_and_too_many_columns():
    import tkr_hip
    rng = np.random.Generator(np.random.PCG64(3))
    a = O.random_source(rng, 5, 77)
    _check([a + (None,)], 0, 77, False)
    _check([a + (np.zeros(0, dtype=np.int64),)], 0, 77, True)
    _check([a + (None,)], 1, 77, True)
    _check([a + (np.array([4]),)], 1, 77, False)
    empty = (np.zeros(1, dtype=np.int64), np.zeros(0, dtype=np.int32), np.zeros(0, dtype=np.int32), np.full(3, -1, dtype=np.int64))
    _check([empty], 3, 77, True)                                       # a file without a line
    with pytest.raises(tkr_hip.DeviceGroupTooLarge):
        _check([a + (None,)], 5, tkr_hip.GROUP_MAX_COLS + 1, False)
    _check([a + (None,)], 5, 77, False)


def test_bad_input_is_refused_and_the_process_goes_on():
    import tkr_hip
    rng = np.random.Generator(np.random.PCG64(4))
    n_cols = 50
    seg_ptr, item, like = O.random_source(rng, 6, n_cols, [5, 9, 0, 70, 3, 8])
    good = [(seg_ptr, item, like, None)]
    bad_item = item.copy()
    bad_item[7] = n_cols                                               # never a bit index
    with pytest.raises(ValueError, match='item >= n_cols'):
        _check([(seg_ptr, bad_item, like, None)], 6, n_cols, False)
    _check(good, 6, n_cols, False)
    down = seg_ptr.copy()
    down[2] = down[1] - 3                                              # seg_ptr decreases
    with pytest.raises(ValueError, match='seg_ptr decreases'):
        _check([(down, item, like, None)], 6, n_cols, True)
    past = seg_ptr.copy()
    past[-1] += 4                                                      # a segment past the entries
    with pytest.raises(ValueError, match='seg_ptr decreases or leaves'):
        _check([(past, item, like, None)], 6, n_cols, True)
    _check(good, 6, n_cols, True)
    for bad in (6, -2):                                                # seg_of_row == n_seg, and below -1
        with pytest.raises(ValueError, match='seg_of_row'):
            _check([(seg_ptr, item, like, np.array([0, bad, 2], dtype=np.int64))], 3, n_cols, False)
    _check([(seg_ptr, item, like, np.array([0, 5, 2], dtype=np.int64))], 3, n_cols, False)


def test_last_line_of_user_and_scenario_lines():
    import tkr_hip
    line_user = np.array([2, -1, 0, 2, -1, -1, 2, 4, 9], dtype=np.int32)      # user 2 on three lines, 1 and 3 on none, 9 beyond n_users
    _same(tkr_hip.last_line_of_user(_dev(line_user), 5), O.last_line_of_user(line_user, 5))
    _same(tkr_hip.last_line_of_user(_dev(line_user[:0]), 3), O.last_line_of_user(line_user[:0], 3))
    rng = np.random.Generator(np.random.PCG64(5))
    many = rng.integers(-1, 3000, 20000).astype(np.int32)
    _same(tkr_hip.last_line_of_user(_dev(many), 3000), O.last_line_of_user(many, 3000))
    for sizes in ([0, 0, 0, 0, 0], [2, 1, 7], [0, 3, 0, 0, 1, 0], list(rng.integers(0, 3, 5000))):      # no row kept, all kept, some
        ptr = np.zeros(len(sizes) + 1, dtype=np.int64)
        np.cumsum(sizes, out=ptr[1:])
        rows, out = tkr_hip.scenario_lines(_dev(ptr))
        want = O.scenario_lines(ptr)
        _same(rows, want[0])
        _same(out, want[1])
    rows, out = tkr_hip.scenario_lines(_dev(np.zeros(1, dtype=np.int64)))
    assert rows.numel() == 0 and out.tolist() == [0]


def _compare_paths(data, scenario):
    import evaluate
    import textio
    uids = evaluate.read_ids(os.path.join(data, 'uid'))
    host = evaluate.load_scenario(data, 0, scenario, uids, where='host')
    before = textio.group_counts['device']
    dev = evaluate.load_scenario(data, 0, scenario, uids, where='device')
    assert textio.group_counts['device'] == before + 1
    for name in NAMES:
        _same(getattr(dev, name), getattr(host, name), name)
        _same(dev.dev[name], getattr(host, name), name)
    assert dev.tcount == host.tcount and dev.teids == host.teids
    return host, dev


@pytest.mark.parametrize('g,scenario', SCENARIOS)
def test_load_scenario_device_equals_host_on_the_golden_sets(golden_dir, g, scenario):
    _compare_paths(os.path.join(golden_dir, g, 'data'), scenario)


def write_fuzz_set(root, seed=0, extra_test_lines=(), drop_train_of=None):
    """a data directory: 30 users, 40 test ids.  Users with two and three train lines (the last one wins), test lines without a like
    (dropped), unknown users and items in the train file, an item twice on a line, a train line with no test column"""
    rng = np.random.Generator(np.random.PCG64(seed))
    users, items = ['u%d' % k for k in range(30)], ['i%d' % k for k in range(40)]
    os.makedirs(root, exist_ok=True)
    with open(os.path.join(root, 'uid'), 'w') as fh:
        fh.write(''.join(u + '\n' for u in users))
    with open(os.path.join(root, 'f0te.fz.idl'), 'w') as fh:
        fh.write(''.join(i + '\n' for i in items))

    def fields(n, pool, likes=(0, 1)):
        return ['%s:%d' % (pool[int(rng.integers(len(pool)))], int(rng.choice(likes))) for _ in range(n)]

    train = []
    for k, u in enumerate(users):
        if u == drop_train_of:
            continue
        for _ in range(1 + (k % 5 == 0) + (k % 10 == 0)):              # two lines for every 5th user, three for every 10th
            train.append(','.join([u] + fields(int(rng.integers(1, 12)), items + ['x1', 'x2'])))      # x1, x2: not test ids
    train.append('u8,x1:1,x2:0')                                       # u8's LAST line has no test column: nothing is rated
    train.append('stranger,i1:1,i2:1')                                 # a user the uid list does not have
    train.insert(3, 'u5,i5:1,i5:0,i5:1,i9:1')                          # an item three times on a line
    order = rng.permutation(len(train) - 2)                            # (u8's and the stranger's line stay last)
    train = [train[j] for j in order] + train[-2:]
    with open(os.path.join(root, 'f0tr.txt'), 'w') as fh:
        fh.write(''.join(ln + '\n' for ln in train))
    test = []
    for k, u in enumerate(users):
        if k % 4 == 3:
            test.append(','.join([u] + fields(int(rng.integers(1, 6)), items, likes=(0, 2, -1))))      # no like: the line is dropped
        elif k % 7 != 6:                                               # (every 7th user has no test line)
            test.append(','.join([u] + fields(int(rng.integers(1, 9)), items) + ['i%d:1' % (k % 40), 'i%d:1' % (k % 40)]))
    test += list(extra_test_lines)
    with open(os.path.join(root, 'f0te.fz.txt'), 'w') as fh:
        fh.write(''.join(ln + '\n' for ln in test))
    return root


def test_load_scenario_device_equals_host_on_a_fuzz_set_and_is_deterministic(tmp_path):
    import evaluate
    data = write_fuzz_set(str(tmp_path / 'fz'))
    host, dev = _compare_paths(data, 'fz')
    assert len(host.users) > 10 and len(host.users) < 30 and host.tcount > len(host.users)
    u8 = list(host.users).index(8)
    assert host.rated_ptr[u8 + 1] == host.rated_ptr[u8]                # the last line won
    again = evaluate.load_scenario(data, 0, 'fz', evaluate.read_ids(os.path.join(data, 'uid')), where='device')
    for name in NAMES:
        _same(getattr(again, name), getattr(dev, name), name)


def test_load_scenario_device_uploads_the_stamped_copies(tmp_path, monkeypatch):
    import textio
    monkeypatch.delenv('TKR_NO_CACHE', raising=False)
    data = write_fuzz_set(str(tmp_path / 'fz'), seed=1)
    parsed = dict(textio.parse_counts)
    _compare_paths(data, 'fz')                                         # the host path parses and leaves the copies
    assert os.path.exists(os.path.join(data, 'f0tr.txt.csr.npz')) and os.path.exists(os.path.join(data, 'f0te.fz.txt.csr.npz'))
    assert textio.parse_counts == {'host': parsed['host'] + 2, 'device': parsed['device']}      # ... which the device path uploaded


@pytest.mark.parametrize('kind', range(3))
def test_the_three_key_errors_are_the_same_on_both_paths(tmp_path, kind):
    import evaluate
    extra = [('u1,i3:1,nothing:1',), ('nobody,i3:1',), ()][kind]
    data = write_fuzz_set(str(tmp_path / 'fz'), seed=2, extra_test_lines=extra, drop_train_of='u2' if kind == 2 else None)
    uids = evaluate.read_ids(os.path.join(data, 'uid'))
    raised = []
    for where in ('host', 'device'):
        with pytest.raises(KeyError) as e:
            evaluate.load_scenario(data, 0, 'fz', uids, where=where)
        raised.append(e.value.args)
    assert raised[0] == raised[1]
    assert ['likes an id', 'test user missing', 'without a line'][kind] in raised[0][0]


def test_auto_takes_the_device_from_the_threshold_upward(tmp_path, monkeypatch):
    import evaluate
    import textio
    data = write_fuzz_set(str(tmp_path / 'fz'), seed=3)
    uids = evaluate.read_ids(os.path.join(data, 'uid'))
    host = evaluate.load_scenario(data, 0, 'fz', uids, where='host')
    n = len(textio.parse_ratings(os.path.join(data, 'f0tr.txt'), uids, host.teids).item) + \
        len(textio.parse_ratings(os.path.join(data, 'f0te.fz.txt'), uids, host.teids).item)
    for threshold, path in ((n, 'device'), (n + 1, 'host')):
        monkeypatch.setenv('TKR_GROUP_DEVICE_FROM', str(threshold))
        before = dict(textio.group_counts)
        sc = evaluate.load_scenario(data, 0, 'fz', uids)
        assert textio.group_counts[path] == before[path] + 1 and sum(textio.group_counts.values()) == sum(before.values()) + 1
        for name in NAMES:
            _same(getattr(sc, name), getattr(host, name), name)


def test_rank_and_candidate_lines_device_equal_host(tmp_path):
    """rows that repeat a user, a user without a line, a second ratings file"""
    import evaluate
    import recommend
    import textio
    data = write_fuzz_set(str(tmp_path / 'fz'), seed=4, drop_train_of='u11')
    uids, vids = evaluate.read_ids(os.path.join(data, 'uid')), evaluate.read_ids(os.path.join(data, 'f0te.fz.idl'))
    umap, vmap = textio.IdMap(uids), textio.IdMap(vids)
    R = textio.parse_ratings(os.path.join(data, 'f0tr.txt'), umap, vmap)
    R2 = textio.parse_ratings(os.path.join(data, 'f0te.fz.txt'), umap, vmap)
    rng = np.random.Generator(np.random.PCG64(9))
    U = torch.from_numpy(rng.standard_normal((30, 8)).astype(np.float32)).cuda()
    V = torch.from_numpy(rng.standard_normal((40, 8)).astype(np.float32)).cuda()
    rows = [3, 3, 7, 0, 11, 29, 3, 11, 20, 10]
    cand = {}
    for where in ('host', 'device'):
        before = textio.group_counts[where]
        cand[where] = recommend.candidate_lines(os.path.join(data, 'f0te.fz.txt'), umap, vmap, 40, where=where)
        assert textio.group_counts[where] == before + 1
    for a, b in zip(cand['host'], cand['device']):
        _same(b, a)
    for also in (None, R2):
        for candidates in (None, (cand['host'][2][:len(rows) + 1], cand['host'][3][:cand['host'][2][len(rows)]])):
            out = {}
            for where in ('host', 'device'):
                before = textio.group_counts[where]
                out[where] = recommend.rank(U, rows, V, None, R, 10, also_rated=also, candidates=candidates, where=where)
                assert textio.group_counts[where] == before + 1
            _same(out['device'][0], out['host'][0], 'ids')
            _same(out['device'][1].view(np.int32), out['host'][1].view(np.int32), 'score bits')
    assert (out['host'][0] >= 0).any()


def test_cli_output_does_not_depend_on_where_the_rows_are_grouped(golden_dir, tmp_path, monkeypatch, capsys):
    import evaluate
    import recommend
    import textio
    d = os.path.join(golden_dir, 'g4')
    data, model = os.path.join(d, 'data'), os.path.join(d, 'model')
    printed = {}
    for where in ('host', 'device'):
        monkeypatch.setenv('TKR_GROUP', where)
        before = textio.group_counts[where]
        evaluate.main(['-d', data, '-m', model, '-sl', 'im', 'om', '-M', 'auc', 'ndcg', 'mrr', 'map', 'acc'])
        printed[where] = capsys.readouterr().out
        assert textio.group_counts[where] == before + 2
    assert printed['host'] == printed['device'] and printed['host'].count('\n') == 12
    monkeypatch.delenv('TKR_GROUP')
    written = {}
    for where in ('host', 'device'):
        out = str(tmp_path / (where + '.txt'))
        before = textio.group_counts[where]
        recommend.main(['-d', data, '-m', model, '-o', out, '-t', '10', '--group', where, '--candidates', os.path.join(data, 'f0te.im.txt')])
        assert textio.group_counts[where] == before + 2               # the candidates and the excluded items
        written[where] = open(out, 'rb').read()
        out = str(tmp_path / (where + '.all.txt'))
        recommend.main(['-d', data, '-m', model, '-o', out, '-t', '10', '--group', where])
        written[where] += open(out, 'rb').read()
    assert written['host'] == written['device'] and len(written['host']) > 1000
