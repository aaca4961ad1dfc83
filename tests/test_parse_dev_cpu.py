"""What of the device-side ratings parser (K11, csrc/parse_dev.hip) can be checked without a GPU: the `where` argument of
textio.parse_ratings, argument validation of the new C entry points (host-only calls), and the id table the host lays out for
the kernels against a pure-Python lookup."""
import ctypes
import os

import numpy as np
import pytest
import torch

E_INVAL = -1
I64, PTR = ctypes.c_int64, ctypes.c_void_p


def test_where_argument(golden_dir, monkeypatch):
    import textio
    import tkr_hip
    from oracle import ref_np as R
    d = os.path.join(golden_dir, 'g1')
    users, items = R.read_id_list(os.path.join(d, 'uid')), R.read_id_list(os.path.join(d, 'vid'))
    path = os.path.join(d, 'tr.txt')
    with pytest.raises(ValueError):
        textio.parse_ratings(path, users, items, where='bogus')
    monkeypatch.setenv('TKR_PARSE', 'bogus')
    with pytest.raises(ValueError):
        textio.parse_ratings(path, users, items)
    monkeypatch.setenv('TKR_PARSE', 'host')
    by_env = textio.parse_ratings(path, users, items)
    monkeypatch.delenv('TKR_PARSE')
    monkeypatch.delenv('TKR_PARSE_DEVICE_FROM', raising=False)
    assert textio.PARSE_DEFAULT in textio.PARSE_WHERE and textio.PARSE_DEVICE_FROM >= 64 << 20
    before = dict(textio.parse_counts)
    host = textio.parse_ratings(path, users, items, where='host')
    auto = textio.parse_ratings(path, users, items, where='auto')
    default = textio.parse_ratings(path, users, items)
    assert textio.parse_counts == dict(before, host=before['host'] + 3)          # a file of a few hundred bytes: the host parser, GPU or not
    for name in ('line_user', 'line_ptr', 'item', 'like'):
        for other in (auto, default, by_env):
            np.testing.assert_array_equal(getattr(host, name), getattr(other, name))
    if not torch.cuda.is_available():
        with pytest.raises(tkr_hip.TkrError, match='MI355X'):
            textio.parse_ratings(path, users, items, where='device')
        with pytest.raises(tkr_hip.TkrError, match='MI355X'):
            textio.parse_ratings_device(path, users, items)
        monkeypatch.setenv('TKR_PARSE_DEVICE_FROM', '0')                         # 'auto' without a GPU is the host at any size
        np.testing.assert_array_equal(textio.parse_ratings(path, users, items, where='auto').item, host.item)


def test_entry_points_check_their_arguments_before_any_device_access():
    """host-only calls: every pointer below is either NULL or an address nothing may touch"""
    import tkr_hip
    lib = tkr_hip.lib()
    assert lib.tkr_parse_dev_workspace_bytes(I64(1000), I64(64)) > 0
    assert lib.tkr_parse_dev_workspace_bytes(I64(0), I64(64)) > 0
    assert lib.tkr_parse_dev_workspace_bytes(I64(1 << 40), I64(1 << 20)) > 24 * (1 << 20)
    for chunk in (0, 1, 32, 63, 96, 100, (1 << 20) + 1, 1 << 21, -64):
        assert lib.tkr_parse_dev_workspace_bytes(I64(1000), I64(chunk)) == E_INVAL, chunk
    assert lib.tkr_parse_dev_workspace_bytes(I64(-1), I64(64)) == E_INVAL
    assert lib.tkr_parse_dev_workspace_bytes(I64(1 << 40), I64(64)) == E_INVAL          # more chunks than one launch takes
    assert lib.tkr_idtable_slots(I64(-1)) == E_INVAL
    assert [lib.tkr_idtable_slots(I64(n)) for n in (0, 1, 4, 5, 1000)] == [8, 8, 8, 16, 2048]
    with pytest.raises(ValueError):
        tkr_hip.parse_dev_workspace_bytes(1000, 96)

    fake = 1 << 12                                                   # aligned, never dereferenced
    ws = lib.tkr_parse_dev_workspace_bytes(I64(1000), I64(64))

    def count(text=fake, n=1000, chunk=64, work=fake, work_bytes=ws, totals=fake):
        return lib.tkr_ratings_count_dev(PTR(text), I64(n), I64(chunk), PTR(work), I64(work_bytes), PTR(totals), None)

    for bad in (dict(text=None), dict(work=None), dict(totals=None), dict(n=-1), dict(chunk=96), dict(chunk=32), dict(chunk=1 << 21),
                dict(text=fake + 4), dict(work=fake + 8), dict(work_bytes=ws - 1), dict(work_bytes=0)):
        assert count(**bad) == E_INVAL, bad

    def emit(**kw):
        a = dict(text=fake, n=1000, chunk=64, work=fake, work_bytes=ws, n_lines=10, n_entries=100, us=fake, uns=8, ub=fake, ubl=5, vs=fake,
                 vns=8, vb=fake, vbl=5, line_start=fake, line_user=fake, line_ptr=fake, item=fake, like=fake, status=fake)
        a.update(kw)
        return lib.tkr_ratings_emit_dev(PTR(a['text']), I64(a['n']), I64(a['chunk']), PTR(a['work']), I64(a['work_bytes']), I64(a['n_lines']),
                                        I64(a['n_entries']), PTR(a['us']), I64(a['uns']), PTR(a['ub']), I64(a['ubl']), PTR(a['vs']), I64(a['vns']),
                                        PTR(a['vb']), I64(a['vbl']), PTR(a['line_start']), PTR(a['line_user']), PTR(a['line_ptr']), PTR(a['item']),
                                        PTR(a['like']), PTR(a['status']), None)

    for bad in (dict(text=None), dict(work=None), dict(n=-1), dict(chunk=96), dict(chunk=32), dict(work_bytes=ws - 1), dict(n_lines=-1),
                dict(n_entries=-1), dict(n_lines=1001), dict(n_entries=1001), dict(us=None), dict(vs=None), dict(uns=12), dict(vns=0),
                dict(ub=None), dict(vb=None), dict(ubl=-1), dict(vbl=1 << 31), dict(line_start=None), dict(line_user=None), dict(line_ptr=None),
                dict(item=None), dict(like=None), dict(status=None), dict(us=fake + 4), dict(vb=fake + 1)):
        assert emit(**bad) == E_INVAL, bad

    slots = np.zeros((8, 4), np.int32)
    index = np.zeros(2, np.int32)

    def build(blob=b'a\nb', blob_len=3, idx=index.ctypes.data, n=2, out=slots.ctypes.data, n_slots=8):
        return lib.tkr_idtable_build(blob, I64(blob_len), PTR(idx), I64(n), PTR(out), I64(n_slots))

    assert build() == 0
    for bad in (dict(out=None), dict(n=-1), dict(blob_len=-1), dict(blob=None), dict(idx=None), dict(n_slots=7), dict(n_slots=4), dict(n=5),
                dict(n=3), dict(blob_len=1 << 31)):
        assert build(**bad) == E_INVAL, bad


def _py_hash(token):
    h = 2166136261
    for byte in token:
        h = ((h ^ byte) * 16777619) & 0xffffffff
    return h ^ (h >> 15)


def _py_lookup(slots, blob, token):
    """open addressing with linear probing over slots of {offset, length (-1 = empty), index, hash} (include/tkr.h)"""
    h, mask = _py_hash(token), len(slots) - 1
    s = h & mask
    for _ in range(len(slots)):
        off, length, index, stored = (int(v) for v in slots[s])
        if length < 0:
            return -1
        if stored & 0xffffffff == h and blob[off:off + length] == token:
            return index
        s = (s + 1) & mask
    return -1


def test_id_table_layout_against_a_python_lookup():
    import textio
    import tkr_hip
    tokens = ['', '1', '11', '111', 'odd id', 'trail ', ' lead', 'x' * 300] + ['t%d' % k for k in range(4992)]
    table = {t: 2 * k + 3 for k, t in enumerate(tokens)}
    m = textio.IdMap(table)
    slots = tkr_hip.idtable_build(m._blob, m._index)
    assert slots.dtype == np.int32 and slots.shape == (16384, 4) and int((slots[:, 1] >= 0).sum()) == 5000
    for t, want in table.items():
        assert _py_lookup(slots, m._blob, t.encode()) == want, t
    for t in ('1111', 't4992', 'trail', 'lead', ' ', 'x' * 299, 'T1'):
        assert _py_lookup(slots, m._blob, t.encode()) == -1, t
    # the smallest tables: no key at all, and '' alone (the same empty blob, told apart by n)
    none = tkr_hip.idtable_build(b'', np.zeros(0, np.int32))
    assert none.shape == (8, 4) and (none[:, 1] == -1).all() and _py_lookup(none, b'', b'') == -1
    only = tkr_hip.idtable_build(b'', np.array([41], np.int32))
    assert _py_lookup(only, b'', b'') == 41 and _py_lookup(only, b'', b'a') == -1
    # a token listed twice keeps its last index, as tkr_idmap_create does
    twice = tkr_hip.idtable_build(b'a\nb\na', np.array([1, 2, 3], np.int32))
    assert _py_lookup(twice, b'a\nb\na', b'a') == 3 and _py_lookup(twice, b'a\nb\na', b'b') == 2 and int((twice[:, 1] >= 0).sum()) == 2
