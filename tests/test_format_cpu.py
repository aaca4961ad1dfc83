"""What of the device-side text writers (K13, csrc/format_dev.hip) can be checked without a GPU: the integer-only '%f' recipe against
Python's own, the declarations, argument validation of the C entry points (host-only calls), the `where` argument of
textio.write_lists / write_matrix and the host writer's bytes."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from _format_oracle import edge_bits, format_f32, python_f

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_INVAL = -1
I64, I32, PTR = ctypes.c_int64, ctypes.c_int32, ctypes.c_void_p
ENTRY_POINTS = ('tkr_lists_format_sizes_dev', 'tkr_lists_format_emit_dev', 'tkr_matrix_format_sizes_dev', 'tkr_matrix_format_emit_dev')


def test_integer_recipe_equals_python_percent_f():
    longest = 0
    for bits in edge_bits():
        assert format_f32(bits) == python_f(bits), hex(int(bits))
        longest = max(longest, len(format_f32(bits)))
    assert longest == 47 and format_f32(0xff7fffff) == '-' + '%d' % (0xffffff << 104) + '.000000'
    assert format_f32(0x80000000) == '-0.000000' and format_f32(0xb089705f) == '-0.000000' and format_f32(0xffc00000) == 'nan'
    rng = np.random.Generator(np.random.PCG64(0))
    bits = rng.integers(0, 1 << 32, 200000, dtype=np.uint64).astype(np.uint32)
    values = bits.view(np.float32)
    for b, x in zip(bits.tolist(), values.tolist()):
        assert format_f32(b) == ('nan' if x != x else '%f' % x), hex(b)


def test_header_binding_and_library_declare_the_writers():
    import tkr_hip
    header = open(os.path.join(ROOT, 'include', 'tkr.h')).read()
    declared = re.findall(r'^int(?:32_t|64_t)? (tkr_\w+)\(', header, flags=re.M)
    lib = ctypes.CDLL(tkr_hip.LIB_PATH)
    for name in ENTRY_POINTS:
        assert name in declared and name in tkr_hip.EXPORTS and getattr(lib, name)
    assert 'recommend.py:50-56' in header and 'csrc/textio.hip:263-283' in header      # the call sites they replace
    assert lib.tkr_version() == tkr_hip.VERSION


def test_entry_points_check_their_arguments_before_any_device_access():
    """host-only calls: every pointer below is either NULL or an address nothing may touch"""
    import tkr_hip
    lib = tkr_hip.lib()
    fake = 1 << 12                                                   # aligned, never dereferenced

    def lists(emit, **kw):
        a = dict(ids=fake, scores=fake, row_user=fake, n=10, K=3, ub=fake, ubl=5, us=fake, ul=fake, nu=4, vb=fake, vbl=5, vs=fake, vl=fake, nv=4,
                 line_ptr=fake, totals=fake, first=0, count=10, out=fake, out_bytes=100, status=fake)
        a.update(kw)
        head = (PTR(a['ids']), PTR(a['scores']), PTR(a['row_user']), I64(a['n']), I32(a['K']), PTR(a['ub']), I64(a['ubl']), PTR(a['us']),
                PTR(a['ul']), I64(a['nu']), PTR(a['vb']), I64(a['vbl']), PTR(a['vs']), PTR(a['vl']), I64(a['nv']), PTR(a['line_ptr']))
        if emit:
            return lib.tkr_lists_format_emit_dev(*head, I64(a['first']), I64(a['count']), PTR(a['out']), I64(a['out_bytes']), PTR(a['status']), None)
        return lib.tkr_lists_format_sizes_dev(*head, PTR(a['totals']), None)

    shared = (dict(ids=None), dict(scores=None), dict(row_user=None), dict(n=-1), dict(K=-1), dict(ub=None), dict(vb=None), dict(ubl=-1),
              dict(vbl=-1), dict(ubl=(1 << 29) + 1), dict(us=None), dict(ul=None), dict(vs=None), dict(vl=None), dict(nu=-1), dict(nv=-1),
              dict(line_ptr=None))
    for bad in shared + (dict(totals=None),):
        assert lists(False, **bad) == E_INVAL, bad
    for bad in shared + (dict(status=None), dict(out=None), dict(out=fake + 8), dict(out_bytes=-1), dict(first=-1), dict(count=-1),
                         dict(first=11), dict(first=5, count=6)):
        assert lists(True, **bad) == E_INVAL, bad

    def matrix(emit, **kw):
        a = dict(data=fake, rows=10, cols=3, line_ptr=fake, totals=fake, first=0, count=10, out=fake, out_bytes=100, status=fake)
        a.update(kw)
        if emit:
            return lib.tkr_matrix_format_emit_dev(PTR(a['data']), I64(a['rows']), I64(a['cols']), PTR(a['line_ptr']), I64(a['first']),
                                                  I64(a['count']), PTR(a['out']), I64(a['out_bytes']), PTR(a['status']), None)
        return lib.tkr_matrix_format_sizes_dev(PTR(a['data']), I64(a['rows']), I64(a['cols']), PTR(a['line_ptr']), PTR(a['totals']), None)

    shared = (dict(data=None), dict(rows=-1), dict(cols=-1), dict(line_ptr=None))
    for bad in shared + (dict(totals=None),):
        assert matrix(False, **bad) == E_INVAL, bad
    for bad in shared + (dict(status=None), dict(out=None), dict(out=fake + 4), dict(out_bytes=-1), dict(first=-1), dict(count=-1),
                         dict(first=11), dict(first=1, count=10)):
        assert matrix(True, **bad) == E_INVAL, bad


def _lists():
    import textio
    users = textio.IdMap({'u1': 0, '77': 1, 'x': 2, '': 5})
    items = textio.IdMap({'a': 0, 'b': 1, 'c10': 10})
    ids = np.array([[10, 0, 1], [-1, 1, -1], [-1, -1, -1], [0, -1, 10]], dtype=np.int32)
    scores = np.array([[1.5, 0.25, -0.125], [9.0, 0.0, 9.0], [1.0, 2.0, 3.0], [-0.0, 7.0, np.inf]], dtype=np.float32)
    row_user = np.array([0, 1, 2, 5], dtype=np.int32)
    want = ['u1,c10:1.500000,a:0.250000,b:-0.125000', '77,b:0.000000', 'x', ',a:-0.000000,c10:inf']
    return users, items, ids, scores, row_user, want


def test_where_argument_and_host_writer(tmp_path, monkeypatch):
    import recommend
    import textio
    import tkr_hip
    monkeypatch.delenv('TKR_FORMAT', raising=False)
    monkeypatch.delenv('TKR_FORMAT_DEVICE_FROM', raising=False)
    users, items, ids, scores, row_user, want = _lists()
    assert recommend.format_lines is textio.format_lines
    assert textio.format_lines(['u1', '77', 'x', ''], ids, scores, items.tokens_by_index()) == want
    path = str(tmp_path / 'lists.txt')
    mat = np.arange(12, dtype=np.float32).reshape(3, 4) / 8
    for call in (lambda **kw: textio.write_lists(path, users, ids, scores, row_user, items, **kw), lambda **kw: textio.write_matrix(path, mat, **kw)):
        with pytest.raises(ValueError, match='TKR_FORMAT'):
            call(where='x')
        monkeypatch.setenv('TKR_FORMAT', 'x')
        with pytest.raises(ValueError, match='TKR_FORMAT'):
            call()
        monkeypatch.delenv('TKR_FORMAT')
    assert textio.FORMAT_DEFAULT in textio.FORMAT_WHERE and textio.FORMAT_DEVICE_FROM >= 65536
    text = ('\n'.join(want) + '\n').encode()
    before = dict(textio.format_counts)
    assert textio.write_lists(path, users, ids, scores, row_user, items, where='host') == len(text)
    assert open(path, 'rb').read() == text
    textio.write_lists(path, users, ids, scores, row_user, items)                # 12 fields: 'auto' is the host writer, GPU or not
    assert open(path, 'rb').read() == text
    monkeypatch.setenv('TKR_FORMAT', 'host')
    assert textio.write_lists(path, users, ids[:2], scores[:2], row_user[:2], items, append=True) == len('\n'.join(want[:2])) + 1
    monkeypatch.delenv('TKR_FORMAT')
    assert open(path, 'rb').read() == text + ('\n'.join(want[:2]) + '\n').encode()
    assert textio.write_lists(path, users, ids[:0], scores[:0], row_user[:0], items, where='host') == 0 and open(path, 'rb').read() == b''
    assert textio.format_counts == dict(before, host=before['host'] + 4)
    mpath = str(tmp_path / 'm.dat')
    textio.write_matrix(mpath, mat, where='host')
    host = open(mpath, 'rb').read()
    assert host == ''.join(''.join('%f ' % v for v in row) + '\n' for row in mat).encode()
    textio.write_matrix(mpath, mat)
    assert open(mpath, 'rb').read() == host and textio.format_counts == dict(before, host=before['host'] + 6)
    if not torch.cuda.is_available():
        with pytest.raises(tkr_hip.TkrError, match='MI355X'):
            textio.write_lists(path, users, ids, scores, row_user, items, where='device')
        with pytest.raises(tkr_hip.TkrError, match='MI355X'):
            textio.write_matrix(mpath, mat, where='device')
        with pytest.raises(tkr_hip.TkrError, match='MI355X'):
            textio.format_lists_device(ids, scores, row_user, users, items)
        monkeypatch.setenv('TKR_FORMAT_DEVICE_FROM', '1')                        # 'auto' without a GPU is the host at any size
        textio.write_lists(path, users, ids, scores, row_user, items, where='auto')
        textio.write_matrix(mpath, mat, where='auto')
        assert open(path, 'rb').read() == text and open(mpath, 'rb').read() == host
        assert textio.format_counts == dict(before, host=before['host'] + 8)


def test_token_table_by_index():
    """IdMap.device_tokens lays the tokens out by index on the host: checked here through the arrays it uploads"""
    import textio
    table = {'b': 3, '': 0, 'héé': 6, 'late': 3, 'neg': -2, 'x' * 40: 1}
    m = textio.IdMap(table)
    assert m.tokens_by_index() == {3: 'late', 0: '', 6: 'héé', -2: 'neg', 1: 'x' * 40}
    if torch.cuda.is_available():
        blob, blob_len, start, length = m.device_tokens('cuda')
        blob, start, length = bytes(blob.cpu().numpy()), start.cpu().numpy(), length.cpu().numpy()
        assert blob_len == len('\n'.join(table).encode()) and length.tolist() == [0, 40, -1, 4, -1, -1, 5]
        for idx, tok in m.tokens_by_index().items():
            if idx >= 0:
                assert blob[start[idx]:start[idx] + length[idx]].decode() == tok
