"""K11 (csrc/parse_dev.hip): the ratings parser on the device against the host parser (textio.parse_ratings(where='host')) and a
per-field Python restatement of the reference's loops -- exact equality of all four arrays, at chunk sizes that put every boundary
case into files of a few KB."""
import json
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

I32_MAX = 2147483647


def _py_ratings(path, users, items):
    """per-field restatement of the three reference parsers' common core on the file's BYTES: '\\n' alone ends a line (a last line
    without one counts), bytes.strip() takes exactly the six ASCII whitespace bytes"""
    data = open(path, 'rb').read()
    lines = data.split(b'\n')
    if lines[-1] == b'':
        lines.pop()
    line_user, line_ptr, item, like = [], [0], [], []
    for line in lines:
        terms = line.strip().split(b',')
        line_user.append(users.get(terms[0].decode(), -1))
        for t in terms[1:]:
            item.append(items.get(t.split(b':')[0].decode(), -1))
            like.append(max(-I32_MAX, min(I32_MAX, int(t.split(b':')[1]))))
        line_ptr.append(len(item))
    return line_user, line_ptr, item, like


DTYPES = dict(line_user=np.int32, line_ptr=np.int64, item=np.int32, like=np.int32)


def _check_file(path, users, items, chunks=(64, None), python=True):
    """device == host == Python on `path`, at every chunk size asked for (None = the default); -> the host Ratings"""
    import textio
    path = str(path)
    um, vm = textio.IdMap(users), textio.IdMap(items)
    host = textio.parse_ratings(path, um, vm, where='host')
    if python:
        for name, want in zip(DTYPES, _py_ratings(path, users, items)):
            assert getattr(host, name).tolist() == want, name
    for cb in chunks:
        dev = textio.parse_ratings_device(path, um, vm, chunk_bytes=cb)
        assert all(getattr(dev, name).is_cuda for name in DTYPES)
        got = dev.host()
        for name, dtype in DTYPES.items():
            a, b = getattr(got, name), getattr(host, name)
            assert a.dtype == dtype and a.shape == b.shape and np.array_equal(a, b), (name, cb)
    return host


def _raises(fn):
    import textio
    try:
        fn()
    except textio.TextFormatError:
        return True
    return False


def test_goldens_and_the_odd_file(golden_dir, tmp_path):
    from oracle import ref_np as R
    cases = [(os.path.join(golden_dir, 'g1', 'tr.txt'), os.path.join(golden_dir, 'g1', 'uid'), os.path.join(golden_dir, 'g1', 'vid')),
             (os.path.join(golden_dir, 'g4', 'data', 'f0tr.txt'), os.path.join(golden_dir, 'g4', 'data', 'uid'),
              os.path.join(golden_dir, 'g4', 'data', 'f0te.om.idl')),
             (os.path.join(golden_dir, 'g7', 'data', 'f0te.sm.txt'), os.path.join(golden_dir, 'g7', 'data', 'uid'),
              os.path.join(golden_dir, 'g7', 'data', 'f0te.sm.idl'))]
    odd = tmp_path / 'odd.txt'                      # CRLF, blank line, spaces, no trailing newline, like with sign, extra ':' part
    odd.write_bytes(b'u1,a:1,b:0\r\n\n  u2,c: 1 ,a:+1:zz,\tq:-3\nu3\nzz,a:1\n u1 ,b:01')
    (tmp_path / 'u').write_text('u1\nu2\nu3\n')
    (tmp_path / 'v').write_text('a\nb\nc\n')
    cases.append((str(odd), str(tmp_path / 'u'), str(tmp_path / 'v')))
    for path, upath, vpath in cases:
        got = _check_file(path, R.read_id_list(upath), R.read_id_list(vpath))
        assert len(got.line_user) > 0
    assert got.like.tolist() == [1, 0, 1, 1, -3, 1, 1] and got.line_user.tolist() == [0, -1, 1, 2, -1, -1]


def test_fuzz(tmp_path):
    """the generator of test_native_ratings_parser_fuzz with its own seed"""
    rng = np.random.Generator(np.random.PCG64(20240611))
    users = {'u%d' % x: x for x in range(40)}
    items = {'i%d' % x: x for x in range(60)}
    items['odd id'] = 60
    for trial in range(26):
        lines = []
        for _ in range(int(rng.integers(0, 30))):
            uid = rng.choice(['u%d' % rng.integers(0, 50), ' u%d' % rng.integers(0, 40), ''])
            fields = []
            for _ in range(int(rng.integers(0, 12))):
                iid = rng.choice(['i%d' % rng.integers(0, 70), 'odd id', 'i%d ' % rng.integers(0, 60)])
                like = rng.choice(['0', '1', '+1', '-1', ' 1', '1 ', '01', '5', '1:extra', '0:1'])
                fields.append('%s:%s' % (iid, like))
            lines.append(','.join([uid] + fields) + rng.choice(['\n', '\r\n', ' \n', '\t\n']))
        text = ''.join(lines)
        if trial % 3 == 0:
            text = text.rstrip('\r\n\t ')
        path = tmp_path / ('f%d.txt' % trial)
        path.write_bytes(text.encode())
        _check_file(path, users, items, chunks=(64, 256))


USERS = {'u' + 'x' * k: k for k in range(64)}
ITEMS = {'a': 0, 'b': 1, 'i7': 7}


def _place(data, delim, target):
    """data + one line "u<pad>,a:1\\n" whose `delim` byte lands at an offset = target (mod 64)"""
    at = {b',': 0, b':': 2, b'\n': 4}[delim]                      # offset of the delimiter behind the uid token
    n = (target - len(data) - at) % 64 or 64                      # length of the uid token
    line = b'u' + b'x' * (n - 1) + b',a:1\n'
    assert (len(data) + line.index(delim)) % 64 == target
    return data + line


def test_chunk_boundaries(tmp_path):
    """chunk_bytes = 64: lines and fields that straddle many chunks, chunks without a delimiter, delimiters on the first and the
    last byte of a chunk, lengths around a multiple of the chunk, the smallest files"""
    long_uid, long_iid = 'U' * 200, 'I' * 200
    users = dict(USERS, **{long_uid: 900})
    items = dict(ITEMS, **{long_iid: 901})
    files = {}
    files['fields3000'] = ('u,' + ','.join('%s:%d' % (('a', 'b', 'i7', 'zz')[k % 4], k % 3) for k in range(3000)) + '\n').encode()
    files['long_tokens'] = ('%s,%s:1,a:0\nux,%s:1\n%s\n' % (long_uid, long_iid, long_iid[:-1], long_uid)).encode()       # > 3 chunks without ','
    files['no_newline_chunks'] = ('ux' + ',a:1' * 60).encode()    # 242 bytes, not one '\n'
    files['no_comma_chunks'] = ('u' + 'x' * 40 + '\n') * 8 + 'q' * 300 + '\nux,a:1\n'
    files['no_comma_chunks'] = files['no_comma_chunks'].encode()
    for name, target in (('first_byte', 0), ('last_byte', 63)):
        data = b'ux,b:0\n'
        for delim in (b'\n', b',', b':'):
            data = _place(data, delim, target)
            data = _place(data, delim, target)
        for delim in (b'\n', b',', b':'):
            assert any(data[o:o + 1] == delim for o in range(target, len(data), 64)), (name, delim)
        files[name] = data
    body = b'ux,a:1,b:0\n' * 11                                    # 121 bytes
    files['multiple'] = body + b'uxxxxxx'                          # 128 = 2 chunks, no final newline
    files['multiple_nl'] = body + b'uxxxxx\n'                      # 128, '\n' on the last byte of the file and of a chunk
    files['multiple_plus_1'] = body + b'uxxxxxx\n'                 # 129: the '\n' alone in a third chunk
    files['multiple_plus_1_comma'] = body + b'uxxxx,a:1'           # 130: ends mid-line
    assert len(files['multiple']) == 128 and len(files['multiple_nl']) == 128 and len(files['multiple_plus_1']) == 129
    files['only_newlines'] = b'\n' * 130
    files['one_byte'] = b'u'
    files['one_newline'] = b'\n'
    files['one_space'] = b' '
    files['empty'] = b''
    for name, data in files.items():
        path = tmp_path / (name + '.txt')
        path.write_bytes(data)
        got = _check_file(path, users, items, chunks=(64,))
        assert got.line_ptr[-1] == len(got.item) == data.count(b','), name
    import textio
    got = textio.parse_ratings_device(str(tmp_path / 'empty.txt'), users, items, chunk_bytes=64).host()
    assert len(got.line_user) == 0 and got.line_ptr.tolist() == [0]
    got = textio.parse_ratings_device(str(tmp_path / 'long_tokens.txt'), users, items, chunk_bytes=64).host()
    assert got.line_user.tolist() == [900, 1, 900] and got.item.tolist() == [901, 0, -1]


def test_three_default_chunks(tmp_path):
    import textio
    rng = np.random.Generator(np.random.PCG64(5))
    users = {'u%d' % x: x for x in range(500)}
    items = {'i%d' % x: x for x in range(800)}
    lines = []
    for u in rng.permutation(520):
        lines.append('u%d' % u + ''.join(',i%d:%d' % (i, rng.integers(0, 2)) for i in rng.integers(0, 830, int(rng.integers(0, 40)))))
    path = tmp_path / 'big.txt'
    path.write_text('\n'.join(lines) + '\n')
    assert os.path.getsize(str(path)) >= 3 * textio.PARSE_CHUNK_BYTES + 1000
    got = _check_file(path, users, items, chunks=(None, 64))
    assert (got.item == -1).any() and (got.line_user == -1).any() and (got.item >= 0).any()


def test_lookup(tmp_path):
    """5,000 tokens with indices that are not their line numbers; '', prefixes of each other, inner and trailing spaces, absent ones"""
    tokens = ['', '1', '11', '111', 'odd id', 'trail ', ' lead', 'a  b', 'x' * 60] + ['t%d' % k for k in range(4991)]
    table = {t: 3 * k + 7 + (k % 5) for k, t in enumerate(tokens)}                     # gaps, as duplicate id lines produce
    assert len(table) == 5000
    rng = np.random.Generator(np.random.PCG64(8))
    absent = ['1111', '2', 't4991', 'T1', 'odd  id', 'trail', 'x' * 59, 'x' * 61, 't', 't 1']
    pool = tokens + absent
    lines = []
    for _ in range(300):
        uid = pool[int(rng.integers(0, len(pool)))]
        fields = ['%s:%d' % (pool[int(rng.integers(0, len(pool)))], rng.integers(0, 2)) for _ in range(int(rng.integers(0, 20)))]
        lines.append(','.join([uid] + fields))
    lines += [',:1,1:0,11:1,111:1,1111:1', '1 ,trail :1, lead:0', '11', '']
    path = tmp_path / 'lookup.txt'
    path.write_text('\n'.join(lines) + '\n')
    got = _check_file(path, table, table, chunks=(64, None))
    n = len(got.line_user)
    assert got.line_user[n - 4:].tolist() == [table[''], -1, table['11'], table['']]
    assert got.item[got.line_ptr[n - 4]:got.line_ptr[n - 3]].tolist() == [table[''], table['1'], table['11'], table['111'], -1]
    assert got.item[got.line_ptr[n - 3]:got.line_ptr[n - 2]].tolist() == [table['trail '], table[' lead']]


def test_errors(tmp_path):
    import textio
    users, items = {'u1': 0}, {'a': 0}
    bad = tmp_path / 'bad.txt'

    def both(data):
        bad.write_bytes(data)
        host = _raises(lambda: textio.parse_ratings(str(bad), users, items, where='host'))
        dev = [_raises(lambda: textio.parse_ratings_device(str(bad), users, items, chunk_bytes=cb)) for cb in (64, None)]
        assert dev == [host, host], data
        return host

    # a field without ':', a like that is no integer, an empty like, an empty field raise; a third part behind the like does not
    for text, want in (('u1,a', True), ('u1,a:x', True), ('u1,a:', True), ('u1,a:1,', True), ('u1,a:1:', False)):
        for tail in ('', '\n', '\r\n', '\nu1,a:1\n'):
            assert both((text + tail).encode()) == want, (text, tail)
    for text in ('u1,a:+', 'u1,a:-', 'u1,a:1 2', 'u1,a:1.0', 'u1,a::1', 'u1,,a:1', 'u1,a:99999999999', 'u1,a:-99999999999', 'u1,a: \t7\r'):
        both(text.encode())
    full = b'u1,a:1,b:0\nu1,a: 1 ,zz:-3:q\n' * 3 + b'u1,a:1,b:12'
    raised = [both(full[:n]) for n in range(len(full) - 14, len(full) + 1)]              # the file's last bytes cut mid-field
    assert True in raised and False in raised
    # the smallest offending offset does not matter to the caller, only that it raises; a later parse in the same process works
    bad.write_bytes(full)
    got = textio.parse_ratings_device(str(bad), users, items, chunk_bytes=64).host()
    assert got.like.tolist() == [1, 0, 1, -3] * 3 + [1, 12] and got.item.tolist() == [0, -1, 0, -1] * 3 + [0, -1]
    got = textio.parse_ratings(str(bad), users, items, where='device')
    assert got.like.tolist() == [1, 0, 1, -3] * 3 + [1, 12]
    with pytest.raises(OSError):
        textio.parse_ratings_device(str(tmp_path / 'missing.txt'), users, items)
    with pytest.raises(OSError):
        textio.parse_ratings(str(tmp_path / 'missing.txt'), users, items, where='device')
    with pytest.raises(ValueError):
        textio.parse_ratings_device(str(bad), users, items, chunk_bytes=96)


def test_saturation_and_wide_likes(tmp_path):
    path = tmp_path / 'sat.txt'
    path.write_text('u1,a:2147483647,a:2147483648,a:-2147483648,a:000000000000000000012,a:99999999999999999999999999,a:-0\n')
    got = _check_file(path, {'u1': 0}, {'a': 0})
    assert got.like.tolist() == [I32_MAX, I32_MAX, -I32_MAX, 12, I32_MAX, 0]


def test_load_training_data_through_the_device_parser(golden_dir, monkeypatch):
    import textio
    from single import BPR
    monkeypatch.setenv('TKR_PARSE', 'device')
    monkeypatch.setenv('TKR_PARSE_DEVICE_FROM', '0')
    d = os.path.join(golden_dir, 'g1')
    exp = json.load(open(os.path.join(d, 'expected.json')))
    before = dict(textio.parse_counts)
    m = BPR(k=4)
    m.load_training_data(os.path.join(d, 'uid'), os.path.join(d, 'vid'), os.path.join(d, 'tr.txt'), data_copy=True)
    assert textio.parse_counts['device'] == before['device'] + 1 and textio.parse_counts['host'] == before['host']
    assert [list(p) for p in m.data] == exp['data']
    assert {str(k): list(v) for k, v in m.tr_data.items()} == exp['tr_data']
    assert m.tr_users == exp['tr_users'] and m.epoch_sample_limit == exp['epoch_sample_limit']


def test_stamped_copy_after_a_device_parse(tmp_path, monkeypatch):
    import textio
    monkeypatch.setenv('TKR_NO_CACHE', '0')
    path = tmp_path / 'f0tr.txt'
    path.write_text('u1,a:1,b:0\nu2,b:1\nu9,a:1\n')
    users, items = {'u1': 0, 'u2': 1}, {'a': 0, 'b': 1}
    first = textio.parse_ratings(str(path), users, items, where='device')
    assert os.path.exists(str(path) + '.csr.npz')
    before = dict(textio.parse_counts)
    for where in ('device', 'host', 'auto'):
        again = textio.parse_ratings(str(path), users, items, where=where)
        for name in DTYPES:
            np.testing.assert_array_equal(getattr(first, name), getattr(again, name))
            assert getattr(again, name).dtype == DTYPES[name]
    assert textio.parse_counts == before                            # all three were served from the copy
    assert first.line_user.tolist() == [0, 1, -1] and first.item.tolist() == [0, 1, 1, 0] and first.like.tolist() == [1, 0, 1, 1]


def test_auto_takes_the_host_for_small_files_and_the_device_above_the_threshold(golden_dir, monkeypatch):
    import textio
    from oracle import ref_np as R
    d = os.path.join(golden_dir, 'g1')
    users, items = R.read_id_list(os.path.join(d, 'uid')), R.read_id_list(os.path.join(d, 'vid'))
    monkeypatch.delenv('TKR_PARSE_DEVICE_FROM', raising=False)
    assert textio.PARSE_DEVICE_FROM >= 64 << 20
    before = dict(textio.parse_counts)
    small = textio.parse_ratings(os.path.join(d, 'tr.txt'), users, items, where='auto')
    assert textio.parse_counts == dict(before, host=before['host'] + 1)
    monkeypatch.setenv('TKR_PARSE_DEVICE_FROM', '0')
    above = textio.parse_ratings(os.path.join(d, 'tr.txt'), users, items, where='auto')
    assert textio.parse_counts == dict(before, host=before['host'] + 1, device=before['device'] + 1)
    for name in DTYPES:
        np.testing.assert_array_equal(getattr(small, name), getattr(above, name))
