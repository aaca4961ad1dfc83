"""K14 (csrc/scan_dev.hip) on the GPU: textio.read_matrix(where='device') and read_matrix_device against the host reader
tkr_matrix_read.  Every comparison is byte equality of the fp32 array, or the same TextFormatError."""
import os

import numpy as np
import pytest
import torch

from _format_oracle import edge_bits

pytestmark = pytest.mark.gpu


def _outcome(path, where):
    import textio
    try:
        a = textio.read_matrix(path, where=where)
    except textio.TextFormatError as e:
        assert not isinstance(e, textio.MatrixNotCanonical)          # read_matrix never lets that one out
        return 'TextFormatError'
    assert a.dtype == np.float32 and a.ndim == 2
    return a.shape, a.tobytes()


def _same(path, canonical=True, chunks=(64, None)):
    """the host reader's outcome (the array's shape and bytes, or TextFormatError) is the device path's; a canonical file is also
    read by read_matrix_device at every chunk size of `chunks` into a CUDA fp32 tensor of the same bytes, any other file makes
    it raise MatrixNotCanonical.  -> the outcome"""
    import textio
    assert os.environ.get('TKR_NO_CACHE') == '1'
    before = dict(textio.scan_counts)
    want = _outcome(path, 'host')
    got = _outcome(path, 'device')
    assert got == want
    if want != 'TextFormatError':                                   # counted under the reader that produced the array
        assert textio.scan_counts == dict(host=before['host'] + (1 if canonical else 2), device=before['device'] + (1 if canonical else 0))
    for chunk in chunks:
        if not canonical:
            with pytest.raises(textio.MatrixNotCanonical):
                textio.read_matrix_device(path, chunk_bytes=chunk)
        elif want == 'TextFormatError':
            with pytest.raises(textio.TextFormatError) as info:
                textio.read_matrix_device(path, chunk_bytes=chunk)
            assert not isinstance(info.value, textio.MatrixNotCanonical)
        else:
            t = textio.read_matrix_device(path, chunk_bytes=chunk)
            assert t.is_cuda and t.dtype == torch.float32 and tuple(t.shape) == want[0]
            assert t.cpu().numpy().tobytes() == want[1]
    return want


def _file(tmp_path, text, name='m.dat'):
    path = str(tmp_path / name)
    with open(path, 'wb') as fh:
        fh.write(text if isinstance(text, bytes) else text.encode())
    return path


HARD_ROUNDING = ['1.0000000596046448', '1.0000000596046449', '9999999999999999999', '0.0000000000000000001', '-0.000000', '+.000', '5.', '.5',
                 '16777217', '16777217.0000001', '8388608.5', '8388609.5', '12345678901234567890', '0.00000000000000000001', '1e-3', '-1E5',
                 '0x1p3', 'inf', '-inf', 'nan', '-nan', 'Infinity', '340282346638528859811704183484516925440.000000', '1e39', '1e-46', '4e-324']


def test_listed_values_and_rounding_literals(tmp_path):
    """K13's edge list (signed zeros, subnormals, powers of two, both sides of 2^64, FLT_MAX, infinities, NaNs, ties) written by the host
    writer: plain tokens, tokens of more than 19 digits and nan / inf through the host patch; then the literals as a file"""
    import textio
    values = edge_bits().view(np.float32)
    cols = 7
    m = values[:len(values) // cols * cols].reshape(-1, cols)
    path = str(tmp_path / 'edge.dat')
    textio.write_matrix(path, m, where='host')
    assert _same(path)[0] == m.shape
    lit = _file(tmp_path, ''.join(' '.join(HARD_ROUNDING[r:r + 2]) + ' \n' for r in range(0, len(HARD_ROUNDING), 2)), 'lit.dat')
    shape, raw = _same(lit)
    got = np.frombuffer(raw, dtype=np.uint32)
    assert shape == (len(HARD_ROUNDING) // 2, 2) and got[0] == 0x3f800000 and got[4] == 0x80000000 and got[5] == 0
    with np.errstate(over='ignore'):
        want = [np.float32(float.fromhex(t) if 'x' in t else float(t)) for t in HARD_ROUNDING]
    for k, (t, w) in enumerate(zip(HARD_ROUNDING, want)):
        assert np.isnan(got[k:k + 1].view(np.float32)[0]) if 'nan' in t else raw[4 * k:4 * k + 4] == w.tobytes(), t


_values = {}


def _model_values(n):
    if 'v' not in _values:
        rng = np.random.Generator(np.random.PCG64(14))
        _values['v'] = np.concatenate([edge_bits().view(np.float32)[:40], (0.3 * rng.standard_normal(130000)).astype(np.float32)])
    return _values['v'][:n]


@pytest.mark.parametrize('rows', [0, 1, 1000])
@pytest.mark.parametrize('cols', [1, 3, 64, 65, 129])
def test_matrix_shapes(tmp_path, rows, cols):
    import textio
    m = _model_values(rows * cols).reshape(rows, cols)
    path = str(tmp_path / 'm.dat')
    textio.write_matrix(path, m, where='host')
    want = _same(path)
    assert want[0] == ((rows, cols) if rows else (0, 0))


@pytest.mark.parametrize('text,shape', [('7.25 \n', (1, 1)), ('', (0, 0)), ('1.0 2.0 \n3.0 4.0 ', (2, 2)), ('1.0 2.0\n', (1, 2)), ('1.0 2.0 ', (1, 2)),
                                        ('1.0 2.0\n3.0 4.0', (2, 2)), ('5', (1, 1)), ('1\n2\n3\n', (3, 1))])
def test_small_files_and_line_ends(tmp_path, text, shape):
    assert _same(_file(tmp_path, text))[0] == shape


def test_chunk_boundaries(tmp_path):
    """chunk_bytes = 64: a token start on the last and on the first byte of a chunk, a 46-byte token across a boundary, a line several
    chunks long, two chunks without a delimiter, and more chunks than the scan's workgroup has threads"""
    import textio
    long_tok = '340282346638528859811704183484516925440.000000'
    run = '1' + '0' * 199 + '.5'                                     # more than 19 digits: the host patches it in
    a = '1.5 ' * 15 + '25 ' + '7 ' + '2.25 ' * 12 + '33 ' + '0.5 ' * 10 + long_tok + ' ' + run + ' \n'
    n = len(a.split())
    text = a + '2 ' * n + '\n' + a
    assert len(long_tok) == 46 and text[62:65] == ' 7 '              # a one-byte token on the last byte of chunk 0
    assert text[127] == ' ' and text[128] == '0'                    # a token start on the first byte of chunk 2
    assert text.index(long_tok) < 192 < text.index(long_tok) + 46
    assert ' ' not in text[256:384] and '\n' not in text[256:384] and len(a) > 6 * 64
    shape, raw = _same(_file(tmp_path, text), chunks=(64, 128, None))
    assert shape == (3, n)
    rng = np.random.Generator(np.random.PCG64(15))
    m = (0.2 * rng.standard_normal((1000, 13))).astype(np.float32)   # ~120 KB: 1,900 chunks of 64 bytes, two per scan thread
    path = str(tmp_path / 'wide.dat')
    textio.write_matrix(path, m, where='host')
    assert os.path.getsize(path) > 64 * 1024 * 1.5
    assert _same(path)[0] == (1000, 13)


def test_hard_token_share(tmp_path):
    rng = np.random.Generator(np.random.PCG64(16))
    v = rng.standard_normal(65 * 40)
    every = ' '.join('%.6e' % x for x in v)
    assert _same(_file(tmp_path, every + '\n', 'all.dat'))[0] == (1, len(v))
    some = ''.join(' '.join(('%.3e' if (r * 65 + c) % 64 == 63 else '%f') % v[r * 65 + c] for c in range(65)) + ' \n' for r in range(40))
    assert _same(_file(tmp_path, some, 'some.dat'))[0] == (40, 65)
    last = ''.join(' '.join('%f' % v[r * 65 + c] if (r, c) != (39, 64) else 'nan' for c in range(65)) + ' \n' for r in range(40))
    shape, raw = _same(_file(tmp_path, last, 'last.dat'))
    assert shape == (40, 65) and np.isnan(np.frombuffer(raw, np.float32)[-1])


NOT_CANONICAL = {
    'leading space': ' 1.0 2.0 \n3.0 4.0 \n',
    'leading space later': '1.0 2.0 \n 3.0 4.0 \n',
    'interior double space': '1.0  2.0 \n3.0 4.0 5.0 \n',
    'interior double space, equal counts': '1.0 2.0 \n3.0  4.0 \n',
    'trailing double space': '1.0 2.0  \n3.0 4.0 \n',
    'crlf': '1.0 2.0\r\n3.0 4.0\r\n',
    'tab between tokens': '1.0\t2.0 \n3.0\t4.0 \n',
    'vertical tab and form feed': '1.0 2.0 \v\n3.0 4.0 \f\n',
    'blank line in the middle': '1.0 2.0 \n\n3.0 4.0 \n',
    'blank line at the end': '1.0 2.0 \n3.0 4.0 \n\n',
    'blank line first': '\n1.0 2.0 \n',
    'first line longer': '1.0 2.0 3.0 \n4.0 5.0 \n6.0 7.0 \n',
    'first line shorter': '1.0 \n4.0 5.0 \n6.0 7.0 \n',
    'middle line longer': '1.0 2.0 \n4.0 5.0 9.0 \n6.0 7.0 \n',
    'middle line shorter': '1.0 2.0 \n4.0 \n6.0 7.0 \n',
    'last line longer': '1.0 2.0 \n4.0 5.0 \n6.0 7.0 8.0 \n',
    'last line shorter': '1.0 2.0 \n4.0 5.0 \n6.0 \n',
    'last line shorter, unterminated': '1.0 2.0 \n4.0 5.0 \n6.0',
    'longer and shorter cancel': '1.0 2.0 \n4.0 5.0 6.0 \n7.0 \n',
    'blank lines only': '\n\n\n',
    'one space': ' ',
    'one newline': '\n',
}


@pytest.mark.parametrize('name', sorted(NOT_CANONICAL))
def test_not_canonical(tmp_path, name):
    """the host reader's outcome either way: an array where it tolerates the layout (CRLF, a leading space, blank lines only),
    TextFormatError where it does not (an empty token, a tab inside a line, ragged rows)"""
    _same(_file(tmp_path, NOT_CANONICAL[name]), canonical=False)


def test_not_canonical_far_into_a_file(tmp_path):
    """the offending byte in another chunk than the file's start, the rule broken across a chunk boundary ('\\n' at 63, ' ' at 64)"""
    import textio
    line = '1.5 ' * 15 + '2.5\n'                                    # 64 bytes, '\n' at 63
    assert len(line) == 64
    ok = _file(tmp_path, line * 40, 'ok.dat')
    assert _same(ok)[0] == (40, 16)
    bad = _file(tmp_path, line * 20 + ' ' + line[1:] + line * 19, 'bad.dat')
    _same(bad, canonical=False)
    with pytest.raises(textio.MatrixNotCanonical) as info:
        textio.read_matrix_device(bad, chunk_bytes=64)
    assert info.value.offset == 20 * 64
    ragged = _file(tmp_path, line * 20 + '1.5 ' * 16 + '2.5\n' + line * 19, 'ragged.dat')
    _same(ragged, canonical=False)
    with pytest.raises(textio.MatrixNotCanonical) as info:
        textio.read_matrix_device(ragged, chunk_bytes=64)
    assert info.value.offset == 21 * 64 + 4                          # the first line that does not start at token line * cols


@pytest.mark.parametrize('token', ['abc', '1.0x', '--1'])
def test_canonical_layout_with_a_bad_token(tmp_path, token):
    import textio
    path = _file(tmp_path, '1.0 2.0 \n3.0 %s \n5.0 6.0 \n' % token)
    assert _same(path) == 'TextFormatError'
    with pytest.raises(textio.TextFormatError):
        textio.read_matrix(path, where='host')


def _is_canonical(text):
    if not text:
        return True
    if any(c in text for c in '\t\r\v\f') or text[0] in ' \n' or any(p in text for p in ('  ', '\n ', '\n\n')):
        return False
    lines = text.split('\n')
    if lines[-1] == '':
        lines.pop()
    return len({len([t for t in ln.split(' ') if t]) for ln in lines}) == 1


def test_fuzz(tmp_path):
    """24 files of up to a few KB, seeded: tokens drawn from plain, exponent, signed-zero, long-digit and inf / nan forms (now and then
    one that is no number), line ends from ' \\n', '\\n', '\\r\\n', '  \\n' -- one kind per file in most files, mixed in the others"""
    import textio
    rng = np.random.Generator(np.random.PCG64(17))

    def token():
        kind = int(rng.integers(0, 100))
        x = float(rng.standard_normal()) * 10.0 ** int(rng.integers(-8, 9))
        if kind < 55:
            return '%f' % x
        if kind < 65:
            return '%.*f' % (int(rng.integers(0, 20)), x)
        if kind < 75:
            return '%.4e' % x
        if kind < 82:
            return ('-0.000000', '0.000000', '-0', '+0.', '-.0')[int(rng.integers(5))]
        if kind < 90:
            return ''.join(str(d) for d in rng.integers(0, 10, int(rng.integers(18, 24)))) + '.25'
        if kind < 98:
            return ('inf', '-inf', 'nan', '1e400', '-1e-400')[int(rng.integers(5))]
        return ('1.0x', 'abc', '')[int(rng.integers(3))] if rng.integers(4) == 0 else '1'
    ends = [' \n', '\n', '\r\n', '  \n']
    outcomes = set()
    for k in range(24):
        rows, cols = int(rng.integers(1, 30)), int(rng.integers(1, 12))
        end = ends[k % 4] if k < 16 else None
        text = ''
        for r in range(rows):
            n = cols + (int(rng.integers(-1, 2)) if k % 6 == 5 and r == rows // 2 else 0)
            text += ' '.join(token() for _ in range(max(n, 1))) + (end if end is not None else ends[int(rng.integers(4))])
        if k % 8 == 3:
            text = text.rstrip('\n')
        path = _file(tmp_path, text, 'f%d.dat' % k)
        try:
            textio.read_matrix_device(path, chunk_bytes=256)
            canonical = True
        except textio.MatrixNotCanonical:
            canonical = False
        except textio.TextFormatError:
            canonical = True
        assert canonical == _is_canonical(text), k
        out = _same(path, canonical=canonical, chunks=(64, 256))
        outcomes.add((canonical, out == 'TextFormatError'))
    assert len(outcomes) >= 3                                        # canonical and not, arrays and errors


def test_cache_holds_the_same_copy(tmp_path, monkeypatch):
    import textio
    rng = np.random.Generator(np.random.PCG64(18))
    m = rng.standard_normal((50, 9)).astype(np.float32) * np.float32(1e7)
    copies = {}
    for where in ('host', 'device'):
        path = str(tmp_path / (where + '.dat'))
        monkeypatch.setenv('TKR_NO_CACHE', '1')
        textio.write_matrix(path, m, where='host')
        assert not os.path.exists(path + '.npy')
        monkeypatch.setenv('TKR_NO_CACHE', '')
        before = dict(textio.scan_counts)
        first = textio.read_matrix(path, where=where)
        assert textio.scan_counts[where] == before[where] + 1 and os.path.exists(path + '.npy')
        again = textio.read_matrix(path, where=where)                # the stamped copy: no reader runs
        assert textio.scan_counts[where] == before[where] + 1 and again.tobytes() == first.tobytes()
        copies[where] = open(path + '.npy', 'rb').read()
    assert copies['host'] == copies['device']


def test_auto_takes_the_device_from_the_threshold(golden_dir, monkeypatch):
    import textio
    path = os.path.join(golden_dir, 'g3', 'mat.dat')
    monkeypatch.delenv('TKR_MATRIX', raising=False)
    host = textio.read_matrix(path, where='host')
    before = dict(textio.scan_counts)
    assert textio.read_matrix(path).tobytes() == host.tobytes()      # a few KB: below MATRIX_DEVICE_FROM
    assert textio.scan_counts == dict(before, host=before['host'] + 1)
    monkeypatch.setenv('TKR_MATRIX_DEVICE_FROM', '0')
    assert textio.read_matrix(path).tobytes() == host.tobytes()
    assert textio.read_matrix(path, where='auto').tobytes() == host.tobytes()
    assert textio.scan_counts == dict(host=before['host'] + 1, device=before['device'] + 2)
    monkeypatch.setenv('TKR_MATRIX_DEVICE_FROM', 'many')
    with pytest.raises(ValueError):
        textio.read_matrix(path)


def test_cli_reads_the_model_on_the_device(golden_dir, tmp_path, monkeypatch, capsys):
    """evaluate.py and recommend.py on golden G4 with TKR_MATRIX=device: the same stdout, the same file"""
    import evaluate
    import recommend
    import textio
    d = os.path.join(golden_dir, 'g4')
    data, model = os.path.join(d, 'data'), os.path.join(d, 'model')
    assert os.environ.get('TKR_NO_CACHE') == '1'
    out, lines, files = {}, {}, {}
    for where in ('host', 'device'):
        monkeypatch.setenv('TKR_MATRIX', where)
        before = dict(textio.scan_counts)
        capsys.readouterr()
        lines[where] = evaluate.main(['-d', data, '-m', model, '-sl', 'im', 'om'])
        out[where] = capsys.readouterr().out
        assert textio.scan_counts[where] >= before[where] + 2        # final-U.dat and final-V.dat
        other = 'device' if where == 'host' else 'host'
        assert textio.scan_counts[other] == before[other]
        path = str(tmp_path / (where + '.txt'))
        recommend.main(['-d', data, '-m', model, '-f', '0', '-t', '30', '-o', path])
        files[where] = open(path, 'rb').read()
    assert out['device'] == out['host'] and lines['device'] == lines['host'] and len(out['host']) > 0
    assert files['device'] == files['host'] and len(files['host']) > 0
