"""What of the device-side matrix reader (K14, csrc/scan_dev.hip) can be checked without a GPU: the `where` argument of
textio.read_matrix, argument validation of the new C entry points (host-only calls), and the classify-and-convert routine of
csrc/scan_num.h -- the code every lane of the convert kernel runs -- on the CPU (tkr_matrix_token_host) against
np.float32(float(token)), compared as bytes."""
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
    path = os.path.join(golden_dir, 'g3', 'mat.dat')
    with pytest.raises(ValueError):
        textio.read_matrix(path, where='bogus')
    monkeypatch.setenv('TKR_MATRIX', 'bogus')
    with pytest.raises(ValueError):
        textio.read_matrix(path)
    monkeypatch.setenv('TKR_MATRIX', 'host')
    by_env = textio.read_matrix(path)
    monkeypatch.delenv('TKR_MATRIX')
    monkeypatch.delenv('TKR_MATRIX_DEVICE_FROM', raising=False)
    assert textio.MATRIX_WHERE == ('host', 'device', 'auto') and textio.MATRIX_DEFAULT == 'auto' and textio.MATRIX_DEVICE_FROM >= 1 << 20
    before = dict(textio.scan_counts)
    host = textio.read_matrix(path, where='host')
    auto = textio.read_matrix(path, where='auto')
    default = textio.read_matrix(path)
    assert textio.scan_counts == dict(before, host=before['host'] + 3)            # a file of a few KB: the host reader, GPU or not
    assert host.dtype == np.float32 and host.ndim == 2 and host.size > 0
    for other in (auto, default, by_env):
        assert other.dtype == np.float32 and other.shape == host.shape and other.tobytes() == host.tobytes()
    if not torch.cuda.is_available():
        with pytest.raises(tkr_hip.TkrError, match='MI355X'):
            textio.read_matrix(path, where='device')
        with pytest.raises(tkr_hip.TkrError, match='MI355X'):
            textio.read_matrix_device(path)
        monkeypatch.setenv('TKR_MATRIX_DEVICE_FROM', '0')                         # 'auto' without a GPU is the host at any size
        assert textio.read_matrix(path, where='auto').tobytes() == host.tobytes()


def test_entry_points_check_their_arguments_before_any_device_access():
    """host-only calls: every pointer below is either NULL or an address nothing may touch"""
    import tkr_hip
    lib = tkr_hip.lib()
    assert lib.tkr_scan_dev_workspace_bytes(I64(1000), I64(64)) > 0
    assert lib.tkr_scan_dev_workspace_bytes(I64(0), I64(64)) > 0
    for chunk in (0, 1, 32, 63, 96, 100, (1 << 20) + 1, 1 << 21, -64):
        assert lib.tkr_scan_dev_workspace_bytes(I64(1000), I64(chunk)) == E_INVAL, chunk
    assert lib.tkr_scan_dev_workspace_bytes(I64(-1), I64(64)) == E_INVAL
    assert lib.tkr_scan_dev_workspace_bytes(I64(1 << 40), I64(64)) == E_INVAL           # more chunks than one launch takes
    with pytest.raises(ValueError):
        tkr_hip.scan_dev_workspace_bytes(1000, 96)

    fake = 1 << 12                                                   # aligned, never dereferenced
    ws = lib.tkr_scan_dev_workspace_bytes(I64(1000), I64(64))

    def count(text=fake, n=1000, chunk=64, work=fake, work_bytes=ws, totals=fake):
        return lib.tkr_matrix_count_dev(PTR(text), I64(n), I64(chunk), PTR(work), I64(work_bytes), PTR(totals), None)

    for bad in (dict(text=None), dict(work=None), dict(totals=None), dict(n=-1), dict(chunk=0), dict(chunk=96), dict(chunk=32),
                dict(chunk=1 << 21), dict(text=fake + 4), dict(work=fake + 8), dict(totals=fake + 4), dict(work_bytes=ws - 1),
                dict(work_bytes=0)):
        assert count(**bad) == E_INVAL, bad

    def emit(**kw):
        a = dict(text=fake, n=1000, chunk=64, work=fake, work_bytes=ws, n_lines=10, n_tokens=100, cols=10, tok_start=fake, data=fake, hard=fake,
                 counts=fake)
        a.update(kw)
        return lib.tkr_matrix_emit_dev(PTR(a['text']), I64(a['n']), I64(a['chunk']), PTR(a['work']), I64(a['work_bytes']), I64(a['n_lines']),
                                       I64(a['n_tokens']), I64(a['cols']), PTR(a['tok_start']), PTR(a['data']), PTR(a['hard']), PTR(a['counts']),
                                       None)

    for bad in (dict(text=None), dict(work=None), dict(n=-1), dict(chunk=0), dict(chunk=96), dict(chunk=32), dict(chunk=1 << 21),
                dict(work_bytes=ws - 1), dict(n_lines=-1), dict(n_tokens=-1), dict(cols=-1), dict(n_lines=1001), dict(n_tokens=1001),
                dict(cols=1001), dict(tok_start=None), dict(data=None), dict(hard=None), dict(counts=None), dict(text=fake + 8),
                dict(work=fake + 4), dict(tok_start=fake + 4), dict(data=fake + 2), dict(hard=fake + 4), dict(counts=fake + 4)):
        assert emit(**bad) == E_INVAL, bad

    out = ctypes.c_float()
    assert lib.tkr_matrix_token_host(None, I64(0), ctypes.byref(out)) == E_INVAL
    assert lib.tkr_matrix_token_host(b'1', I64(-1), ctypes.byref(out)) == E_INVAL
    assert lib.tkr_matrix_token_host(b'1', I64(1), None) == E_INVAL
    start, res = np.zeros(1, np.int64), np.zeros(1, np.float32)

    def tokens(text, at):
        start[0] = at
        return lib.tkr_matrix_tokens_host(text, I64(len(text)), PTR(start.ctypes.data), I64(1), PTR(res.ctypes.data))

    assert tokens(b'1.5 2e1\n', 4) == 0 and res[0] == 20.0
    assert tokens(b'1.5 2e1\n', 8) == E_INVAL and tokens(b'1.5 2e1\n', -1) == E_INVAL
    assert tokens(b'1.5 2e1x', 4) == -4                              # TKR_E_PARSE, as tkr_matrix_read answers
    assert lib.tkr_matrix_tokens_host(None, I64(8), PTR(start.ctypes.data), I64(1), PTR(res.ctypes.data)) == E_INVAL


def _want(token):
    return np.float32(float(token)).tobytes()


def _check_tokens(tokens, hard_allowed=None):
    """every token is converted to the bytes of np.float32(float(token)), or reported hard where hard_allowed(token) says it may be;
    -> the number of hard ones"""
    import tkr_hip
    hard = 0
    for tok in tokens:
        got = tkr_hip.matrix_token_host(tok.encode())
        if got is None:
            assert hard_allowed is not None and hard_allowed(tok), tok
            hard += 1
        else:
            assert hard_allowed is None or not hard_allowed(tok), tok
            assert got == _want(tok), (tok, got.hex(), _want(tok).hex())
    return hard


def _significant(tok):
    return len(tok.lstrip('+-').replace('.', '').lstrip('0'))


def test_percent_f_of_random_bit_patterns():
    """'%f' of 100,000 random fp32 bit patterns: hard is exactly the set of non-finite values and of more than 19 significant digits"""
    rng = np.random.Generator(np.random.PCG64(141))
    values = rng.integers(0, 1 << 32, 100000, dtype=np.uint64).astype(np.uint32).view(np.float32)
    tokens = ['%f' % float(v) for v in values]
    hard = _check_tokens(tokens, lambda t: t.lstrip('-') in ('inf', 'nan') or _significant(t) > 19)
    assert 25000 < hard < 40000                                      # 1e13 and above: about a third


def test_percent_f_of_gaussian_values():
    rng = np.random.Generator(np.random.PCG64(142))
    values = np.concatenate([rng.standard_normal(60000), 0.05 * rng.standard_normal(40000)]).astype(np.float32)
    assert _check_tokens(['%f' % float(v) for v in values]) == 0


def test_random_plain_digit_strings():
    """100,000 plain tokens, f = 0 ... 19 digits behind the '.', up to 19 significant digits, optional sign, with and without digits in
    front of and behind the '.'"""
    rng = np.random.Generator(np.random.PCG64(143))
    tokens = ['5.', '.5', '+.000', '-0.000000', '0', '-0', '+0.', '00012.500', '-.0000000000000000001', '000000000000000000000001']
    while len(tokens) < 100000:
        f = int(rng.integers(0, 20))
        n = int(rng.integers(1, 20))                                 # digits in all, at least f of them... or fewer: zeros fill in
        digits = ''.join(str(d) for d in rng.integers(0, 10, n))
        if f >= n:
            whole, frac = ('0' if rng.integers(2) else ''), '0' * (f - n) + digits
        else:
            whole, frac = digits[:n - f], digits[n - f:]
        tok = ('', '+', '-')[int(rng.integers(3))] + whole + ('.' + frac if f or rng.integers(2) else '')
        if any(c.isdigit() for c in tok):
            tokens.append(tok)
    assert _check_tokens(tokens) == 0
    import tkr_hip
    assert tkr_hip.matrix_token_host(b'-0.000000') == bytes.fromhex('00000080')
    assert tkr_hip.matrix_token_host(b'+.000') == bytes(4) and tkr_hip.matrix_token_host(b'5.') == _want('5.0')


def test_neighbours_of_fp32_rounding_midpoints():
    """for every f = 0 ... 19: floor(mid * 10^f) + {-1, 0, 1} / 10^f around 10,000 midpoints between adjacent fp32 values, where the
    integer stays within 19 digits -- the decimal strings closest to where the second rounding flips"""
    from fractions import Fraction
    rng = np.random.Generator(np.random.PCG64(144))
    tokens = []
    for f in range(20):
        # values whose midpoint times 10^f has at most 19 digits: below 10^(19 - f); exponents drawn evenly, mantissas at random
        top = min(19 - f, 19) * np.log2(10.0) - 1
        exps = rng.integers(-20, max(int(top), -19), 500)
        mants = rng.integers(1 << 23, 1 << 24, 500)
        for e, m in zip(exps.tolist(), mants.tolist()):
            mid = Fraction(2 * m + 1, 2) * Fraction(2) ** (e - 23)
            base = int(mid * 10 ** f)
            for w in (base - 1, base, base + 1):
                if 0 < w < 10 ** 19:
                    s = str(w).rjust(f + 1, '0')
                    tokens.append(s[:len(s) - f] + '.' + s[len(s) - f:] if f else s)
    assert len(tokens) > 25000
    assert _check_tokens(tokens) == 0


def test_literals():
    import tkr_hip
    assert tkr_hip.matrix_token_host(b'1.0000000596046448') == bytes.fromhex('0000803f')      # two roundings: a direct one gives 0x3f800001
    assert _want('1.0000000596046448') == bytes.fromhex('0000803f')
    for tok in ('9999999999999999999', '0.0000000000000000001', '-9999999999.999999999', '1.0000000596046449', '16777217', '16777217.0000001',
                '0.1', '1', '8388608.5', '8388609.5', '0.000001'):
        assert tkr_hip.matrix_token_host(tok.encode()) == _want(tok), tok


@pytest.mark.parametrize('token', [b'1e-3', b'0x1p3', b'inf', b'nan', b'', b'.', b'+', b'-', b'+.', b'1_0', b'12345678901234567890',
                                   b'1.2345678901234567890', b'0.00000000000000000000', b'\t1.0', b'1.0x', b'1.0\x001', b'1\xc2\xa0', b'\xff',
                                   b'--1', b'1..0', b'1.0.', b'1 2', b'1\n', b'1-', b'Infinity', b'1E5'])
def test_hard_tokens(token):
    """exponent forms, words, hex, nothing but a sign or a '.', 20 significant digits, 20 digits behind the '.', a tab in front, junk
    behind, an embedded NUL, non-ASCII bytes, a delimiter inside: all left to the host"""
    import tkr_hip
    assert tkr_hip.matrix_token_host(token) is None
