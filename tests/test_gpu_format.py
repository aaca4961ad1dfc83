"""K13 (csrc/format_dev.hip) on the GPU: textio.write_matrix / write_lists / format_lists_device with where='device' against the host
writers and against Python's own '%f'.  Every comparison is byte equality."""
import os
import shutil

import numpy as np
import pytest
import torch

from _format_oracle import edge_bits, python_f

pytestmark = pytest.mark.gpu

_cache = {}


def value_list():
    """-> (fp32 values, their '%f' texts): the edge list of tests/_format_oracle.py (specials, extremes, powers of two, ties, carries,
    each with its negative), 65,536 random bit patterns and 65,536 values from N(0, 3); computed once"""
    if 'values' not in _cache:
        rng = np.random.Generator(np.random.PCG64(13))
        bits = np.concatenate([edge_bits(), rng.integers(0, 1 << 32, 65536, dtype=np.uint64).astype(np.uint32),
                               (3.0 * rng.standard_normal(65536)).astype(np.float32).view(np.uint32)])
        _cache['values'] = (bits.view(np.float32).copy(), [python_f(b) for b in bits.tolist()])
    return _cache['values']


def matrix_text(texts, rows, cols):
    return ''.join(''.join(t + ' ' for t in texts[r * cols:(r + 1) * cols]) + '\n' for r in range(rows)).encode()


def test_every_listed_value_as_a_matrix(tmp_path):
    import textio
    values, texts = value_list()
    cols = 67
    rows = len(values) // cols                                       # the edge values come first: what the cut drops is random
    m = values[:rows * cols].reshape(rows, cols)
    want = matrix_text(texts, rows, cols)
    before = dict(textio.format_counts)
    dev, host = str(tmp_path / 'dev.dat'), str(tmp_path / 'host.dat')
    textio.write_matrix(dev, m, where='device')
    textio.write_matrix(host, m, where='host')
    assert textio.format_counts == dict(host=before['host'] + 1, device=before['device'] + 1)
    assert open(dev, 'rb').read() == want
    assert open(host, 'rb').read() == want
    assert max(len(t) for t in texts) == 47
    # a tensor that is on the device already, in blocks of a few rows, and the run repeated: the same bytes
    textio.write_matrix(dev, torch.from_numpy(m).cuda(), where='device', block_bytes=8192)
    assert open(dev, 'rb').read() == want
    with pytest.raises(ValueError, match='at least'):
        textio.write_matrix(dev, m, where='device', block_bytes=100)


@pytest.mark.parametrize('rows', [0, 1, 1000])
@pytest.mark.parametrize('cols', [1, 3, 64, 65, 129])
def test_matrix_shapes(tmp_path, rows, cols):
    import textio
    values, texts = value_list()
    at = (rows * 31 + cols) % 200                                    # a different cut of the list per shape, the edge values in it
    m = values[at:at + rows * cols].reshape(rows, cols)
    path = str(tmp_path / 'm.dat')
    textio.write_matrix(path, m, where='device')
    assert open(path, 'rb').read() == matrix_text(texts[at:], rows, cols)


def test_matrix_without_columns_and_golden_g3(golden_dir, tmp_path, monkeypatch):
    import textio
    path = str(tmp_path / 'm.dat')
    textio.write_matrix(path, np.zeros((5, 0), np.float32), where='device')
    assert open(path, 'rb').read() == b'\n' * 5
    d = os.path.join(golden_dir, 'g3')
    exp = np.load(os.path.join(d, 'expected.npz'))
    for name in ('mat', 'bias'):
        textio.write_matrix(path, exp[name], where='device')
        assert open(path, 'rb').read() == open(os.path.join(d, name + '.dat'), 'rb').read()      # the reference's export_embed_to_file
    assert not os.path.exists(path + '.npy')                         # TKR_NO_CACHE=1 in the test environment
    monkeypatch.setenv('TKR_NO_CACHE', '')                           # with the stamped copy: a cached read returns what the text says
    textio.write_matrix(path, exp['mat'], where='device')
    assert os.path.exists(path + '.npy')
    np.testing.assert_array_equal(textio.read_matrix(path), exp['back_all'])
    # utils.export_embed_to_file goes through write_matrix: 'auto' takes the device from the threshold on
    import utils
    monkeypatch.setenv('TKR_NO_CACHE', '1')
    monkeypatch.setenv('TKR_FORMAT_DEVICE_FROM', '1')
    before = textio.format_counts['device']
    utils.export_embed_to_file(path, exp['mat'])
    assert textio.format_counts['device'] == before + 1
    assert open(path, 'rb').read() == open(os.path.join(d, 'mat.dat'), 'rb').read()


# ---- lists -------------------------------------------------------------------------------------------------------------------------
def token_tables():
    """-> (users IdMap, items IdMap, the user indices, the item indices): token lengths 0 ... 40 bytes, '' among both, multi-byte UTF-8,
    indices permuted against token order, with indices no token has in between"""
    if 'tables' not in _cache:
        import textio
        rng = np.random.Generator(np.random.PCG64(21))
        alphabet = list('abcXYZ019-_. ') + ['é', 'ß', '日', '😀']

        def tokens(n):
            seen, out = set(), []
            for k in range(n):
                while True:
                    t = ''
                    target = k if k < 41 else 1 + k % 40              # bytes: 0 ... 40 once each, then 1 ... 40 again
                    while len(t.encode()) < target:
                        c = alphabet[int(rng.integers(len(alphabet)))]
                        if len((t + c).encode()) <= target:
                            t += c
                    if t not in seen:
                        break
                seen.add(t)
                out.append(t)
            return out

        utoks, itoks = tokens(90), tokens(330)
        uidx = rng.permutation(120)[:len(utoks)]
        iidx = rng.permutation(400)[:len(itoks)]
        users = textio.IdMap({t: int(i) for t, i in zip(utoks, uidx)})
        items = textio.IdMap({t: int(i) for t, i in zip(itoks, iidx)})
        assert '' in utoks and '' in itoks and max(len(t.encode()) for t in itoks) == 40
        _cache['tables'] = (users, items, uidx.astype(np.int32), iidx.astype(np.int32))
    return _cache['tables']


def make_lists(n, K, seed):
    """n rows of K entries: ids drawn from the item indices, negatives at the start, in the middle, at the end of a row and rows of
    nothing but negatives; row_user drawn with repeats, the '' uid among them; scores cut from the value list"""
    users, items, uidx, iidx = token_tables()
    rng = np.random.Generator(np.random.PCG64(seed))
    values, _ = value_list()
    ids = iidx[rng.integers(0, len(iidx), (n, K))].astype(np.int32)
    for r in range(n):
        if r % 5 == 0:
            ids[r, 0] = -1
        elif r % 5 == 1:
            ids[r, K // 2] = -7
        elif r % 5 == 2:
            ids[r, K - 1] = -1
        if r % 7 == 3:
            ids[r, :] = -1
        if r % 11 == 4:
            ids[r, rng.integers(0, K, max(K // 2, 1))] = -2
    at = (seed * 977) % 100
    scores = np.resize(values[at:at + 4000], (n, K)).astype(np.float32)
    row_user = uidx[rng.integers(0, len(uidx), n)].astype(np.int32)
    if n:
        empty_uid = [i for i, t in users.tokens_by_index().items() if t == ''][0]
        row_user[n // 2] = empty_uid
    return ids, scores, row_user


def host_text(ids, scores, row_user):
    import textio
    users, items, _, _ = token_tables()
    utok = users.tokens_by_index()
    lines = textio.format_lines([utok[int(u)] for u in row_user], ids, scores, items.tokens_by_index())
    return lines, ('\n'.join(lines) + '\n').encode() if lines else b''


@pytest.mark.parametrize('n', [0, 1, 257])
@pytest.mark.parametrize('K', [1, 30, 64, 65, 200])
def test_lists_structure(tmp_path, n, K):
    import textio
    users, items, _, _ = token_tables()
    ids, scores, row_user = make_lists(n, K, seed=K * 1000 + n)
    lines, want = host_text(ids, scores, row_user)
    if n == 257:
        assert any(ln.startswith(',') or ln == '' for ln in lines) and any(',' not in ln for ln in lines)      # '' as uid; a uid alone
    text, line_ptr = textio.format_lists_device(ids, scores, row_user, users, items)
    assert text.is_cuda and text.dtype == torch.uint8 and line_ptr.dtype == torch.int64
    assert bytes(text.cpu().numpy()) == want
    assert line_ptr.cpu().tolist() == np.concatenate([[0], np.cumsum([len(ln.encode()) + 1 for ln in lines])]).astype(np.int64).tolist()
    dev, host = str(tmp_path / 'dev.txt'), str(tmp_path / 'host.txt')
    assert textio.write_lists(dev, users, torch.from_numpy(ids).cuda(), torch.from_numpy(scores).cuda(), row_user, items, where='device') == len(want)
    assert textio.write_lists(host, users, ids, scores, row_user, items, where='host') == len(want)
    assert open(dev, 'rb').read() == want and open(host, 'rb').read() == want
    # determinism: a second device run gives the same bytes
    again, again_ptr = textio.format_lists_device(ids, scores, row_user, users, items)
    assert torch.equal(again, text) and torch.equal(again_ptr, line_ptr)


def test_lists_more_rows_than_one_scan_run_and_blocks(tmp_path):
    """70,000 rows: every thread of the scan's workgroup sums a run of rows.  block_bytes at the default, at 4,096 and at the longest
    line give the same file; below the longest line nothing is written and the ValueError states the minimum"""
    import textio
    users, items, _, _ = token_tables()
    n, K = 70000, 2
    ids, scores, row_user = make_lists(n, K, seed=5)
    lines, want = host_text(ids, scores, row_user)
    ptr = np.concatenate([[0], np.cumsum([len(ln.encode()) + 1 for ln in lines])]).astype(np.int64)
    text, line_ptr = textio.format_lists_device(ids, scores, row_user, users, items)
    assert bytes(text.cpu().numpy()) == want and np.array_equal(line_ptr.cpu().numpy(), ptr)
    path = str(tmp_path / 'rec.txt')
    for block in (None, 4096):
        assert textio.write_lists(path, users, ids, scores, row_user, items, where='device', block_bytes=block) == len(want)
        assert open(path, 'rb').read() == want
    longest = int(np.diff(ptr).max())
    os.remove(path)
    with pytest.raises(ValueError, match='at least %d' % longest):
        textio.write_lists(path, users, ids, scores, row_user, items, where='device', block_bytes=longest - 1)
    assert not os.path.exists(path)
    # exactly the longest line: rows go out a few at a time, the longest one alone (a slice, to keep the number of blocks small)
    cut = slice(int(np.argmax(np.diff(ptr))) - 1000, int(np.argmax(np.diff(ptr))) + 1000) if np.argmax(np.diff(ptr)) >= 1000 else slice(0, 2000)
    sub = np.diff(ptr)[cut]
    textio.write_lists(path, users, ids[cut], scores[cut], row_user[cut], items, where='device', block_bytes=int(sub.max()))
    assert open(path, 'rb').read() == want[ptr[cut.start]:ptr[cut.stop]]
    # appended parts: the file of the whole
    half = n // 2
    textio.write_lists(path, users, ids[:half], scores[:half], row_user[:half], items, where='device')
    textio.write_lists(path, users, ids[half:], scores[half:], row_user[half:], items, where='device', append=True, block_bytes=1 << 16)
    assert open(path, 'rb').read() == want


def test_indices_without_a_token_raise(tmp_path):
    import textio
    import tkr_hip
    users, items, uidx, iidx = token_tables()
    ids, scores, row_user = make_lists(40, 6, seed=2)
    ids[ids < 0] = int(iidx[0])
    _, want = host_text(ids, scores, row_user)
    n_items = int(iidx.max()) + 1
    hole = sorted(set(range(n_items)) - set(iidx.tolist()))[0]
    path = str(tmp_path / 'rec.txt')

    def both(bad_ids, bad_rows, row):
        with pytest.raises(tkr_hip.TkrError, match='row %d ' % row):
            textio.format_lists_device(bad_ids, scores, bad_rows, users, items)
        with pytest.raises(tkr_hip.TkrError, match='row %d ' % row):
            textio.write_lists(path, users, bad_ids, scores, bad_rows, items, where='device')

    bad = ids.copy()
    bad[17, 3] = bad[30, 0] = n_items                                # equal to the table size: the first offending row is named
    both(bad, row_user, 17)
    bad = ids.copy()
    bad[9, 5] = hole                                                 # inside the table, no token
    both(bad, row_user, 9)
    bad = ids.copy()
    bad[3, 0] = 2 ** 31 - 1
    both(bad, row_user, 3)
    rows = row_user.copy()
    rows[12] = int(uidx.max()) + 1
    both(ids, rows, 12)
    rows[12], rows[5] = row_user[12], -1
    both(ids, rows, 5)
    # the run after it is clean
    text, _ = textio.format_lists_device(ids, scores, row_user, users, items)
    assert bytes(text.cpu().numpy()) == want
    assert textio.write_lists(path, users, ids, scores, row_user, items, where='device') == len(want) and open(path, 'rb').read() == want


# ---- recommend.py --format ---------------------------------------------------------------------------------------------------------
def _g4(golden_dir):
    d = os.path.join(golden_dir, 'g4')
    return os.path.join(d, 'data'), os.path.join(d, 'model')


def _cli_config(name, golden_dir, tmp_path):
    """-> the arguments of one recommend.py configuration on golden G4 (without -o and --format)"""
    data, model = _g4(golden_dir)
    tokens = open(os.path.join(data, 'uid')).read().split()
    items = open(os.path.join(data, 'vid')).read().split()
    base = ['-d', data, '-m', model, '-f', '0', '-t', '30']
    if name == 'plain':
        return base
    if name == 'users':
        (tmp_path / 'some').write_text('%s\n%s\n%s\n' % (tokens[5], tokens[2], tokens[5]))
        return ['-d', data, '-m', model, '-t', '40', '-u', str(tmp_path / 'some')]
    if name == 'candidates':
        rng = np.random.Generator(np.random.PCG64(8))
        asked = [tokens[x] for x in rng.permutation(len(tokens))[:60]] + [tokens[5], tokens[5]]
        lists = [[items[c] for c in rng.choice(len(items), int(rng.integers(1, 80)), replace=False)] for _ in asked]
        (tmp_path / 'cand').write_text(''.join('%s,%s\n' % (u, ','.join('%s:0' % v for v in l)) for u, l in zip(asked, lists)))
        return ['-d', data, '-m', model, '-t', '12', '--candidates', str(tmp_path / 'cand')]
    if name == 'new_users':
        work = tmp_path / 'data'
        shutil.copytree(data, str(work))
        (work / 'uid').write_text('\n'.join(tokens[:-3]) + '\n')
        (tmp_path / 'new_uid').write_text('\n'.join(tokens[-3:]) + '\n')
        return ['-d', str(work), '-m', model, '-t', '10', '--new-uid', str(tmp_path / 'new_uid'), '--new-history', os.path.join(data, 'f0tr.txt'),
                '--seed', '3']
    assert name == 'new_items'
    work, cut_model, cut = tmp_path / 'data', tmp_path / 'model', 5
    shutil.copytree(data, str(work))
    cut_model.mkdir()
    (work / 'vid').write_text('\n'.join(items[:-cut]) + '\n')
    shutil.copy(os.path.join(model, 'final-U.dat'), str(cut_model / 'final-U.dat'))
    rows = open(os.path.join(model, 'final-V.dat')).read().strip('\n').split('\n')
    (cut_model / 'final-V.dat').write_text('\n'.join(rows[:-cut]) + '\n')
    (tmp_path / 'new_vid').write_text('\n'.join(items[-cut:]) + '\n')
    (tmp_path / 'new_ratings').write_text(open(os.path.join(data, 'f0tr.txt')).read() + open(os.path.join(data, 'f0te.om.txt')).read())
    return ['-d', str(work), '-m', str(cut_model), '-t', '10', '--new-vid', str(tmp_path / 'new_vid'), '--new-ratings', str(tmp_path / 'new_ratings'),
            '--seed', '3']


@pytest.mark.parametrize('name', ['plain', 'users', 'candidates', 'new_users', 'new_items'])
def test_recommend_cli_formats_on_the_device(golden_dir, tmp_path, monkeypatch, name):
    import recommend
    import textio
    monkeypatch.delenv('TKR_FORMAT', raising=False)
    monkeypatch.delenv('TKR_FORMAT_DEVICE_FROM', raising=False)
    args = _cli_config(name, golden_dir, tmp_path)
    out = {k: str(tmp_path / (k + '.txt')) for k in ('host', 'device', 'auto', 'auto_device')}
    parts = 2 if name == 'new_users' else 1                          # the model users' lines and the new users' are two writes
    counts = dict(textio.format_counts)
    host = recommend.main(args + ['-o', out['host'], '--format', 'host'])
    assert textio.format_counts == dict(counts, host=counts['host'] + parts)
    device = recommend.main(args + ['-o', out['device'], '--format', 'device'])
    assert textio.format_counts == dict(host=counts['host'] + parts, device=counts['device'] + parts)
    want = open(out['host'], 'rb').read()
    assert len(host) > 0 and want == ('\n'.join(host) + '\n').encode()
    assert device == host and open(out['device'], 'rb').read() == want
    # 'auto' on these inputs (a few thousand fields) is the host writer; TKR_FORMAT_DEVICE_FROM=1 sends it to the device
    counts = dict(textio.format_counts)
    assert recommend.main(args + ['-o', out['auto']]) == host and open(out['auto'], 'rb').read() == want
    assert textio.format_counts == dict(counts, host=counts['host'] + parts)
    monkeypatch.setenv('TKR_FORMAT_DEVICE_FROM', '1')
    assert recommend.main(args + ['-o', out['auto_device']]) == host and open(out['auto_device'], 'rb').read() == want
    assert textio.format_counts == dict(host=counts['host'] + parts, device=counts['device'] + parts)
