"""K19 (tkr_nearest_anchors; csrc/explain.hip), explain.py, recommend.py --explain and evaluate.py -M unexp on the GPU, against
tests/_explain_oracle.py.  Positions are integers and compared exactly, similarities bit for bit."""
import ctypes as C
import os
import shutil
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _explain_oracle as O

import diversity
import explain
import tkr_hip
from oracle import ref_np as R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N_ITEMS = 600
# (rows, t, e): every t of 1, 5, 30, 64, 65, 256 (and 300: the 1024-thread workgroup below its full width), every e of 1, 3, 8, and 1, 3,
# 70 rows.  The list's rows and 8 anchor rows must fit the 160 KB of a CU for the staged form; where they do not, the form that reads
# through L2 runs: at k = 1000 from t = 64 (the plans with t = 64, 65, 256, 300), at k = 264 at t = 256 and 300, at k = 128 and 130 at
# t = 300.  Every other (k, plan) -- all of k = 1, 7, 50 -- runs staged.
PLANS = [(1, 1, 1), (3, 5, 3), (70, 30, 3), (70, 30, 8), (3, 64, 8), (70, 65, 1), (3, 256, 3), (1, 256, 8), (3, 300, 3)]
LONG = (3, 1024, 3)                                                   # t = 1024, staged: where the chain is short (k = 1, 7)


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to('cuda')


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


def _case(rng, rows, t, e):
    """lists with replacement (duplicated ids), anchor rows of 0, 1, e - 1, e, 63, 64, 65, 300 or 2500 columns with replacement (2500 >
    N_ITEMS: repeats), and the rows the kernel must get right -- see the test's text"""
    ids = rng.integers(0, N_ITEMS, (rows, t)).astype(np.int32)
    counts = rng.choice([0, 1, e - 1, e, 63, 64, 65, 300, 2500], rows)
    counts[0] = 2500 if rows <= 3 else counts[0]
    if rows >= 3:
        ids[1, t // 2] = -1                                           # everything behind it is ignored (t = 1: an empty list)
        counts[2] = 0                                                 # a row without anchors
    if rows >= 70:
        ids[3, :] = -1                                                # an empty list
        counts[4], counts[5], counts[6] = 7, 2500, 65
        ids[69, 0] = -1                                               # the last row: empty from the start, ids behind the -1
    anchors = [rng.integers(0, N_ITEMS, c).astype(np.int32) for c in counts]
    if rows >= 70:
        anchors[4][:] = ids[4, 0]                                     # nothing is eligible for entry 0 of row 4
    ptr = np.zeros(rows + 1, dtype=np.int64)
    np.cumsum(counts, out=ptr[1:])
    return ids, ptr, np.concatenate(anchors).astype(np.int32)


@pytest.mark.parametrize('k', [1, 7, 17, 50, 128, 130, 136, 264, 1000])
def test_exact_arithmetic_with_ties_matches_oracle(k):
    """S entries m / 8 with integer |m| <= 2: every product and sum is exact in fp32 in any order and equal similarities are everywhere,
    so the tie rule decides most results.  best_pos and the bits of best_sim equal the oracle's for EVERY row, among them an empty list,
    a -1 in the middle of a list with ids behind it, a row without anchors, a row whose anchors all equal one of its entries, and an
    empty last row."""
    rng = np.random.Generator(np.random.PCG64(1900 + k))
    S = rng.integers(-2, 3, (N_ITEMS, k)).astype(np.float32) / 8
    full = R.mfma_chain_scores(S, S)                                  # the oracle's similarities, once
    Sd = _dev(S)
    for rows, t, e in PLANS + ([LONG] if k <= 7 else []):
        ids, ptr, cols = _case(rng, rows, t, e)
        want_pos, want_sim, _ = O.nearest(S, ids, ptr, cols, e, N_ITEMS, full=full)
        pos, sim = tkr_hip.nearest_anchors(Sd, _dev(ids), _dev(ptr), _dev(cols), e)
        pos, sim = pos.cpu().numpy(), sim.cpu().numpy()
        assert pos.shape == sim.shape == (rows, t, e) and pos.dtype == np.int32 and sim.dtype == np.float32
        np.testing.assert_array_equal(pos, want_pos, err_msg=str((k, rows, t, e)))
        np.testing.assert_array_equal(_bits(sim), _bits(want_sim), err_msg=str((k, rows, t, e)))
        if rows >= 3:
            assert np.all(pos[1, t // 2:] == -1) and np.all(pos[2] == -1) and np.all(sim[2] == -np.inf)
        if rows >= 70:
            assert np.all(pos[3] == -1) and np.all(pos[69] == -1) and np.all(pos[4, 0] == -1) and np.all(pos[5, :, e - 1] >= 0)
            same = ids[4] == ids[4, 0]
            assert np.all(pos[4][same] == -1) and np.all(pos[4][~same][:, min(e, 7) - 1] >= 0)
        cols_got, _ = explain.explain(Sd, _dev(ids), _dev(ptr), _dev(cols), e)
        np.testing.assert_array_equal(cols_got.cpu().numpy(), O.columns(want_pos, ptr, cols))


def _random_case(seed, k, t, rows, longest):
    """Gaussian factors; a row's list and its history are drawn together without replacement, so they are disjoint; the history holds
    0 ... longest items"""
    rng = np.random.Generator(np.random.PCG64(seed))
    V = rng.standard_normal((N_ITEMS, k)).astype(np.float32)
    ids = np.empty((rows, t), dtype=np.int32)
    hist = []
    for r in range(rows):
        h = int(rng.integers(0, longest + 1))
        drawn = rng.choice(N_ITEMS, t + h, replace=False)
        ids[r] = drawn[:t]
        hist.append(drawn[t:].astype(np.int32))
    ptr = np.zeros(rows + 1, dtype=np.int64)
    np.cumsum([len(h) for h in hist], out=ptr[1:])
    return V, ids, ptr, np.concatenate(hist).astype(np.int32)


@pytest.mark.parametrize('seed,k,t,rows,longest,e', [(1, 50, 30, 300, 40, 3), (2, 128, 30, 300, 150, 3), (3, 24, 40, 300, 7, 8),
                                                     # wide tables on generic floats: an odd width above one tile, a fused width (three
                                                     # k = 128 models with bias), and one above every MFMA form of K4
                                                     (4, 129, 30, 300, 40, 3), (5, 387, 30, 300, 150, 3), (6, 1032, 40, 300, 7, 8)])
def test_random_floats_match_oracle_outside_ambiguous_entries(seed, k, t, rows, longest, e):
    """cosine S from diversity.similarity_table, downloaded and handed to the oracle: every entry without a near-tie (a gap <= 2^-20
    between neighbours among its best e + 1 similarities) has the oracle's positions and the oracle's similarity bits, and at most 0.5 %
    of the entries may have one (a CPU probe of the oracle at these cases marked 1, 0 and 0 of 9,000, 9,000 and 12,000; at k = 129, 387
    and 1032: 3, 5 and 1).  In most rows
    the nearest like is not the same for every entry of the list, and a second call returns the same bits."""
    V, ids, ptr, cols = _random_case(seed, k, t, rows, longest)
    S_d = diversity.similarity_table(_dev(V), 'cosine')
    S = S_d.cpu().numpy()
    np.testing.assert_allclose(np.linalg.norm(S, axis=1), 1.0, rtol=1e-6)
    want_pos, want_sim, amb = O.nearest(S, ids, ptr, cols, e, N_ITEMS)
    print('ambiguous entries: %d of %d' % (amb.sum(), amb.size))
    assert amb.sum() <= 0.005 * amb.size
    args = (S_d, _dev(ids), _dev(ptr), _dev(cols), e)
    pos_d, sim_d = tkr_hip.nearest_anchors(*args)
    pos, sim = pos_d.cpu().numpy(), sim_d.cpu().numpy()
    np.testing.assert_array_equal(pos[~amb], want_pos[~amb])
    np.testing.assert_array_equal(_bits(sim[~amb]), _bits(want_sim[~amb]))
    differs = [len(set(pos[r, :, 0].tolist())) >= 2 for r in range(rows)]
    assert np.mean(differs) > 0.5                                     # the test is not vacuous
    assert np.mean(pos[:, :, 0] >= 0) > 0.7 and np.all(pos[ptr[1:] == ptr[:-1]] == -1)
    again_pos, again_sim = tkr_hip.nearest_anchors(*args)
    assert torch.equal(again_pos, pos_d) and torch.equal(again_sim.view(torch.int32), sim_d.view(torch.int32))
    # unexpectedness of these lists: the float64 loop on the oracle's similarities
    grid = [5, 10, t]
    got = explain.list_unexpectedness(S_d, _dev(ids), _dev(ptr), _dev(cols), grid)
    np.testing.assert_allclose(got, O.unexpectedness_loop(O.nearest(S, ids, ptr, cols, 1, N_ITEMS)[1][:, :, 0], ids, grid), rtol=0, atol=1e-9)
    assert all(0.0 < v < 1.0 for v in got)


def _raw(S, ids, ptr, cols, e):
    """the entry point without the wrapper's status check -> (rc, best_pos, best_sim, status word)"""
    fn = tkr_hip.lib().tkr_nearest_anchors
    pos = torch.full(tuple(ids.shape) + (e,), -7, dtype=torch.int32, device='cuda')
    sim = torch.full(tuple(ids.shape) + (e,), float('nan'), dtype=torch.float32, device='cuda')
    status = torch.zeros(1, dtype=torch.int64, device='cuda')
    p = lambda x: C.c_void_p(x.data_ptr())
    rc = fn(p(S), C.c_int32(S.shape[0]), C.c_int32(S.shape[1]), p(ids), C.c_int32(ids.shape[0]), C.c_int32(ids.shape[1]), p(ptr), p(cols),
            C.c_int64(cols.numel()), C.c_int32(e), p(pos), p(sim), p(status), C.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    return rc, pos.cpu().numpy(), sim.cpu().numpy(), int(status.item())


def test_refused_input_is_reported_and_never_used():
    """a list id >= n_items ends its row, an anchor outside the table is skipped, a descending anchor_ptr empties its row: the wrapper
    raises and names the row (TkrError, TkrError, ValueError); through the bare entry point the status word is the smallest
    4 * row + kind and EVERY row -- the refused ones as defined, all others untouched -- equals the oracle's.  Nothing refused is used as
    an index, so these are ordinary error paths."""
    rng = np.random.Generator(np.random.PCG64(29))
    k, rows, t, e = 16, 9, 40, 3
    S = rng.integers(-2, 3, (N_ITEMS, k)).astype(np.float32) / 8
    ids = rng.integers(0, N_ITEMS, (rows, t)).astype(np.int32)
    counts = np.array([50, 3, 70, 0, 120, 64, 33, 90, 10])
    ptr = np.zeros(rows + 1, dtype=np.int64)
    np.cumsum(counts, out=ptr[1:])
    cols = rng.integers(0, N_ITEMS, int(ptr[-1])).astype(np.int32)
    ids[1, 20], ids[1, 30] = -1, 1 << 30                              # behind the end: ignored, no report
    Sd = _dev(S)

    def check(ids, ptr, cols, word):
        rc, pos, sim, got = _raw(Sd, _dev(ids), _dev(ptr), _dev(cols), e)
        assert rc == 0 and got == word == O.status_word(ids, ptr, cols, N_ITEMS)
        want_pos, want_sim, _ = O.nearest(S, ids, ptr, cols, e, N_ITEMS)
        np.testing.assert_array_equal(pos, want_pos)
        np.testing.assert_array_equal(_bits(sim), _bits(want_sim))
        return pos

    clean = check(ids, ptr, cols, -1)
    assert np.array_equal(tkr_hip.nearest_anchors(Sd, _dev(ids), _dev(ptr), _dev(cols), e)[0].cpu().numpy(), clean)
    # kind 0: list ids outside the table in rows 6 and 4
    bad = ids.copy()
    bad[6, 35], bad[4, 7] = N_ITEMS, 1 << 30
    with pytest.raises(tkr_hip.TkrError, match='row 4'):
        tkr_hip.nearest_anchors(Sd, _dev(bad), _dev(ptr), _dev(cols), e)
    pos = check(bad, ptr, cols, 4 * 4 + 0)
    assert np.all(pos[4, 7:] == -1) and np.all(pos[4, :7] >= 0) and np.all(pos[6, 35:] == -1) and np.array_equal(pos[5], clean[5])
    bad[4, 7] = 3
    check(bad, ptr, cols, 4 * 6 + 0)
    # kind 1: anchors outside the table in rows 2 and 7; their positions stay counted
    badc = cols.copy()
    badc[ptr[2] + 5], badc[ptr[7]], badc[ptr[7] + 89] = N_ITEMS, -1, 1 << 30
    with pytest.raises(tkr_hip.TkrError, match='row 2'):
        tkr_hip.nearest_anchors(Sd, _dev(ids), _dev(ptr), _dev(badc), e)
    pos = check(ids, ptr, badc, 4 * 2 + 1)
    assert not np.any(pos[2] == 5) and not np.any(pos[7] == 0) and not np.any(pos[7] == 89) and np.array_equal(pos[4], clean[4])
    check(bad, ptr, badc, 4 * 2 + 1)                                  # with a kind 0 in row 6: the smallest word
    # kind 3: a descending anchor_ptr (row 4), one that does not start at 0, one that leaves the array
    badp = ptr.copy()
    badp[5] = badp[4] - 1
    with pytest.raises(ValueError, match='row 4'):
        tkr_hip.nearest_anchors(Sd, _dev(ids), _dev(badp), _dev(cols), e)
    pos = check(ids, badp, cols, 4 * 4 + 3)
    assert np.all(pos[4] == -1) and np.array_equal(pos[3], clean[3]) and np.array_equal(pos[6], clean[6])
    badp = ptr.copy()
    badp[0] = 2
    check(ids, badp, cols, 3)
    badp = ptr.copy()
    badp[9] += 1
    pos = check(ids, badp, cols, 4 * 8 + 3)
    assert np.all(pos[8] == -1)


# ---- the command lines, on the g4 fixture copied to tmp_path ----------------------------------------------------------------------
def _g4(golden_dir, tmp_path):
    work = tmp_path / 'g4'
    shutil.copytree(os.path.join(golden_dir, 'g4'), str(work))
    return str(work / 'data'), str(work / 'model')


class _Seen:
    """records what explain.explain is given (the similarity table, the final lists, the anchors) while a command line runs"""

    def __init__(self, monkeypatch):
        self.calls = []
        inner = explain.explain

        def spy(S, ids, anchor_ptr, anchor_cols, e):
            self.calls.append([x.cpu().numpy() for x in (S, ids, anchor_ptr, anchor_cols)] + [e])
            return inner(S, ids, anchor_ptr, anchor_cols, e)
        monkeypatch.setattr(explain, 'explain', spy)


def _liked_by_token(path):
    """uid token -> the like == 1 item tokens of the user's LAST line in a ratings file, by plain string work"""
    out = {}
    for ln in open(path).read().strip().split('\n'):
        f = ln.strip().split(',')
        out[f[0]] = {x.split(':')[0] for x in f[1:] if x.split(':')[1] == '1'}
    return out


def _split(path):
    """an explain file -> per line (uid, [(item token, [(anchor token, '%f' text), ...]), ...])"""
    out = []
    for ln in open(path).read().split('\n')[:-1]:
        f = ln.split(',')
        out.append((f[0], [(x.split(':')[0], list(zip(x.split(':')[1::2], x.split(':')[2::2]))) for x in f[1:]]))
    return out


def _check_explain_file(seen, main_path, why_path, tokens, e, liked):
    """the explain file against the oracle run on what explain.explain was given; the anchors against the ratings files themselves"""
    main = [ln.split(',') for ln in open(main_path).read().split('\n')[:-1]]
    got = _split(why_path)
    assert len(got) == len(main) == sum(len(c[1]) for c in seen.calls)
    at = n_amb = n_entries = 0
    for S, ids, ptr, cols, e_seen in seen.calls:
        assert e_seen == e
        pos, sim, amb = O.nearest(S, ids, ptr, cols, e, len(S))
        users = [m[0] for m in main[at:at + len(ids)]]
        lines, fields = O.explain_lines(users, ids, O.columns(pos, ptr, cols), sim, tokens)
        for r in range(len(ids)):
            uid, why = got[at + r]
            assert uid == users[r] and [i for i, _ in why] == [x.split(':')[0] for x in main[at + r][1:]] == [i for i, _ in fields[r]]
            assert {tokens[int(c)] for c in cols[ptr[r]:ptr[r + 1]]} == {x for x in liked[uid] if x in tokens}, uid
            assert list(cols[ptr[r]:ptr[r + 1]]) == sorted(set(cols[ptr[r]:ptr[r + 1]].tolist()))
            for p, ((item, pairs), (_, want)) in enumerate(zip(why, fields[r])):
                n_entries += 1
                if amb[r, p]:
                    n_amb += 1
                    assert {a for a, _ in pairs} <= {tokens[int(c)] for c in cols[ptr[r]:ptr[r + 1]]} - {item} and len(pairs) == len(want)
                else:
                    assert pairs == want, (uid, item)
            if not amb[r].any():
                assert open(why_path).read().split('\n')[at + r] == lines[r]
        at += len(ids)
    print('ambiguous entries: %d of %d' % (n_amb, n_entries))
    assert n_amb <= 0.005 * n_entries
    return got


def test_recommend_explain_on_golden_g4(golden_dir, tmp_path, monkeypatch):
    import recommend
    data, model = _g4(golden_dir, tmp_path)
    tokens = list(R.read_id_list(os.path.join(data, 'vid')))
    liked = _liked_by_token(os.path.join(data, 'f0tr.txt'))
    base = ['-d', data, '-m', model, '-f', '0', '-t', '30']
    plain, out, why = (str(tmp_path / n) for n in ('plain.txt', 'out.txt', 'why.txt'))
    recommend.main(base + ['-o', plain])
    seen = _Seen(monkeypatch)
    lines = recommend.main(base + ['-o', out, '--explain', '3', '--explain-output', why])
    assert open(out, 'rb').read() == open(plain, 'rb').read() and open(out).read() == '\n'.join(lines) + '\n'
    assert len(seen.calls) == 1
    np.testing.assert_allclose(np.linalg.norm(seen.calls[0][0], axis=1), 1.0, rtol=1e-6)         # cosine by default
    got = _check_explain_file(seen, out, why, tokens, 3, liked)
    # not vacuous: most lines name at least two different nearest likes, no item explains itself, every anchor is a like of the user
    assert np.mean([len({pairs[0][0] for _, pairs in why_ if pairs}) >= 2 for _, why_ in got]) > 0.5
    for uid, why_ in got:
        for item, pairs in why_:
            assert item not in {a for a, _ in pairs} and {a for a, _ in pairs} <= liked[uid] and len(pairs) <= 3
            assert [float(s) for _, s in pairs] == sorted((float(s) for _, s in pairs), reverse=True)
    # --group host and --group device write the same two files
    for where in ('host', 'device'):
        o2, w2 = str(tmp_path / ('out_%s.txt' % where)), str(tmp_path / ('why_%s.txt' % where))
        recommend.main(base + ['-o', o2, '--explain', '3', '--explain-output', w2, '--group', where])
        assert open(o2, 'rb').read() == open(plain, 'rb').read() and open(w2, 'rb').read() == open(why, 'rb').read()
    # --similarity dot: S is V itself
    seen.calls.clear()
    recommend.main(base + ['-o', out, '--explain', '8', '--explain-output', why, '--similarity', 'dot'])
    assert open(out, 'rb').read() == open(plain, 'rb').read()
    assert not np.allclose(np.linalg.norm(seen.calls[0][0], axis=1), 1.0)
    _check_explain_file(seen, out, why, tokens, 8, liked)
    # with --diversify the FINAL lists are explained, and the main output is the one --diversify writes alone
    mmr = str(tmp_path / 'mmr.txt')
    recommend.main(base + ['-o', mmr, '--diversify', '0.7', '--pool', '50'])
    seen.calls.clear()
    recommend.main(base + ['-o', out, '--diversify', '0.7', '--pool', '50', '--explain', '3', '--explain-output', why])
    assert open(out, 'rb').read() == open(mmr, 'rb').read() != open(plain, 'rb').read()
    assert len(seen.calls) == 1 and seen.calls[0][1].shape[1] == 30
    _check_explain_file(seen, out, why, tokens, 3, liked)


def test_recommend_explain_with_candidates_and_new_users(golden_dir, tmp_path, monkeypatch):
    """the funnel is recommend.rank: shortlists and folded-in users are explained too, the new users by their own history file"""
    import recommend
    data, model = _g4(golden_dir, tmp_path)
    users = open(os.path.join(data, 'uid')).read().split()
    tokens = list(R.read_id_list(os.path.join(data, 'vid')))
    liked = _liked_by_token(os.path.join(data, 'f0tr.txt'))
    rng = np.random.Generator(np.random.PCG64(14))
    new = users[-3:]
    open(os.path.join(data, 'uid'), 'w').write('\n'.join(users[:-3]) + '\n')
    (tmp_path / 'new_uid').write_text('\n'.join(new) + '\n')
    fold = ['--new-uid', str(tmp_path / 'new_uid'), '--new-history', os.path.join(data, 'f0tr.txt'), '--seed', '3']
    base = ['-d', data, '-m', model, '-t', '10']
    plain, out, why = (str(tmp_path / n) for n in ('plain.txt', 'out.txt', 'why.txt'))
    recommend.main(base + ['-o', plain] + fold)
    seen = _Seen(monkeypatch)
    recommend.main(base + ['-o', out, '--explain', '3', '--explain-output', why] + fold)
    assert open(out, 'rb').read() == open(plain, 'rb').read() and len(seen.calls) == 2          # the model's users, then the new ones
    got = _check_explain_file(seen, out, why, tokens, 3, liked)
    assert [g[0] for g in got] == users
    asked = [users[x] for x in rng.permutation(len(users) - 3)[:40]] + [new[1], users[2], new[0]]
    lists = [[tokens[c] for c in rng.choice(len(tokens), int(rng.integers(5, 90)), replace=False)] for _ in asked]
    cand = tmp_path / 'cand'
    cand.write_text(''.join('%s,%s\n' % (u, ','.join('%s:1' % v for v in l)) for u, l in zip(asked, lists)))
    recommend.main(base + ['-o', plain, '--candidates', str(cand)] + fold)
    seen.calls.clear()
    recommend.main(base + ['-o', out, '--candidates', str(cand), '--explain', '3', '--explain-output', why] + fold)
    assert open(out, 'rb').read() == open(plain, 'rb').read() and len(seen.calls) == 2
    got = _check_explain_file(seen, out, why, tokens, 3, liked)
    order = [i for i, u in enumerate(asked) if u not in new] + [i for i, u in enumerate(asked) if u in new]
    assert [g[0] for g in got] == [asked[i] for i in order]
    assert any(len(g[1]) < 10 for g in got)                           # short shortlists: the padding was met


def test_recommend_explain_with_new_items(golden_dir, tmp_path, monkeypatch):
    """--new-vid: G4 with its last five items cut out of vid and final-V.dat and folded back in (the recipe of tests/test_gpu_item_foldin.py).
    The table is the grown catalogue's, and a user's anchors are the likes of the history line AND of the user's last line of
    --new-ratings, the two sources whose items the line excludes"""
    import recommend
    src_data, src_model = os.path.join(golden_dir, 'g4', 'data'), os.path.join(golden_dir, 'g4', 'model')
    data, model = tmp_path / 'data', tmp_path / 'model'
    shutil.copytree(src_data, str(data))
    model.mkdir()
    tokens = open(os.path.join(src_data, 'vid')).read().split()
    (data / 'vid').write_text('\n'.join(tokens[:-5]) + '\n')
    shutil.copy(os.path.join(src_model, 'final-U.dat'), str(model / 'final-U.dat'))
    rows = open(os.path.join(src_model, 'final-V.dat')).read().strip('\n').split('\n')
    (model / 'final-V.dat').write_text('\n'.join(rows[:-5]) + '\n')
    (tmp_path / 'new_vid').write_text('\n'.join(tokens[-5:]) + '\n')
    new_ratings = tmp_path / 'new_ratings'
    new_ratings.write_text(open(os.path.join(src_data, 'f0tr.txt')).read() + open(os.path.join(src_data, 'f0te.om.txt')).read())
    base = ['-d', str(data), '-m', str(model), '-t', '10', '--new-vid', str(tmp_path / 'new_vid'), '--new-ratings', str(new_ratings), '--seed', '3']
    plain, out, why = (str(tmp_path / n) for n in ('plain.txt', 'out.txt', 'why.txt'))
    recommend.main(base + ['-o', plain])
    seen = _Seen(monkeypatch)
    recommend.main(base + ['-o', out, '--explain', '3', '--explain-output', why])
    assert open(out, 'rb').read() == open(plain, 'rb').read() and len(seen.calls) == 1
    assert seen.calls[0][0].shape[0] == len(tokens)                   # the grown catalogue
    first, second = _liked_by_token(os.path.join(src_data, 'f0tr.txt')), _liked_by_token(str(new_ratings))
    liked = {u: first.get(u, set()) | second.get(u, set()) for u in set(first) | set(second)}
    assert any(second[u] - first.get(u, set()) for u in second)      # the second source adds anchors
    _check_explain_file(seen, out, why, tokens, 3, liked)


def test_evaluate_unexpectedness_on_golden_g4(golden_dir, tmp_path, monkeypatch, capsys):
    import evaluate as E
    data, model = _g4(golden_dir, tmp_path)
    scs = ['im', 'om']
    args = ['-d', data, '-m', model, '-s', '5', '-t', '30', '-sl'] + scs
    before = E.main(args + ['-M', 'acc', 'ild'])
    capsys.readouterr()
    seen = _Seen(monkeypatch)
    values = []
    inner = explain.unexpectedness
    monkeypatch.setattr(explain, 'unexpectedness', lambda sims0, ids, grid: (values.append(inner(sims0, ids, grid)), values[-1])[1])
    got = E.main(args + ['-M', 'acc', 'ild', 'unexp'])
    assert capsys.readouterr().out.strip().split('\n') == got
    assert [l for l in got if '.unexp' not in l] == before            # every other line: unchanged, in place
    assert [l.split(',')[0] for l in got[-4:]] == ['im.ild', 'im.unexp', 'om.ild', 'om.unexp']       # after the scenario's ild line
    grid = [5, 10, 15, 20, 25, 30]
    vids = R.read_id_list(os.path.join(data, 'vid'))
    tokens = list(vids)
    liked = _liked_by_token(os.path.join(data, 'f0tr.txt'))
    uid_tokens = list(R.read_id_list(os.path.join(data, 'uid')))
    V = np.loadtxt(os.path.join(model, 'final-V.dat'), dtype=np.float32)
    assert len(seen.calls) == len(scs) == len(values)
    for q, sc in enumerate(scs):
        S, ids, ptr, cols, e = seen.calls[q]
        assert e == 1 and S.shape == V.shape and ids.shape[1] == 30   # the table of the whole final-V.dat, the lists in vid rows
        teids = set(R.read_id_list(os.path.join(data, 'f0te.%s.idl' % sc)))
        assert {tokens[int(c)] for c in ids[ids >= 0]} <= teids
        full = E.load_scenario(data, 0, sc, R.read_id_list(os.path.join(data, 'uid')))
        for r, u in enumerate(full.users):
            assert {tokens[int(c)] for c in cols[ptr[r]:ptr[r + 1]]} == {x for x in liked[uid_tokens[int(u)]] if x in vids}
        _, sim, _ = O.nearest(S, ids, ptr, cols, 1, len(S))
        want = O.unexpectedness_loop(sim[:, :, 0], ids, grid)
        np.testing.assert_allclose(values[q], want, rtol=0, atol=1e-9)
        line = [l for l in got if l.startswith('%s.unexp,' % sc)]
        assert len(line) == 1 and line[0].split(',')[1:] == ['%.6f' % v for v in values[q]]
    # with --diversify the re-ranked lists get their own line
    seen.calls.clear()
    del values[:]
    mmr = E.main(args + ['-M', 'acc', 'ild', 'unexp', '--diversify', '0.7'])
    names = [l.split(',')[0] for l in mmr]
    assert all('%s.mmr.unexp' % sc in names and '%s.unexp' % sc in names for sc in scs) and len(seen.calls) == 2 * len(scs)
    value = {l.split(',')[0]: [float(v) for v in l.split(',')[1:]] for l in mmr}
    for sc in scs:
        assert value['%s.unexp' % sc] == [float(v) for v in [l for l in got if l.startswith('%s.unexp,' % sc)][0].split(',')[1:]]
        # (no order between the two is asserted: on this fixture the re-ranked 'im' lists measured 0.569237 against 0.571310 at 30 --
        # MMR spreads a list's items apart from each other, which need not move them away from the user's 5-10 training likes)
        print(sc, 'unexp', value['%s.unexp' % sc][-1], 'mmr.unexp', value['%s.mmr.unexp' % sc][-1])
        assert all(0.0 <= v <= 2.0 for v in value['%s.mmr.unexp' % sc])
