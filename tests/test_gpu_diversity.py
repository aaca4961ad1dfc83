"""K17 (tkr_mmr_select, tkr_list_pair_sums; csrc/diversity.hip), diversity.py, recommend.py --diversify and evaluate.py -M ild cov gini
--diversify on the GPU, against tests/_diversity_oracle.py.  Picks are integers and compared exactly; pair sums to 1e-9."""
import ctypes as C
import os
import shutil
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _diversity_oracle as O

import diversity
import tkr_hip
from oracle import ref_np as R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N_ITEMS = 600
# (rows, N, t, lambda): every N of 1, 2, 63, 64, 65, 100, 129, 256, 1024 (one wave, more than one, the largest workgroup), every t of
# 1, 5, 30, N, and 1, 3, 70 rows; lambda 0 and 1 among them.  Rows of 1024 x 4 k bytes do not fit the LDS: the form that reads through L2
# runs there at every k, from 63 entries at k = 1000 and from 256 at k = 264; the staged form everywhere else
PLANS = [(1, 1, 1, 0.5), (3, 2, 2, 0.25), (70, 63, 5, 0.75), (3, 64, 64, 0.0), (70, 65, 30, 0.5), (70, 100, 30, 0.75), (3, 100, 1, 0.0),
         (3, 129, 129, 0.25), (70, 256, 30, 1.0), (1, 256, 256, 0.5), (3, 1024, 30, 0.5)]
LONG = (1, 1024, 1024, 0.75)                                          # t = N = 1024: where the chain is short (k = 1, 7)


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to('cuda')


def _pool(rng, rows, N, t):
    """ids int32 [rows, N] with replacement (duplicated ids) and the rows the kernel must get right: no valid entry, fewer than t,
    fewer than N, a -1 in the middle with ids behind it, one id twice in front"""
    ids = rng.integers(0, N_ITEMS, (rows, N)).astype(np.int32)
    if rows >= 3 and N >= 8:
        ids[1, N // 2] = -1                                           # everything behind it is ignored
        ids[2, N - 3:] = -1
        ids[2, 1] = ids[2, 0]
    if rows >= 70:
        ids[3, :] = -1
        ids[4, max(t - 1, 0):] = -1                                   # t - 1 valid entries
        ids[5, 1:] = -1                                               # a single entry
        ids[69, 0] = -1                                               # the last row: empty from the start, ids behind the -1
    return ids


@pytest.mark.parametrize('k', [1, 7, 17, 50, 128, 130, 136, 264, 1000])
def test_exact_arithmetic_with_ties_matches_oracle(k):
    """S entries m / 8 with integer |m| <= 2, rel entries q / 64, lambda a multiple of 1/4: every product and sum is exact in fp32 in any
    order and equal objectives are everywhere, so the tie rule decides most picks.  sel_pos equals the oracle's for EVERY row, and the
    pair sums of the same ids, read as lists, equal the float64 oracle's to 1e-9."""
    rng = np.random.Generator(np.random.PCG64(1700 + k))
    S = rng.integers(-2, 3, (N_ITEMS, k)).astype(np.float32) / 8
    full = R.mfma_chain_scores(S, S)                                  # the oracle's similarities, once
    Sd = _dev(S)
    for rows, N, t, lam in PLANS + ([LONG] if k <= 7 else []):
        ids = _pool(rng, rows, N, t)
        rel = rng.integers(0, 65, (rows, N)).astype(np.float32) / 64
        want, _ = O.mmr(S, ids, rel, lam, t, N_ITEMS, full=full)
        got = tkr_hip.mmr_select(Sd, _dev(ids), _dev(rel), lam, t).cpu().numpy()
        np.testing.assert_array_equal(got, want, err_msg=str((k, rows, N, t, lam)))
        ps = tkr_hip.list_pair_sums(Sd, _dev(ids)).cpu().numpy()
        np.testing.assert_allclose(ps, O.pair_sums(S, ids, N_ITEMS, full=full), rtol=0, atol=1e-9, err_msg=str((k, rows, N)))
        if rows >= 70:
            assert np.all(got[3] == -1) and np.all(got[69] == -1) and got[4, t - 1] == -1 and (t < 2 or got[4, t - 2] >= 0)


def _random_case(seed, n_items, k, N, rows):
    """Gaussian factors; the pool of a row is a random user's N best of a random half of the catalogue, best first, with its scores"""
    rng = np.random.Generator(np.random.PCG64(seed))
    V = rng.standard_normal((n_items, k)).astype(np.float32)
    U = rng.standard_normal((rows, k)).astype(np.float32)
    ids = np.empty((rows, N), dtype=np.int32)
    scores = np.empty((rows, N), dtype=np.float32)
    for r in range(rows):
        c = rng.choice(n_items, n_items // 2, replace=False)
        s = V[c] @ U[r]
        order = np.argsort(-s, kind='stable')[:N]
        ids[r], scores[r] = c[order], s[order]
    return V, ids, scores


@pytest.mark.parametrize('seed,n_items,k,N,t,rows,lam', [(1, 600, 50, 96, 30, 300, 0.7), (2, 600, 128, 64, 30, 300, 0.5), (3, 600, 24, 130, 40, 300, 0.7),
                                                         # wide tables on generic floats: an odd width above one tile, a fused width
                                                         # (three k = 128 models with bias), and one whose 64 rows do not fit the LDS
                                                         (4, 600, 129, 96, 30, 300, 0.7), (5, 600, 387, 64, 30, 300, 0.5), (6, 600, 1032, 64, 30, 300, 0.7)])
def test_random_floats_match_oracle_outside_ambiguous_rows(seed, n_items, k, N, t, rows, lam):
    """cosine S and rel from diversity.prepare, downloaded and handed to the oracle: every row without a near-tie (a gap <= 2^-20 between
    the two best objectives of a pick) equals the oracle exactly, and at most 2 % of the rows may have one (a float64 NumPy probe at
    these shapes marked 2, 0 and 0 of 300; the oracle on these pools marks 0, 1 and 1; at k = 129, 387 and 1032 a CPU run of the oracle
    marked 0, 2 and 1).  The pick order differs from the score order in most rows, lambda = 1 gives the pool's
    first t entries back, and the pair sums of the picked lists match the float64 oracle."""
    V, ids, scores = _random_case(seed, n_items, k, N, rows)
    ids_d, scores_d = _dev(ids), _dev(scores)
    S_d, rel_d = diversity.prepare(_dev(V), ids_d, scores_d, 'cosine')
    S, rel = S_d.cpu().numpy(), rel_d.cpu().numpy()
    np.testing.assert_allclose(np.linalg.norm(S, axis=1), 1.0, rtol=1e-6)
    assert rel.min() == 0.0 and rel.max() == 1.0 and np.all(rel[:, 0] == 1.0)
    full = R.mfma_chain_scores(S, S) if k > 256 else None             # wide tables: the oracle's similarities once, not per row
    want, amb = O.mmr(S, ids, rel, lam, t, n_items, full=full)
    print('ambiguous rows: %d of %d' % (amb.sum(), rows))
    assert amb.sum() <= 0.02 * rows
    got = tkr_hip.mmr_select(S_d, ids_d, rel_d, lam, t).cpu().numpy()
    np.testing.assert_array_equal(got[~amb], want[~amb])
    assert np.mean(np.any(got != np.arange(t), axis=1)) > 0.9         # not the score order: the test is not vacuous
    out_ids, out_scores = diversity.rerank(S_d, rel_d, ids_d, scores_d, lam, t)
    np.testing.assert_array_equal(out_ids.cpu().numpy(), np.take_along_axis(ids, got, 1))
    np.testing.assert_array_equal(out_scores.cpu().numpy(), np.take_along_axis(scores, got, 1))
    same_ids, same_scores = diversity.rerank(S_d, rel_d, ids_d, scores_d, 1.0, t)
    np.testing.assert_array_equal(same_ids.cpu().numpy(), ids[:, :t])
    np.testing.assert_array_equal(same_scores.cpu().numpy(), scores[:, :t])
    ps = tkr_hip.list_pair_sums(S_d, out_ids).cpu().numpy()
    np.testing.assert_allclose(ps, O.pair_sums(S, out_ids.cpu().numpy(), n_items, full=full), rtol=0, atol=1e-9)
    m = diversity.list_metrics(S_d, out_ids, n_items, [5, 10, t])
    w = O.metrics_loop(ps, out_ids.cpu().numpy(), n_items, [5, 10, t])
    for name in m:
        np.testing.assert_allclose(m[name], w[name], rtol=1e-12, atol=1e-15)
    plain = diversity.list_metrics(S_d, ids_d[:, :t].contiguous(), n_items, [t])
    assert m['ild'][-1] > plain['ild'][0]                             # what the re-ranking is for


def _raw(lib_fn, S, ids, rel, lam, t):
    """the entry point without the wrapper's status check -> (sel_pos, status word)"""
    sel = torch.full((ids.shape[0], t), -7, dtype=torch.int32, device='cuda')
    status = torch.zeros(1, dtype=torch.int64, device='cuda')
    p = lambda x: C.c_void_p(x.data_ptr())
    rc = lib_fn(p(S), C.c_int32(S.shape[0]), C.c_int32(S.shape[1]), p(ids), p(rel), C.c_int32(ids.shape[0]), C.c_int32(ids.shape[1]),
                C.c_double(lam), C.c_int32(t), p(sel), p(status), C.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    return rc, sel.cpu().numpy(), int(status.item())


def test_out_of_range_ids_end_the_row_and_are_reported():
    """a row holding an id equal to n_items and one holding 2^30: TkrError from the wrappers; through the bare entry point the status
    word names the first such row, those rows end at that id and every other row of the call is the oracle's.  An id out of range
    BEHIND a row's -1 is not looked at."""
    rng = np.random.Generator(np.random.PCG64(23))
    k, rows, N, t = 16, 9, 70, 20
    S = rng.integers(-2, 3, (N_ITEMS, k)).astype(np.float32) / 8
    ids = rng.integers(0, N_ITEMS, (rows, N)).astype(np.int32)
    rel = rng.integers(0, 65, (rows, N)).astype(np.float32) / 64
    ids[1, 40], ids[1, 50] = -1, 1 << 30                              # behind the end: ignored, no report
    clean = tkr_hip.mmr_select(_dev(S), _dev(ids), _dev(rel), 0.5, t).cpu().numpy()
    np.testing.assert_array_equal(clean, O.mmr(S, ids, rel, 0.5, t, N_ITEMS)[0])
    ids[6, 65] = N_ITEMS
    ids[4, 7] = 1 << 30
    Sd, idd, reld = _dev(S), _dev(ids), _dev(rel)
    with pytest.raises(tkr_hip.TkrError, match='row 4'):
        tkr_hip.mmr_select(Sd, idd, reld, 0.5, t)
    with pytest.raises(tkr_hip.TkrError, match='row 4'):
        tkr_hip.list_pair_sums(Sd, idd)
    fn = tkr_hip.lib().tkr_mmr_select
    rc, sel, word = _raw(fn, Sd, idd, reld, 0.5, t)
    assert rc == 0 and word == 4 * 4 + 1
    want = O.mmr(S, ids, rel, 0.5, t, N_ITEMS)[0]
    np.testing.assert_array_equal(sel, want)
    assert np.all(sel[4, 7:] == -1) and np.all(sel[4, :7] >= 0) and np.all(sel[6] >= 0) and np.all(sel[6] < 65)
    ids[4, 7] = 3                                                     # only row 6 is left
    rc, sel, word = _raw(fn, Sd, _dev(ids), reld, 0.5, t)
    assert rc == 0 and word == 4 * 6 + 1


def test_raw_abi_through_ctypes():
    """the symbol as a maintainer of the reference would bind it: no helper module in between"""
    lib = C.CDLL(os.path.join(ROOT, 'top-k-rec_amd', 'libtkr_hip.so'))
    fn = lib.tkr_mmr_select
    fn.restype = C.c_int
    fn.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_double, C.c_int32, C.c_void_p, C.c_void_p,
                   C.c_void_p]
    rng = np.random.Generator(np.random.PCG64(4))
    k, rows, N, t = 24, 11, 90, 25
    S = rng.integers(-2, 3, (N_ITEMS, k)).astype(np.float32) / 8
    ids = rng.integers(0, N_ITEMS, (rows, N)).astype(np.int32)
    ids[3, 10:] = -1
    rel = rng.integers(0, 65, (rows, N)).astype(np.float32) / 64
    Sd, idd, reld = _dev(S), _dev(ids), _dev(rel)
    sel = torch.empty((rows, t), dtype=torch.int32, device='cuda')
    status = torch.zeros(1, dtype=torch.int64, device='cuda')
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    p = lambda x: C.c_void_p(x.data_ptr())
    good = [p(Sd), N_ITEMS, k, p(idd), p(reld), rows, N, 0.25, t, p(sel), p(status), stream]
    assert fn(*good) == 0
    torch.cuda.synchronize()
    assert int(status.item()) == -1
    np.testing.assert_array_equal(sel.cpu().numpy(), O.mmr(S, ids, rel, 0.25, t, N_ITEMS)[0])
    for at, bad in ((0, None), (3, None), (4, None), (9, None), (10, None), (1, 0), (2, 0), (5, 0), (6, 0), (8, 0), (8, N + 1), (7, 1.5), (7, float('nan'))):
        args = list(good)
        args[at] = bad
        assert fn(*args) == -1, at
    torch.cuda.synchronize()


# ---- the command lines, on the g4 fixture copied to tmp_path ----------------------------------------------------------------------
def _g4(golden_dir, tmp_path):
    work = tmp_path / 'g4'
    shutil.copytree(os.path.join(golden_dir, 'g4'), str(work))
    return str(work / 'data'), str(work / 'model')


def _parse_lines(path):
    out = []
    for ln in open(path).read().strip().split('\n'):
        f = ln.split(',')
        out.append((f[0], [t.split(':')[0] for t in f[1:]], [t.split(':')[1] for t in f[1:]]))
    return out


class _Seen:
    """records what diversity.rerank is given (K4's / K12's pool, prepare's S and rel) while the command line runs"""

    def __init__(self, monkeypatch):
        self.calls = []
        inner = diversity.rerank

        def rerank(S, rel, ids, scores, lam, t):
            self.calls.append([x.cpu().numpy() for x in (S, rel, ids, scores)] + [lam, t])
            return inner(S, rel, ids, scores, lam, t)
        monkeypatch.setattr(diversity, 'rerank', rerank)

    def oracle_lines(self, tokens):
        """per call: (the lines' item tokens and '%f' scores the oracle picks, ambiguous rows)"""
        out = []
        for S, rel, ids, scores, lam, t in self.calls:
            sel, amb = O.mmr(S, ids, rel, lam, t, len(S))
            rows = []
            for r in range(len(ids)):
                at = sel[r][sel[r] >= 0]
                rows.append(([tokens[int(c)] for c in ids[r, at]], ['%f' % float(s) for s in scores[r, at]]))
            out.append((rows, amb))
        return out


def _check_against_oracle(seen, got, tokens, pool):
    want = [(row, a) for rows, amb in seen.oracle_lines(tokens) for row, a in zip(rows, amb)]
    assert len(want) == len(got) and all(c[2].shape[1] == pool for c in seen.calls)
    n_amb = sum(1 for _, a in want if a)
    print('ambiguous lines: %d of %d' % (n_amb, len(want)))
    assert n_amb <= 0.02 * len(want)
    for (row, a), g in zip(want, got):
        if not a:
            assert (g[1], g[2]) == row, g[0]


def test_recommend_diversify_on_golden_g4(golden_dir, tmp_path, monkeypatch):
    import recommend
    data, model = _g4(golden_dir, tmp_path)
    tokens = list(R.read_id_list(os.path.join(data, 'vid')))
    base = ['-d', data, '-m', model, '-f', '0', '-t', '30']
    plain, same, out, pool50 = (str(tmp_path / n) for n in ('plain.txt', 'same.txt', 'mmr.txt', 'pool.txt'))
    recommend.main(base + ['-o', plain])
    recommend.main(base + ['-o', same, '--diversify', '1'])           # lambda = 1: the file written without the flag, byte for byte
    assert open(same, 'rb').read() == open(plain, 'rb').read()
    seen = _Seen(monkeypatch)
    lines = recommend.main(base + ['-o', out, '--diversify', '0.7', '--pool', '50'])
    got = _parse_lines(out)
    assert open(out).read() == '\n'.join(lines) + '\n' and len(seen.calls) == 1
    _check_against_oracle(seen, got, tokens, 50)
    # the pool is K4's: the lines of -t 50; a re-ranked line holds 30 of its 50 items, the best one first, and most lines changed
    recommend.main(base[:-1] + ['50', '-o', pool50])
    before = _parse_lines(plain)
    changed = 0
    for g, p, b in zip(got, _parse_lines(pool50), before):
        assert g[0] == p[0] and set(g[1]) <= set(p[1]) and len(g[1]) == min(30, len(p[1])) and g[1][0] == p[1][0]
        changed += g[1] != b[1]
    assert changed > 0.5 * len(got)
    seen.calls.clear()
    recommend.main(base + ['-o', out, '--diversify', '0.7', '--pool', '50', '--similarity', 'dot'])
    _check_against_oracle(seen, _parse_lines(out), tokens, 50)
    assert not np.allclose(np.linalg.norm(seen.calls[0][0], axis=1), 1.0)          # S is V itself


def test_recommend_diversify_with_candidates_and_new_users(golden_dir, tmp_path, monkeypatch):
    """the funnel is recommend.rank: shortlists (K12's pool, shorter than --pool: padded) and folded-in users get the same re-ranking"""
    import recommend
    data, model = _g4(golden_dir, tmp_path)
    users = open(os.path.join(data, 'uid')).read().split()
    tokens = list(R.read_id_list(os.path.join(data, 'vid')))
    rng = np.random.Generator(np.random.PCG64(12))
    new = users[-3:]
    open(os.path.join(data, 'uid'), 'w').write('\n'.join(users[:-3]) + '\n')
    (tmp_path / 'new_uid').write_text('\n'.join(new) + '\n')
    fold = ['--new-uid', str(tmp_path / 'new_uid'), '--new-history', os.path.join(data, 'f0tr.txt'), '--seed', '3']
    base = ['-d', data, '-m', model, '-t', '10', '--diversify', '0.7', '--pool', '50']
    out = str(tmp_path / 'out.txt')
    seen = _Seen(monkeypatch)
    recommend.main(base + ['-o', out] + fold)
    got = _parse_lines(out)
    assert [g[0] for g in got] == users and len(seen.calls) == 2      # the model's users, then the new ones
    _check_against_oracle(seen, got, tokens, 50)
    asked = [users[x] for x in rng.permutation(len(users) - 3)[:40]] + [new[1], users[2], new[0]]
    lists = [[tokens[c] for c in rng.choice(len(tokens), int(rng.integers(5, 90)), replace=False)] for _ in asked]
    cand = tmp_path / 'cand'
    cand.write_text(''.join('%s,%s\n' % (u, ','.join('%s:1' % v for v in l)) for u, l in zip(asked, lists)))
    seen.calls.clear()
    recommend.main(base + ['-o', out, '--candidates', str(cand)] + fold)
    got = _parse_lines(out)
    order = [i for i, u in enumerate(asked) if u not in new] + [i for i, u in enumerate(asked) if u in new]
    assert [g[0] for g in got] == [asked[i] for i in order] and len(seen.calls) == 2
    _check_against_oracle(seen, got, tokens, 50)
    for g, i in zip(got, order):
        assert set(g[1]) <= set(lists[i]) and len(g[1]) <= 10
    assert any(len(g[1]) < 10 for g in got) or any(np.any(c[2] < 0) for c in seen.calls)       # short shortlists: the padding was met


def test_evaluate_list_metrics_and_diversify_on_golden_g4(golden_dir, tmp_path, monkeypatch, capsys):
    import evaluate as E
    data, model = _g4(golden_dir, tmp_path)
    scs = ['im', 'om']
    args = ['-d', data, '-m', model, '-s', '5', '-t', '30', '-sl'] + scs
    before = E.main(args + ['-M', 'acc'])
    capsys.readouterr()
    seen = _Seen(monkeypatch)
    pairs = []
    inner = tkr_hip.list_pair_sums
    monkeypatch.setattr(tkr_hip, 'list_pair_sums', lambda S, ids: (pairs.append((S.cpu().numpy(), ids.cpu().numpy())), inner(S, ids))[1])
    got = E.main(args + ['-M', 'acc', 'ild', 'cov', 'gini', '--diversify', '0.7'])
    assert capsys.readouterr().out.strip().split('\n') == got
    assert got[:len(before)] == before                                # the old lines: unchanged, and first
    new = got[len(before):]
    names = ['%s.%s' % (sc, m) for sc in scs for m in ('ild', 'cov', 'gini')] + ['%s.mmr.%s' % (sc, m) for sc in scs for m in ('acc', 'ild', 'cov', 'gini')]
    assert [l.split(',')[0] for l in new] == names
    value = {l.split(',')[0]: l.split(',')[1:] for l in new}
    grid = [5, 10, 15, 20, 25, 30]
    uids = R.read_id_list(os.path.join(data, 'uid'))
    assert len(seen.calls) == len(scs) and len(pairs) == 2 * len(scs)
    for q, sc in enumerate(scs):
        S, rel, pool, scores, lam, t = seen.calls[q]
        assert pool.shape[1] == 100 and lam == 0.7 and t == 30
        n_cols = len(S)
        (S0, plain), (S1, picked) = pairs[2 * q], pairs[2 * q + 1]
        np.testing.assert_array_equal(S0, S)
        np.testing.assert_array_equal(plain, pool[:, :30])            # the ordinary lists are the head of the pool
        sel, amb = O.mmr(S, pool, rel, lam, t, n_cols)
        assert amb.sum() <= 0.02 * len(pool)
        want_lists = np.where(sel >= 0, np.take_along_axis(pool, np.maximum(sel, 0), 1), -1)
        np.testing.assert_array_equal(picked[~amb], want_lists[~amb])
        want_lists[amb] = picked[amb]                                 # either order is right there
        for tag, lists in (('', plain), ('mmr.', want_lists)):
            w = O.metrics_loop(O.pair_sums(S, lists, n_cols), lists, n_cols, grid)
            for m in ('ild', 'cov', 'gini'):
                assert value['%s.%s%s' % (sc, tag, m)] == ['%.6f' % v for v in w[m]], (sc, tag, m)
        full = E.load_scenario(data, 0, sc, uids)
        hits = np.zeros(6)
        for r in range(len(full.users)):
            likes = set(full.like_cols[full.like_ptr[r]:full.like_ptr[r + 1]].tolist())
            hits += R.bucket_hits([int(c) for c in want_lists[r] if c >= 0], likes, 5, 6)
        assert value['%s.mmr.acc' % sc] == ['%.6f' % (h / full.tcount) for h in hits]
        assert float(value['%s.mmr.ild' % sc][-1]) >= float(value['%s.ild' % sc][-1])
    # --diversify alone prints the accuracy of the re-ranked lists and nothing else new
    alone = E.main(args + ['--diversify', '0.7'])
    assert alone[:len(scs)] == before[:len(scs)] and alone[len(scs):] == [l for l in new if '.mmr.acc' in l]
