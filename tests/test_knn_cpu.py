"""K28 / K29 without a GPU: the oracle of tests/test_gpu_knn.py (tests/_knn_oracle.py) against a second, dense restatement written
another way, the symbols of include/tkr.h, what knn.ItemKNN stores and refuses, and the flags evaluate.py and recommend.py refuse for a
neighbourhood model before they look for a GPU."""
import ctypes
import functools
import math
import os
import re

import numpy as np
import pytest

import _knn_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G2 = os.path.join(ROOT, 'tests', 'golden', 'g2')


def g2_likes():
    """-> (u_ptr, u_cols, i_ptr, i_rows, n_users, n_items) of the like == 1 entries of g2's train file"""
    import foldin
    import textio
    from utils import get_id_dict_from_file
    uids, vids = get_id_dict_from_file(os.path.join(G2, 'uid')), get_id_dict_from_file(os.path.join(G2, 'vid'))
    R = textio.parse_ratings(os.path.join(G2, 'f0tr.txt'), uids, vids)
    up, uc = foldin.liked_csr(R, len(uids), len(vids), by='user')
    ip, ir = foldin.liked_csr(R, len(vids), len(uids), by='item')
    return up, uc, ip, ir, len(uids), len(vids)


def _zipf(n_users, n_items, seed, mean=12):
    rng = np.random.Generator(np.random.PCG64(seed))
    pop = np.arange(1, n_items + 1, dtype=np.float64) ** -0.9
    pop /= pop.sum()
    rows = [rng.choice(n_items, size=min(n_items, int(rng.integers(0, 2 * mean))), replace=False, p=pop) for _ in range(n_users)]
    return O.csr(rows, n_users)


# ---- a second restatement: python sets, python floats, sorted() with a key -------------------------------------------------------------
def _build_again(u_ptr, u_cols, n_items, norm, shrink, N):
    likers = [set() for _ in range(n_items)]
    for u in range(len(u_ptr) - 1):
        for c in u_cols[u_ptr[u]:u_ptr[u + 1]]:
            likers[int(c)].add(u)
    ids, w = np.full((n_items, N), -1, np.int32), np.zeros((n_items, N), np.float32)
    for i in range(n_items):
        cand = []
        for j in range(n_items):
            c = len(likers[i] & likers[j])
            if j != i and c > 0:
                cand.append((np.float32(c / (float(norm[i]) * float(norm[j]) + shrink)), j))      # python floats are IEEE fp64
        cand.sort(key=lambda x: (-float(x[0]), -x[1]))
        for p, (s, j) in enumerate(cand[:N]):
            ids[i, p], w[i, p] = j, s
    return ids, w


def _score_again(hist, nbr_ids, nbr_w, col_of_item, n_cols, masked, K, likes):
    """one line: the dense W of the table, the chain as np.float32 additions, python sorting"""
    n_items = len(nbr_ids)
    s = [np.float32(0)] * n_cols
    for i in sorted(hist):
        W = {int(j): wt for j, wt in zip(nbr_ids[i], nbr_w[i]) if j >= 0}
        for j in range(n_items):
            c = j if col_of_item is None else int(col_of_item[j])
            if c >= 0 and j in W:
                s[c] = np.float32(s[c] + W[j])
    kept = sorted((c for c in range(n_cols) if not masked[c]), key=lambda c: (-float(s[c]), -c))
    rank = [kept.index(l) if 0 <= l < n_cols and not masked[l] else -1 for l in likes]
    return kept[:K], [s[c] for c in kept[:K]], rank


def test_g2_is_the_fixture_the_gpu_tests_say_it_is():
    up, uc, ip, ir, n_users, n_items = g2_likes()
    assert (n_users, n_items) == (40, 30)
    assert int((np.diff(up) == 0).sum()) == 3 and int((np.diff(ip) == 0).sum()) == 4
    tp, tr = O.transpose(up, uc, n_items)
    np.testing.assert_array_equal(tp, ip)
    np.testing.assert_array_equal(tr, ir)
    _, _, C, sim = O.build(up, uc, n_items, O.norms(np.diff(ip), 'cosine'), 0.0, 5)
    tied = 0
    for i in range(n_items):
        cand = [j for j in range(n_items) if j != i and C[i, j] > 0]
        tied += len(cand) - len(set(sim[i, cand].tolist()))
    assert tied == 51                                             # similarities equal to an earlier one of their row: the tie rule is exercised


@pytest.mark.parametrize('similarity,shrink,N', [('cosine', 0.0, 5), ('cosine', 2.5, 40), ('cooc', 0.0, 7)])
def test_build_oracle_against_the_second_restatement(similarity, shrink, N):
    for up, uc, n_items in (g2_likes()[:2] + (30,), _zipf(60, 37, 3) + (37,)):
        ip, _ = O.transpose(up, uc, n_items)
        norm = O.norms(np.diff(ip), similarity)
        ids, w, C, _ = O.build(up, uc, n_items, norm, shrink, N)
        ids2, w2 = _build_again(up, uc, n_items, norm, shrink, N)
        np.testing.assert_array_equal(ids, ids2)
        np.testing.assert_array_equal(w.view(np.int32), w2.view(np.int32))
        assert (C == C.T).all() and (np.diag(C) == np.diff(ip)).all()
        if similarity == 'cooc':
            assert all(w[i, p] == C[i, ids[i, p]] for i in range(n_items) for p in range(N) if ids[i, p] >= 0)


def test_score_oracle_against_the_second_restatement():
    up, uc, ip, ir, n_users, n_items = g2_likes()
    ids, w, _, _ = O.build(up, uc, n_items, O.norms(np.diff(ip), 'cosine'), 0.0, 5)
    rng = np.random.Generator(np.random.PCG64(29))
    col_of_item = np.full(n_items, -1, np.int32)
    keep = np.sort(rng.permutation(n_items)[:21])
    col_of_item[keep] = rng.permutation(21)
    rated = O.csr([rng.permutation(21)[:rng.integers(0, 6)] for _ in range(n_users)], n_users)
    likes = O.csr([rng.permutation(21)[:rng.integers(0, 4)] for _ in range(n_users)], n_users)
    masked = O.masked_columns(rated[0], rated[1], n_users, 21)
    s = O.scores(up, uc, ids, w, col_of_item, 21)
    top, top_s = O.topk(s, masked, 25)
    rk = O.ranks(s, masked, *likes)
    for r in range(n_users):
        mine = likes[1][likes[0][r]:likes[0][r + 1]]
        kept, ks, rank = _score_again(uc[up[r]:up[r + 1]], ids, w, col_of_item, 21, masked[r], 25, mine)
        assert top[r, :len(kept)].tolist() == kept and (top[r, len(kept):] == -1).all()
        assert [float(x) for x in top_s[r, :len(kept)]] == [float(x) for x in ks] and np.isneginf(top_s[r, len(kept):]).all()
        assert rk[likes[0][r]:likes[0][r + 1]].tolist() == rank
        for l, q in zip(mine, rank):                              # a like at position p of the list has rank p
            assert q == -1 or q >= 25 or top[r, q] == l


def test_the_chain_is_the_ascending_one():
    """2^24 + 1 + 1 in fp32 is 2^24 in history order (each 1 is lost) and 2^24 + 2 any other way"""
    ids = np.asarray([[3], [3], [3], [-1]], np.int32)
    w = np.asarray([[2.0 ** 24], [1.0], [1.0], [0.0]], np.float32)
    s = O.scores(np.asarray([0, 3], np.int64), np.asarray([0, 1, 2], np.int32), ids, w, None, 4)
    assert s[0, 3] == np.float32(2.0 ** 24) and np.float32(np.float32(1 + 1) + np.float32(2.0 ** 24)) == np.float32(2.0 ** 24 + 2)


def test_library_declares_and_exports_the_knn_entry_points():
    """every name of the binding layer is declared and exported; K28 / K29 change no existing entry point, so TKR_VERSION stays"""
    import tkr_hip
    header = open(os.path.join(ROOT, 'include', 'tkr.h')).read()
    declared = set(re.findall(r'^int(?:32_t|64_t)? (tkr_\w+)\(', header, flags=re.M))
    for name in ('tkr_knn_build', 'tkr_knn_score', 'tkr_knn_build_workspace_bytes'):
        assert name in declared and name in tkr_hip.EXPORTS + tkr_hip.EXPORTS_I64
    for name in ('KNN_MAX_N', 'KNN_MAX_K', 'KNN_MAX_SLAB', 'KNN_HEAVY_FROM', 'KnnRefused', 'knn_build', 'knn_score', 'knn_build_workspace_bytes'):
        assert hasattr(tkr_hip, name), name
    assert issubclass(tkr_hip.KnnRefused, tkr_hip.TkrError)
    for macro in ('MAX_N', 'MAX_K', 'MAX_SLAB', 'HEAVY_FROM'):
        assert re.search(r'#define TKR_KNN_%s %d\b' % (macro, getattr(tkr_hip, 'KNN_' + macro)), header), macro
    assert int(re.search(r'#define TKR_VERSION (\d+)\b', header).group(1)) == tkr_hip.VERSION == 120
    if not os.path.exists(tkr_hip.LIB_PATH):
        return
    lib = ctypes.CDLL(tkr_hip.LIB_PATH)
    for name in ('tkr_knn_build', 'tkr_knn_score', 'tkr_knn_build_workspace_bytes'):
        getattr(lib, name)
    lib.tkr_knn_build_workspace_bytes.restype = ctypes.c_int64
    assert lib.tkr_knn_build_workspace_bytes(ctypes.c_int64(0)) < 0
    need = lib.tkr_knn_build_workspace_bytes(ctypes.c_int64(17770))
    assert 17770 * 8 < need < 64 << 20                            # lists of items and a bounded batch of rows, never n_items^2 counters


def test_status_words_raise_knn_refused():
    import tkr_hip
    for messages, kinds in ((tkr_hip._KNN_BUILD_REFUSED, (0, 1, 2, 3)), (tkr_hip._KNN_SCORE_REFUSED, (0, 1, 2))):
        tkr_hip.status_check('knn', messages, tkr_hip.KnnRefused, -1)
        for kind in kinds:
            with pytest.raises(tkr_hip.KnnRefused) as e:
                tkr_hip.status_check('knn', messages, tkr_hip.KnnRefused, 4 * 7 + kind)
            assert (e.value.row, e.value.kind) == (7, kind)
    with pytest.raises(tkr_hip.TkrError, match='none of the refusals'):
        tkr_hip.status_check('knn', tkr_hip._KNN_SCORE_REFUSED, tkr_hip.KnnRefused, 4 * 7 + 3)


def _model(n_items=6, N=3):
    import knn
    m = knn.ItemKNN(n_neighbors=N, shrink=1.5, similarity='cosine')
    m.n_items = n_items
    m.nbr_ids = np.asarray([[(i + p + 1) % n_items if p < 2 else -1 for p in range(N)] for i in range(n_items)], np.int32)
    m.nbr_w = np.asarray([[1.0 / (p + 1) if p < 2 else 0.0 for p in range(N)] for i in range(n_items)], np.float32)
    m.n_likers = np.arange(n_items, dtype=np.int64)
    return m


def test_knn_npz_round_trip(tmp_path):
    import knn
    m = _model()
    assert not knn.is_model_dir(str(tmp_path))
    m.export_model(str(tmp_path / 'deep' / 'knn'))                 # parents are made
    m.export_model(str(tmp_path))
    assert knn.is_model_dir(str(tmp_path)) and sorted(os.listdir(tmp_path)) == ['deep', 'knn.npz']
    back = knn.load(str(tmp_path))
    for name in ('nbr_ids', 'nbr_w', 'n_likers'):
        a, b = getattr(m, name), getattr(back, name)
        assert a.dtype == b.dtype and a.tobytes() == b.tobytes(), name
    assert (back.n_neighbors, back.shrink, back.similarity, back.n_items) == (3, 1.5, 'cosine', 6)
    with np.load(str(tmp_path / 'knn.npz')) as z:
        assert sorted(z.files) == ['n_likers', 'n_neighbors', 'nbr_ids', 'nbr_w', 'shrink', 'similarity']


def test_hyper_parameters_are_checked():
    import knn
    for kw in (dict(n_neighbors=0), dict(n_neighbors=513), dict(n_neighbors=2.5), dict(shrink=-1.0), dict(shrink=math.inf), dict(shrink=math.nan),
               dict(similarity='jaccard')):
        with pytest.raises(ValueError):
            knn.ItemKNN(**kw)
    with pytest.raises(ValueError, match='load_training_data'):
        knn.ItemKNN().train()
    np.testing.assert_array_equal(knn.norms([0, 1, 4, 9], 'cosine'), [1.0, 1.0, 2.0, 3.0])
    np.testing.assert_array_equal(knn.norms([0, 1, 4, 9], 'cooc'), [1.0, 1.0, 1.0, 1.0])
    np.testing.assert_array_equal(knn.norms([0, 2, 3], 'cosine'), O.norms([0, 2, 3], 'cosine'))


@pytest.mark.parametrize('what,change', [
    ('int32', lambda z: z.update(nbr_ids=z['nbr_ids'].astype(np.int64))),
    ('float32', lambda z: z.update(nbr_w=z['nbr_w'].astype(np.float64))),
    ('int64', lambda z: z.update(n_likers=z['n_likers'].astype(np.int32))),
    ('shapes', lambda z: z.update(nbr_w=z['nbr_w'][:, :2])),
    ('shapes', lambda z: z.update(n_likers=z['n_likers'][:5])),
    ('shapes', lambda z: z.update(nbr_ids=z['nbr_ids'].reshape(-1), nbr_w=z['nbr_w'].reshape(-1))),
    ('outside', lambda z: z['nbr_ids'].__setitem__((2, 1), 6)),
    ('outside', lambda z: z['nbr_ids'].__setitem__((2, 1), -2)),
    ('not finite', lambda z: z['nbr_w'].__setitem__((0, 0), np.inf)),
    ('not finite', lambda z: z['nbr_w'].__setitem__((5, 2), np.nan)),
    ('negative count', lambda z: z['n_likers'].__setitem__(3, -1)),
    ('n_neighbors', lambda z: z.update(n_neighbors=np.int64(4))),
    ('similarity', lambda z: z.update(similarity=np.str_('dot'))),
    ('shrink', lambda z: z.update(shrink=np.float64(-0.5))),
    ('lacks', lambda z: z.pop('n_likers')),
])
def test_import_model_refuses(tmp_path, what, change):
    import knn
    _model().export_model(str(tmp_path))
    with np.load(str(tmp_path / 'knn.npz')) as z:
        arrays = {name: z[name].copy() for name in z.files}
    change(arrays)
    np.savez(str(tmp_path / 'knn.npz'), **arrays)
    with pytest.raises(ValueError, match=what):
        knn.load(str(tmp_path))


def test_import_model_refuses_another_catalogue(tmp_path):
    import knn
    _model().export_model(str(tmp_path))
    other = knn.ItemKNN()
    other.n_items = 7
    with pytest.raises(ValueError, match='7'):
        other.import_model(str(tmp_path))


def test_flags_a_neighbourhood_model_refuses(tmp_path, capsys):
    """parser errors that name the flag, before anything looks for a GPU; a factor directory is not asked"""
    import evaluate
    import recommend
    _model(30, 5).export_model(str(tmp_path))
    model = str(tmp_path)
    factors = os.path.join(ROOT, 'tests', 'golden', 'g4', 'model')
    ev = ['-d', G2, '-m', model, '-sl', 'im']
    for extra, flag in ((['-M', 'ndcg', '--negatives', '20'], '--negatives'), (['--diversify', '0.5'], '--diversify'),
                        (['-M', 'ild'], '-M ild'), (['-M', 'acc', 'cov', 'gini'], '-M cov gini'), (['-M', 'unexp'], '-M unexp')):
        with pytest.raises(SystemExit):
            evaluate.main(ev + extra)
        err = capsys.readouterr().err
        assert flag in err and 'neighbourhood model' in err, (flag, err)
    with pytest.raises(SystemExit):                               # the neighbourhood model on the other side of --compare
        evaluate.main(['-d', G2, '-m', factors, '-sl', 'im', '-M', 'ndcg', 'ild', '--bootstrap', '10', '--compare', model])
    assert 'neighbourhood model' in capsys.readouterr().err
    os.environ['WORLD_SIZE'] = '2'
    try:
        with pytest.raises(SystemExit):
            evaluate.main(ev)
        assert 'multi-process' in capsys.readouterr().err
    finally:
        del os.environ['WORLD_SIZE']
    rec = ['-d', G2, '-m', model, '-o', str(tmp_path / 'out.txt')]
    new = str(tmp_path / 'new')
    open(new, 'w').write('n1\n')
    for extra, flag in ((['--candidates', os.path.join(G2, 'f0tr.txt')], '--candidates'), (['--new-vid', new, '--new-ratings', new], '--new-vid'),
                        (['--diversify', '0.5'], '--diversify'), (['--explain', '2', '--explain-output', str(tmp_path / 'why.txt')], '--explain')):
        with pytest.raises(SystemExit):
            recommend.main(rec + extra)
        err = capsys.readouterr().err
        assert flag in err and 'neighbourhood model' in err, (flag, err)
    assert not os.path.exists(str(tmp_path / 'out.txt'))


# ---- the wide cases of tests/test_gpu_knn_wide.py: their generators, and the conditions each exists for -----------------------------------
# A case is only worth its GPU time while it still holds what it was built to hold, so every condition is asserted here, without a GPU:
# a later change of generator or seed cannot quietly empty a case.
EDGES = (256, 36864, 65536)                                        # the first column of byte 1 of a column id, of the second natural slab, of byte 2
WIDE_ITEMS = 66000
CHAIN_AT = {5: 0.25, 7: 0.75, 8: 0.6875, 10: 0.9375, 15: 0.625, 16: 1.0625, 17: 0.0625}     # position of the large term -> the terms in front of it
CHAIN_LEN = 40


def _work(up, ip, ir):
    """a row's work as knn_plan_kernel counts it: the list lengths of its likers"""
    n_u = np.diff(up)
    return np.asarray([n_u[ir[ip[i]:ip[i + 1]]].sum() for i in range(len(ip) - 1)])


@functools.lru_cache(maxsize=None)
def wide_build_case():
    """case 1: 700 users x 600 items, lists and liker sets long enough for every loop of knn_count_likers to repeat"""
    up, uc = _zipf(700, 600, 281, mean=80)
    ip, ir = O.transpose(up, uc, 600)
    return dict(up=up, uc=uc, ip=ip, ir=ir, n_items=600, work=_work(up, ip, ir))


@functools.lru_cache(maxsize=None)
def wide_build_oracle(similarity, N):
    c = wide_build_case()
    return O.build(c['up'], c['uc'], 600, O.norms(np.diff(c['ip']), similarity), 0.0, N)


def cut_ties(ids, w, N, tied_with, shift):
    """the rows whose last kept and first dropped candidate have equal similarity and columns that differ in col >> shift; tied_with: the
    table of N + 1 neighbours"""
    full = tied_with[0][:, N] >= 0
    same = _bits32(tied_with[1][:, N - 1]) == _bits32(tied_with[1][:, N])
    apart = (tied_with[0][:, N - 1] >> shift) != (tied_with[0][:, N] >> shift)
    assert (ids == tied_with[0][:, :N]).all() and (_bits32(w) == _bits32(tied_with[1][:, :N])).all()      # a list is a prefix of the longer one
    return np.flatnonzero(full & same & apart)


def _bits32(a):
    return np.ascontiguousarray(a).view(np.int32)


@functools.lru_cache(maxsize=None)
def band_case():
    """case 2: 400 users x 66,000 items; the liked items lie in three bands, one at the bottom, one astride the edge of the natural slab
    and one astride 65,536, with a Zipf-like popularity inside each band"""
    rng = np.random.Generator(np.random.PCG64(66))
    bands = [np.arange(0, 300), np.arange(36700, 37000), np.arange(65400, 66000)]
    cols = np.concatenate(bands)
    pop = np.concatenate([rng.permutation(np.arange(1, len(b) + 1, dtype=np.float64) ** -0.9) / len(bands) for b in bands])
    pop /= pop.sum()
    rows = [cols[rng.choice(len(cols), size=int(rng.integers(10, 61)), replace=False, p=pop)] for _ in range(400)]
    up, uc = O.csr(rows, 400)
    ip, ir = O.transpose(up, uc, WIDE_ITEMS)
    return dict(up=up, uc=uc, ip=ip, ir=ir, n_items=WIDE_ITEMS, work=_work(up, ip, ir), heavy_from=600)


@functools.lru_cache(maxsize=None)
def band_oracle(similarity, N=100):
    c = band_case()
    return O.build_compact(c['up'], c['uc'], WIDE_ITEMS, O.norms(np.diff(c['ip']), similarity), 0.0, N)


def _csr_as_given(rows):
    """(ptr int64, cols int32) of rows kept as they are: repeats and any order stay (O.csr sorts and drops them)"""
    ptr = np.zeros(len(rows) + 1, np.int64)
    np.cumsum([len(r) for r in rows], out=ptr[1:])
    return ptr, np.asarray([c for r in rows for c in r], np.int64).astype(np.int32)


def _take(ptr, cols, rows):
    return _csr_as_given([cols[ptr[r]:ptr[r + 1]] for r in rows])


@functools.lru_cache(maxsize=None)
def serve_case(columns):
    """case 3: 96 lines of case 1 as histories (the longest, the shortest that is not empty, every empty one, the rest evenly spaced by
    length); columns = 'identity' (600) or 'subset' (400 of the 600 items under a random permutation); a rated mask of 0 to 40 columns per
    line; 0 to 12 likes per line, but `many` has 300 (repeats, masked and out-of-range columns among them) and `chunk` exactly 256"""
    c = wide_build_case()
    rng = np.random.Generator(np.random.PCG64(3 if columns == 'identity' else 4))
    n_u = np.diff(c['up'])
    by_length = np.argsort(n_u, kind='stable')
    must = [int(by_length[-1]), int(by_length[n_u[by_length] > 0][0])] + [int(u) for u in np.flatnonzero(n_u == 0)]
    rest = [int(u) for u in by_length if u not in must]
    users = sorted(must + [rest[int(round(x))] for x in np.linspace(0, len(rest) - 1, 96 - len(must))])
    assert len(set(users)) == 96
    hist = _take(c['up'], c['uc'], users)
    n_cols, col_of_item = 600, None
    if columns == 'subset':
        n_cols, col_of_item = 400, np.full(600, -1, np.int32)
        col_of_item[np.sort(rng.permutation(600)[:400])] = rng.permutation(400)
    rated = O.csr([rng.permutation(n_cols)[:rng.integers(0, 41)] for _ in range(96)], 96)
    masked = O.masked_columns(rated[0], rated[1], 96, n_cols)
    likes = [rng.permutation(n_cols)[:rng.integers(0, 13)].tolist() for _ in range(96)]
    many = users.index(must[0])                                    # the longest history ranks 300 likes
    chunk = int(np.flatnonzero(masked.sum(1) >= 5)[5])
    chunk += chunk == many
    some_masked = np.flatnonzero(masked[many])[:5].tolist()
    outside = [n_cols, n_cols + 1000, -1, 2 ** 31 - 1]
    likes[many] = rng.permutation(some_masked + outside + rng.integers(0, n_cols, 300 - len(some_masked) - len(outside)).tolist()).tolist()
    likes[chunk] = rng.permutation(n_cols)[:256].tolist()
    return dict(users=users, hist=hist, n_cols=n_cols, col_of_item=col_of_item, rated=rated, masked=masked, likes=_csr_as_given(likes),
                many=many, chunk=chunk, some_masked=some_masked)


@functools.lru_cache(maxsize=None)
def serve_oracle(columns, N):
    """-> (nbr_ids, nbr_w, scores, ranks) of case 3 at N neighbours"""
    c = serve_case(columns)
    ids, w = wide_build_oracle('cosine', N)[:2]
    s = O.scores_by_item(*c['hist'], ids, w, c['col_of_item'], c['n_cols'])
    return ids, w, s, O.ranks(s, c['masked'], *c['likes'])


def _tie_row(place, negative, rng):
    """a neighbour list of 512 with three weights: 16 columns of 3.0 astride the next edge, 32 of 2.0 astride EDGES[place], so that a list
    of 32 is cut between EDGES[place] and the column below it, and the rest 1.0 astride the third edge.  negative: a 17th column of 3.0 (the
    caller masks it), the low group below its edge is -1.0 and its highest column is -0.0"""
    e, e_high, e_low = EDGES[place], EDGES[(place + 1) % 3], EDGES[(place + 2) % 3]
    high = np.arange(e_high - 8, e_high + 8 + negative)
    mid = np.arange(e - 16, e + 16)
    low = np.arange(e_low - 232, e_low + 232 - negative)
    cols = np.concatenate([high, mid, low])
    w = np.concatenate([np.full(len(high), 3.0), np.full(len(mid), 2.0), np.full(len(low), 1.0)]).astype(np.float32)
    if negative:
        w[len(high) + len(mid):][low < e_low] = -1.0
        w[-1] = -0.0
    assert len(cols) == len(set(cols.tolist())) == 512
    order = rng.permutation(512)                                   # K29 takes any table: the list is in no order
    return cols[order].astype(np.int32), w[order]


LIKED_EDGES = [0, 255, 256, 36863, 36864, 65535, 65536, 65999]


@functools.lru_cache(maxsize=None)
def hand_case():
    """case 4 at N = 512 over 66,000 identity columns: a table that is -1 / 0 but for six rows, and eight lines
       0      an empty history, nothing masked: every column scores +0.0
       1      an empty history, [30,000, 66,000) masked but for 65,536 and 36,864
       2-4    one history item whose list is _tie_row(place): the cut of a list of 32 falls inside a tie group at each edge in turn
       5-7    the same with negative weights, a -0.0 and one masked column
    every line likes the columns of LIKED_EDGES (lines 5-7 also a negative column, the -0.0 one and the masked one)"""
    rng = np.random.Generator(np.random.PCG64(512))
    ids = np.full((WIDE_ITEMS, 512), -1, np.int32)
    w = np.zeros((WIDE_ITEMS, 512), np.float32)
    hist, rated, likes = [[], []], [[], [c for c in range(30000, WIDE_ITEMS) if c not in (65536, 36864)]], [LIKED_EDGES, LIKED_EDGES]
    for negative in (0, 1):
        for place in range(3):
            item = 1000 * (1 + negative) + 7 * place
            ids[item], w[item] = _tie_row(place, negative, rng)
            hist.append([item])
            hidden = EDGES[(place + 1) % 3] + 8                    # the 17th column of 3.0
            low_edge = EDGES[(place + 2) % 3]
            rated.append([hidden] if negative else [])
            likes.append(LIKED_EDGES + ([low_edge - 1, low_edge - 232, low_edge + 230, hidden] if negative else []))
    return dict(ids=ids, w=w, hist=O.csr(hist, 8), rated=O.csr(rated, 8), likes=_csr_as_given(likes), n_lines=8)


def chain_weights(q, at):
    """CHAIN_LEN weights whose fp32 sum in this order is one value with the large term at position `at` = q and another at q - 1 or q + 1:
    CHAIN_AT[q] in front of position q, then 1.0, then 2.0, and 2^24 put in at `at`"""
    small = [CHAIN_AT[q]] * q + [1.0] + [2.0] * (CHAIN_LEN - q - 2)
    return np.asarray(small[:at] + [2.0 ** 24] + small[at:], np.float32)


def chain_columns(k):
    """the two columns line k of the chain case sums into: through the first piece of every list, and through the last"""
    return 36860 + 2 * k, 65530 + 2 * k


@functools.lru_cache(maxsize=None)
def chain_case(N):
    """case 4, the chains: line k has a history of CHAIN_LEN items of its own; the list of its t-th item holds chain_columns(k)[0] in the
    first piece of 64 (slot (5 t + 3) % 64) and chain_columns(k)[1] in the last slot of the list, both with chain_weights(q, q)[t], and
    a filler column of weight 0.5 in every other slot, so that every piece of every list adds something"""
    ids = np.full((WIDE_ITEMS, N), -1, np.int32)
    w = np.zeros((WIDE_ITEMS, N), np.float32)
    hist = []
    for k, q in enumerate(sorted(CHAIN_AT)):
        items = 3000 + 100 * k + np.arange(CHAIN_LEN)
        weights = chain_weights(q, q)
        for t, item in enumerate(items):
            ids[item] = 10000 + np.arange(N)
            w[item] = 0.5
            first = (5 * t + 3) % 64
            ids[item, first], ids[item, N - 1] = chain_columns(k)
            w[item, first] = w[item, N - 1] = weights[t]
        hist.append(items)
    n = len(CHAIN_AT)
    likes = [list(chain_columns(k)) + [10000, 10000 + N // 2, 65999] for k in range(n)]
    return dict(ids=ids, w=w, hist=O.csr(hist, n), rated=O.csr([[]] * n, n), likes=_csr_as_given(likes), n_lines=n)


@functools.lru_cache(maxsize=None)
def hand_oracle(which, N=512):
    """-> (scores, masked, ranks, top ids at K = 70, their scores) of hand_case() or chain_case(N); a list of K < 70 is a prefix"""
    c = hand_case() if which == 'hand' else chain_case(N)
    s = O.scores(*c['hist'], c['ids'], c['w'], None, WIDE_ITEMS)
    masked = O.masked_columns(c['rated'][0], c['rated'][1], c['n_lines'], WIDE_ITEMS)
    return (s, masked, O.ranks(s, masked, *c['likes'])) + O.topk(s, masked, 70)


def test_wide_build_case_repeats_every_loop_of_the_count():
    c = wide_build_case()
    n_u, n_i = np.diff(c['up']), np.diff(c['ip'])
    assert len(c['uc']) == 53984
    assert (n_u > 64).sum() == 398 and (n_u > 128).sum() == 122 and n_u.max() == 159       # the x += 64 loop runs twice and three times
    assert (n_i > 256).sum() == 37 and (n_i > 512).sum() == 8 and n_i.max() == 658         # the b0 += 256 loop likewise
    assert n_i.min() > 0 and c['work'].max() == 53674
    assert (c['work'] > 700).mean() > 0.5 and (np.minimum(n_i, -(-c['work'] // 700)) >= 64).any()      # heavy_from = 700: most rows split, some to the cap
    C = wide_build_oracle('cooc', 16)[2]
    assert ((C > 0).sum(1) - 1).min() > 512                        # the radix select runs on every row at every N


@pytest.mark.parametrize('similarity,N,rows', [('cooc', 100, 3), ('cooc', 512, 18), ('cosine', 100, 11), ('cosine', 512, 91)])
def test_wide_build_case_has_ties_that_column_byte_1_decides(similarity, N, rows):
    c = wide_build_case()
    norm = O.norms(np.diff(c['ip']), similarity)
    ids, w = wide_build_oracle(similarity, N)[:2]
    tied = cut_ties(ids, w, N, O.build(c['up'], c['uc'], 600, norm, 0.0, N + 1)[:2], 8)
    assert len(tied) == rows


def test_build_compact_is_build():
    """the 700 x 600 case widened to 1,000 columns with empty items between the liked ones, and a hand-made case"""
    c = wide_build_case()
    rng = np.random.Generator(np.random.PCG64(1000))
    where = np.sort(rng.permutation(1000)[:600]).astype(np.int32)
    wide_cols = where[c['uc']]
    for similarity, shrink, N in (('cosine', 0.0, 100), ('cooc', 1.5, 512)):
        norm = O.norms(np.bincount(wide_cols, minlength=1000), similarity)
        want = O.build(c['up'], wide_cols, 1000, norm, shrink, N)[:2]
        got = O.build_compact(c['up'], wide_cols, 1000, norm, shrink, N)
        assert (got[0] == want[0]).all() and (_bits32(got[1]) == _bits32(want[1])).all()
        unliked = np.setdiff1d(np.arange(1000), where)
        assert len(unliked) == 400 and (got[0][unliked] == -1).all() and (_bits32(got[1][unliked]) == 0).all()
    up, uc = O.csr([[2, 9, 11], [2, 9], [9, 11, 14], [], [2, 14], [0]], 6)
    norm = np.asarray([1.0 + 0.25 * i for i in range(16)])
    want = O.build(up, uc, 16, norm, 0.5, 3)[:2]
    got = O.build_compact(up, uc, 16, norm, 0.5, 3)
    assert (got[0] == want[0]).all() and (_bits32(got[1]) == _bits32(want[1])).all()
    assert got[0][9].tolist() == [2, 11, 14] and got[0][0].tolist() == [-1] * 3 and got[0][15].tolist() == [-1] * 3


def test_band_case_spans_both_slabs_and_byte_2():
    c = band_case()
    n_u, n_i = np.diff(c['up']), np.diff(c['ip'])
    liked = np.flatnonzero(n_i)
    assert n_u.min() >= 10 and n_u.max() <= 60 and len(liked) > 1000
    assert set(np.unique(liked // 300 * 300).tolist()) <= {0, 36600, 36900, 65400, 65700}
    assert (c['work'] > c['heavy_from']).sum() >= 50               # rows that take the partial / finish path
    for similarity in ('cooc', 'cosine'):
        ids, w = band_oracle(similarity)
        kept = ids >= 0
        assert ((kept & (ids < 36864)).any(1) & (ids >= 36864).any(1)).any()           # a kept list with columns from both natural slabs
        assert (ids[:, -1] == -1).mean() > 0.5                     # most rows are padded
        assert (ids[n_i == 0] == -1).all() and (_bits32(w[n_i == 0]) == 0).all()
        assert (ids[liked, -1] == -1).any() and (ids[liked, -1] >= 0).sum() >= 50       # of the liked rows some are padded and some are cut
        tied = cut_ties(ids, w, 100, band_oracle(similarity, 101), 16)
        assert len(tied) >= 1                                      # a tie at the cut that only column byte 2 decides


def test_serve_case_holds_the_lines_it_names():
    b = wide_build_case()
    for columns in ('identity', 'subset'):
        c = serve_case(columns)
        n_h, n_l = np.diff(c['hist'][0]), np.diff(c['likes'][0])
        assert len(n_h) == 96 and n_h.max() == 159 and (n_h == 0).sum() == (np.diff(b['up']) == 0).sum() == 2 and n_h[n_h > 0].min() == 1
        assert len(set(n_h.tolist())) > 60                         # evenly spaced by length
        assert n_l[c['many']] == 300 and n_l[c['chunk']] == 256 and np.delete(n_l, [c['many'], c['chunk']]).max() <= 12 and (n_l == 0).any()
        mine = c['likes'][1][c['likes'][0][c['many']]:c['likes'][0][c['many'] + 1]]
        assert len(set(mine.tolist())) < 300 and set(c['some_masked']) <= set(mine.tolist()) and (mine >= c['n_cols']).sum() == 3 and (mine < 0).sum() == 1
        assert np.diff(c['rated'][0]).max() <= 40 and (np.diff(c['rated'][0]) == 0).any()
        ranks = serve_oracle(columns, 100)[3]
        assert (ranks[c['likes'][0][c['many']]:c['likes'][0][c['many'] + 1]] == -1).sum() >= 9 and ranks.max() > 300


def test_scores_by_item_is_the_loop():
    """the vectorised oracle against the scalar one: on g2, and on 40 lines of case 3"""
    up, uc, ip, _, _, n_items = g2_likes()
    ids, w = O.build(up, uc, n_items, O.norms(np.diff(ip), 'cosine'), 0.0, 5)[:2]
    col_of_item = np.full(n_items, -1, np.int32)
    col_of_item[::2] = np.arange(15)[::-1]
    for cols, n_cols in ((None, n_items), (col_of_item, 15)):
        assert O.scores_by_item(up, uc, ids, w, cols, n_cols).tobytes() == O.scores(up, uc, ids, w, cols, n_cols).tobytes()
    c = serve_case('subset')
    ids, w, s, _ = serve_oracle('subset', 130)
    hist = _take(c['hist'][0], c['hist'][1], range(50, 90))
    assert s[50:90].tobytes() == O.scores(*hist, ids, w, c['col_of_item'], 400).tobytes()


def test_hand_case_is_decided_by_construction():
    c = hand_case()
    s, masked, ranks, top, top_s = hand_oracle('hand')
    assert top[0].tolist() == list(range(65999, 65929, -1)) and (_bits32(top_s[0]) == 0).all()         # all of column bytes 2, 1 and 0
    assert top[1, :5].tolist() == [65536, 36864, 29999, 29998, 29997]
    lp = c['likes'][0]
    assert ranks[lp[0]:lp[1]].tolist() == [65999 - col for col in LIKED_EDGES]
    assert ranks[lp[1]:lp[2]].tolist() == [30001, 29746, 29745, -1, 1, -1, 0, -1]
    for line in range(2, 8):
        place, negative = (line - 2) % 3, line >= 5
        e, e_high = EDGES[place], EDGES[(place + 1) % 3]
        want = list(range(e_high + 7, e_high - 9, -1)) + list(range(e + 15, e - 1, -1))
        assert top[line, :32].tolist() == want and top[line, 32] == e - 1 and s[line, e] == s[line, e - 1] == 2      # the cut is inside the tie
        assert (s[line] != 0).sum() == 512 - negative and masked[line].sum() == negative
        if negative:
            mine = ranks[lp[line]:lp[line + 1]][-4:]
            assert (s[line] < 0).sum() == 232 and mine[3] == -1 and mine[0] > 65000 and mine[1] == WIDE_ITEMS - 2      # behind every +0.0; one column is masked
            assert _bits32(s[line, EDGES[(place + 2) % 3] + 230]) == 0 and 200 < mine[2] < WIDE_ITEMS - 232         # -0.0 is +0.0: among the untouched columns


def _chain(weights, order):
    acc = np.float32(0)
    for t in order:
        acc = np.float32(acc + weights[t])
    return acc


@pytest.mark.parametrize('N', [100, 130])
def test_chain_case_depends_on_the_position_of_the_large_term(N):
    """moving 2^24 by one position changes the sum, and so does adding each batch of sixteen list pieces backwards"""
    c = chain_case(N)
    s = hand_oracle('chain', N)[0]
    nch = -(-N // 64)
    for k, q in enumerate(sorted(CHAIN_AT)):
        base = _chain(chain_weights(q, q), range(CHAIN_LEN))
        assert len({float(base), float(_chain(chain_weights(q, q - 1), range(CHAIN_LEN))), float(_chain(chain_weights(q, q + 1), range(CHAIN_LEN)))}) == 3
        for col, piece in zip(chain_columns(k), (0, nch - 1)):
            assert _bits32(s[k, col]) == _bits32(base)
            steps = [t * nch + piece for t in range(CHAIN_LEN)]    # the pieces that add to this column, in order
            backwards = sorted(steps, key=lambda x: (x // 16, -(x % 16)))
            assert _chain(chain_weights(q, q), [x // nch for x in backwards]) != base
        assert (s[k, 10000:10000 + N] != 0).sum() == N - 1 and s[k].max() == base       # every filler but the last slot's, which no list holds
    straddles = [t for t in range(CHAIN_LEN) if (t * nch) // 16 != (t * nch + nch - 1) // 16]
    assert (straddles == []) if N == 100 else (5 in straddles and 10 in straddles)     # N = 130: the pieces of items 5 and 10 lie in two batches
