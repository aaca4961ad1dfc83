"""K28 / K29 without a GPU: the oracle of tests/test_gpu_knn.py (tests/_knn_oracle.py) against a second, dense restatement written
another way, the symbols of include/tkr.h, what knn.ItemKNN stores and refuses, and the flags evaluate.py and recommend.py refuse for a
neighbourhood model before they look for a GPU."""
import ctypes
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
