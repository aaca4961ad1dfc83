"""K28 / K29 on the GPU (csrc/knn.hip, top-k-rec_amd/knn.py) against tests/_knn_oracle.py.

Every comparison is bit for bit: the counts are integers, the similarity is three fp64 operations and one rounding that NumPy restates,
the score is one fp32 chain in history order, and the order is the canonical one.  Nothing here has a tolerance."""
import functools
import os

import numpy as np
import pytest
import torch

import _knn_oracle as O
from test_knn_cpu import G2, _zipf, g2_likes

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G4 = os.path.join(ROOT, 'tests', 'golden', 'g4')
NO_HEAVY = 1 << 40


def _dev(a):
    return torch.from_numpy(np.array(a, order='C')).cuda()


def _bits(a):
    return np.ascontiguousarray(a).view(np.int32)


def _build(up, uc, n_items, norm, N, shrink=0.0, **kw):
    import tkr_hip
    ip, ir = O.transpose(up, uc, n_items)
    ids, w = tkr_hip.knn_build(_dev(up), _dev(uc), _dev(ip), _dev(ir), _dev(np.asarray(norm, np.float64)), N, shrink=shrink, **kw)
    return ids.cpu().numpy(), w.cpu().numpy()


def _same_table(got, want, what=''):
    np.testing.assert_array_equal(got[0], want[0], err_msg='ids ' + what)
    np.testing.assert_array_equal(_bits(got[1]), _bits(want[1]), err_msg='weights ' + what)


def _cosine(up, uc, n_items):
    return O.norms(np.bincount(uc, minlength=n_items), 'cosine')


@functools.lru_cache(maxsize=None)
def _zipf_case():
    up, uc = _zipf(300, 200, 28)
    norm = _cosine(up, uc, 200)
    return up, uc, norm, O.build(up, uc, 200, norm, 0.0, 16)[:2]


# ---- K28 ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('N', [5, 40])
def test_build_g2(N):
    """40 users, 30 items, 3 users without likes, 4 items without likers, 51 tied similarities; at N = 40 every row is padded"""
    up, uc, _, _, _, n_items = g2_likes()
    norm = _cosine(up, uc, n_items)
    want = O.build(up, uc, n_items, norm, 0.0, N)[:2]
    got = _build(up, uc, n_items, norm, N)
    _same_table(got, want)
    if N == 40:
        assert (got[0][:, -1] == -1).all() and (_bits(got[1][:, -1]) == 0).all()
    again = _build(up, uc, n_items, norm, N)                       # two runs give equal bits
    _same_table(again, got, 'of the second run')


def test_build_split_rows_and_slabs_change_nothing():
    """Zipf-shaped 300 x 200, N = 16: heavy_from = 50 splits most rows over several workgroups (and the 200 items over four batches of
    workspace rows), slab_cols = 64 walks every row four times; both give the bits of the plain call and of the oracle"""
    up, uc, norm, want = _zipf_case()
    n_u = np.diff(up)
    ip, ir = O.transpose(up, uc, 200)
    work = np.asarray([n_u[ir[ip[i]:ip[i + 1]]].sum() for i in range(200)])            # a row's work: the list lengths of its likers
    assert (work > 50).mean() > 0.5
    _same_table(_build(up, uc, 200, norm, 16, heavy_from=NO_HEAVY), want, 'unsplit')
    _same_table(_build(up, uc, 200, norm, 16, heavy_from=50), want, 'split')
    _same_table(_build(up, uc, 200, norm, 16, heavy_from=NO_HEAVY, slab_cols=64), want, 'in slabs')
    _same_table(_build(up, uc, 200, norm, 16, heavy_from=7, slab_cols=33), want, 'split and in slabs')


@pytest.mark.parametrize('n_items', [1, 65, 129])
def test_build_small_catalogues(n_items):
    up, uc = _zipf(50, n_items, n_items, mean=min(n_items, 8))
    norm = _cosine(up, uc, n_items)
    for N in (1, 64, 65):
        want = O.build(up, uc, n_items, norm, 0.0, N)[:2]
        _same_table(_build(up, uc, n_items, norm, N), want, 'N = %d' % N)
        _same_table(_build(up, uc, n_items, norm, N, heavy_from=3, slab_cols=64), want, 'N = %d, split, in slabs' % N)


def test_build_identical_liker_sets_tie_to_the_higher_column():
    rows = [[0, 1, 2, 3, 4, 5], [0, 1, 2, 3, 4, 5], [0, 1, 2, 3, 4, 5, 6], [6, 7], []]
    up, uc = O.csr(rows, 5)
    norm = _cosine(up, uc, 9)
    want = O.build(up, uc, 9, norm, 0.0, 4)[:2]
    assert want[0][0].tolist() == [5, 4, 3, 2] and want[0][5].tolist() == [4, 3, 2, 1] and want[0][8].tolist() == [-1] * 4
    _same_table(_build(up, uc, 9, norm, 4), want)
    _same_table(_build(up, uc, 9, norm, 4, heavy_from=1, slab_cols=2), want, 'split, in slabs')


@pytest.mark.parametrize('similarity,shrink', [('cooc', 0.0), ('cosine', 2.5), ('cosine', 1e-3)])
def test_build_cooc_and_shrink(similarity, shrink):
    up, uc, _, _ = _zipf_case()
    norm = O.norms(np.bincount(uc, minlength=200), similarity)
    want = O.build(up, uc, 200, norm, shrink, 16)
    got = _build(up, uc, 200, norm, 16, shrink=shrink)
    _same_table(got, want[:2])
    if similarity == 'cooc':                                       # the raw count
        C = want[2]
        assert all(got[1][i, p] == C[i, got[0][i, p]] for i in range(200) for p in range(16) if got[0][i, p] >= 0)


def _refused(kind, change):
    import tkr_hip
    up, uc = _zipf(20, 12, 5, mean=4)
    ip, ir = O.transpose(up, uc, 12)
    arrays = dict(up=up.copy(), uc=uc.copy(), ip=ip.copy(), ir=ir.copy(), norm=_cosine(up, uc, 12))
    change(arrays)
    ids = torch.full((12, 3), 77, dtype=torch.int32, device='cuda')
    w = torch.full((12, 3), 7.5, dtype=torch.float32, device='cuda')
    with pytest.raises(tkr_hip.KnnRefused) as e:
        tkr_hip.knn_build(_dev(arrays['up']), _dev(arrays['uc']), _dev(arrays['ip']), _dev(arrays['ir']), _dev(arrays['norm']), 3, out=(ids, w))
    assert e.value.kind == kind
    assert (ids.cpu().numpy() == 77).all() and (w.cpu().numpy() == 7.5).all()      # a refused call leaves both outputs untouched
    return e.value


@pytest.mark.parametrize('kind,change', [
    (0, lambda a: a['up'].__setitem__(0, 1)),                                       # does not start at 0
    (0, lambda a: a['up'].__setitem__(5, a['up'][4] - 1)),                          # decreases
    (0, lambda a: a['ip'].__setitem__(12, len(a['ir']) + 1)),                       # leaves its array
    (0, lambda a: a['ip'].__setitem__(3, -2)),
    (1, lambda a: a['uc'].__setitem__(2, 12)),                                      # a column outside [0, n_items)
    (1, lambda a: a['uc'].__setitem__(0, -1)),
    (1, lambda a: a['ir'].__setitem__(1, 20)),                                      # a row outside [0, n_users)
    (2, lambda a: a['up'].__setitem__(20, a['up'][20] - 1)),                        # the CSRs hold different numbers of entries
    (3, lambda a: a['norm'].__setitem__(4, 0.0)),
    (3, lambda a: a['norm'].__setitem__(4, -1.0)),
    (3, lambda a: a['norm'].__setitem__(11, np.inf)),
    (3, lambda a: a['norm'].__setitem__(0, np.nan)),
])
def test_build_refusals_leave_the_outputs_untouched(kind, change):
    _refused(kind, change)


def test_build_refusal_names_the_place():
    assert _refused(3, lambda a: a['norm'].__setitem__(4, 0.0)).row == 4
    assert _refused(1, lambda a: a['uc'].__setitem__(2, 12)).row == 2
    assert _refused(0, lambda a: a['ip'].__setitem__(3, -2)).row == 20 + 1 + 2      # row 2 of i_ptr is the first that sees it: it decreases


# ---- K29 ----------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _score_case():
    """g2's likes as histories, its table at N = 5, a subset of 21 of the 30 items as permuted columns, a mask and likes per line"""
    up, uc, ip, _, n_users, n_items = g2_likes()
    ids, w = O.build(up, uc, n_items, O.norms(np.diff(ip), 'cosine'), 0.0, 5)[:2]
    rng = np.random.Generator(np.random.PCG64(29))
    col_of_item = np.full(n_items, -1, np.int32)
    col_of_item[np.sort(rng.permutation(n_items)[:21])] = rng.permutation(21)
    rated = O.csr([rng.permutation(21)[:rng.integers(0, 6)] for _ in range(n_users)], n_users)
    likes = O.csr([rng.permutation(21)[:rng.integers(0, 4)] for _ in range(n_users)], n_users)
    masked = O.masked_columns(rated[0], rated[1], n_users, 21)
    s = O.scores(up, uc, ids, w, col_of_item, 21)
    return dict(up=up, uc=uc, ids=ids, w=w, col_of_item=col_of_item, rated=rated, likes=likes, masked=masked, s=s,
                ranks=O.ranks(s, masked, *likes), n_users=n_users)


def _score(c, K, lines=None, **kw):
    """K29 on the lines [lo, hi) of the case -> (ids, scores, ranks) as numpy"""
    import tkr_hip
    lo, hi = lines or (0, c['n_users'])
    cut = lambda ptr, cols: (_dev(ptr[lo:hi + 1] - ptr[lo]), _dev(cols[ptr[lo]:ptr[hi]]))
    mask, pitch = tkr_hip.build_rated_mask(*cut(*c['rated']), hi - lo, 21)
    lp, lc = cut(*c['likes'])
    out = tkr_hip.knn_score(*cut(c['up'], c['uc']), _dev(c['ids']), _dev(c['w']), K, col_of_item=_dev(c['col_of_item']), n_cols=21, mask=mask,
                            mask_pitch=pitch, want_scores=True, like_ptr=lp, like_cols=lc, **kw)
    return tuple(x.cpu().numpy() for x in out)


@pytest.mark.parametrize('K', [5, 25, 40])
def test_score_g2_lists_scores_and_ranks(K):
    """K = 5; K = 25 above the kept columns of every line (at most 21); K = 40 above what one launch lists"""
    c = _score_case()
    want_ids, want_s = O.topk(c['s'], c['masked'], K)
    ids, scores, ranks = _score(c, K)
    np.testing.assert_array_equal(ids, want_ids)
    np.testing.assert_array_equal(_bits(scores), _bits(want_s))
    np.testing.assert_array_equal(ranks, c['ranks'])
    if K > 21:
        assert (ids[:, 21:] == -1).all() and np.isneginf(scores[:, 21:]).all()
    lp, lc = c['likes']
    seen = 0
    for r in range(c['n_users']):                                  # a like at position p of the list has rank p
        for e in range(lp[r], lp[r + 1]):
            if 0 <= ranks[e] < K:
                assert ids[r, ranks[e]] == lc[e]
                seen += 1
    assert seen > 10 and (ranks == -1).any()
    empty = np.flatnonzero(np.diff(c['up']) == 0)                  # an empty history: the unmasked columns, descending, all +0.0
    assert len(empty) == 3
    for r in empty:
        kept = [col for col in range(20, -1, -1) if not c['masked'][r, col]][:K]
        assert ids[r, :len(kept)].tolist() == kept and (_bits(scores[r, :len(kept)]) == 0).all()
    again = _score(c, K)                                           # two runs give the same bits
    for a, b in zip(again, (ids, scores, ranks)):
        assert a.tobytes() == b.tobytes()


@pytest.mark.parametrize('slab_cols', [1, 8, 20])
def test_score_in_slabs_changes_nothing(slab_cols):
    c = _score_case()
    want_ids, want_s = O.topk(c['s'], c['masked'], 25)
    ids, scores, ranks = _score(c, 25, slab_cols=slab_cols)
    np.testing.assert_array_equal(ids, want_ids)
    np.testing.assert_array_equal(_bits(scores), _bits(want_s))
    np.testing.assert_array_equal(ranks, c['ranks'])


def test_score_a_block_of_lines_alone_is_the_block_inside_the_call():
    c = _score_case()
    whole = _score(c, 7)
    block = _score(c, 7, lines=(9, 23))
    lp = c['likes'][0]
    assert block[0].tobytes() == whole[0][9:23].tobytes() and block[1].tobytes() == whole[1][9:23].tobytes()
    assert block[2].tobytes() == whole[2][lp[9]:lp[23]].tobytes()


def test_score_identity_columns_no_mask_ranks_alone():
    """col_of_item = None, no mask; K = 0 gives the ranks alone"""
    import tkr_hip
    c = _score_case()
    s = O.scores(c['up'], c['uc'], c['ids'], c['w'], None, 30)
    nothing = np.zeros((c['n_users'], 30), bool)
    likes = O.csr([[r % 30, (7 * r + 3) % 30, 31] for r in range(c['n_users'])], c['n_users'])      # 31: out of range -> -1
    likes = (likes[0], likes[1])
    args = (_dev(c['up']), _dev(c['uc']), _dev(c['ids']), _dev(c['w']))
    ids, ranks = tkr_hip.knn_score(*args, 30, like_ptr=_dev(likes[0]), like_cols=_dev(likes[1]))
    np.testing.assert_array_equal(ids.cpu().numpy(), O.topk(s, nothing, 30)[0])
    want = O.ranks(s, nothing, *likes)
    np.testing.assert_array_equal(ranks.cpu().numpy(), want)
    assert (want == -1).sum() == c['n_users']
    alone = tkr_hip.knn_score(*args, 0, like_ptr=_dev(likes[0]), like_cols=_dev(likes[1]))
    np.testing.assert_array_equal(alone.cpu().numpy(), want)


def test_score_hand_made_table():
    """weights 2^24, 1 and 1 on one column: the ascending chain gives 2^24, any other order 2^24 + 2; item 3's row is all -1"""
    import tkr_hip
    ids = np.asarray([[4, -1], [4, 0], [4, -1], [-1, -1], [1, 2]], np.int32)
    w = np.asarray([[2.0 ** 24, 0], [1, 0.5], [1, 0], [0, 0], [0.25, 0.125]], np.float32)
    hist = O.csr([[0, 1, 2], [1, 2, 0], [3], [2, 3], [3, 4]], 5)
    s = O.scores(*hist, ids, w, None, 5)
    assert s[0, 4] == np.float32(2.0 ** 24) and s[1, 4] == np.float32(2.0 ** 24) and s[3, 4] == 1 and (s[2] == 0).all()
    nothing = np.zeros((5, 5), bool)
    got_ids, got_s = tkr_hip.knn_score(_dev(hist[0]), _dev(hist[1]), _dev(ids), _dev(w), 5, want_scores=True)
    want_ids, want_s = O.topk(s, nothing, 5)
    np.testing.assert_array_equal(got_ids.cpu().numpy(), want_ids)
    np.testing.assert_array_equal(_bits(got_s.cpu().numpy()), _bits(want_s))
    assert got_ids.cpu().numpy()[2].tolist() == [4, 3, 2, 1, 0]    # the history is item 3 alone: nobody contributes


@pytest.mark.parametrize('kind,change', [
    (0, lambda a: a['hp'].__setitem__(0, 2)),
    (0, lambda a: a['hp'].__setitem__(7, a['hp'][6] - 1)),
    (0, lambda a: a['hp'].__setitem__(40, len(a['hc']) + 1)),
    (1, lambda a: a['hc'].__setitem__(3, 30)),
    (1, lambda a: a['hc'].__setitem__(0, -1)),
    (2, lambda a: a['lp'].__setitem__(40, len(a['lc']) + 5)),
    (2, lambda a: a['lp'].__setitem__(2, -1)),
])
def test_score_refusals(kind, change):
    import tkr_hip
    c = _score_case()
    a = dict(hp=c['up'].copy(), hc=c['uc'].copy(), lp=c['likes'][0].copy(), lc=c['likes'][1].copy())
    change(a)
    with pytest.raises(tkr_hip.KnnRefused) as e:
        tkr_hip.knn_score(_dev(a['hp']), _dev(a['hc']), _dev(c['ids']), _dev(c['w']), 5, col_of_item=_dev(c['col_of_item']), n_cols=21,
                          like_ptr=_dev(a['lp']), like_cols=_dev(a['lc']))
    assert e.value.kind == kind


# ---- end to end ---------------------------------------------------------------------------------------------------------------------------
def _trained(data, N, tmp):
    import knn
    model = knn.ItemKNN(n_neighbors=N)
    model.load_training_data(os.path.join(data, 'uid'), os.path.join(data, 'vid'), os.path.join(data, 'f0tr.txt'))
    model.train(model_path=tmp)
    return model


def _oracle_scenario(data, model, scenario, total):
    """the oracle on a scenario as evaluate.py serves it -> (sc, top ids [n_lines, total], ranks)"""
    import evaluate
    import foldin
    import textio
    uids, vids = evaluate.read_ids(os.path.join(data, 'uid')), evaluate.read_ids(os.path.join(data, 'vid'))
    sc = evaluate.load_scenario(data, 0, scenario, uids, where='host')
    R = textio.parse_ratings(os.path.join(data, 'f0tr.txt'), textio.IdMap(uids), textio.IdMap(vids))
    lp, lc = foldin.liked_csr(R, len(uids), len(vids))
    hist = evaluate._take_rows(lp, lc, sc.users)
    col_of_item = np.full(len(vids), -1, np.int32)
    for tok, col in sc.teids.items():
        col_of_item[vids[tok]] = col
    s = O.scores(*hist, model.nbr_ids, model.nbr_w, col_of_item, len(sc.teids))
    masked = O.masked_columns(sc.rated_ptr, sc.rated_cols, len(sc.users), len(sc.teids))
    return sc, O.topk(s, masked, total)[0], O.ranks(s, masked, sc.like_ptr, sc.like_cols)


def test_train_g2_then_evaluate(tmp_path):
    import evaluate
    import rankmetrics
    model = _trained(G2, 5, str(tmp_path / 'knn'))
    up, uc, ip, _, _, n_items = g2_likes()
    want = O.build(up, uc, n_items, O.norms(np.diff(ip), 'cosine'), 0.0, 5)[:2]
    _same_table((model.nbr_ids, model.nbr_w), want)
    assert sorted(os.listdir(str(tmp_path / 'knn'))) == ['knn.npz']
    lines = evaluate.main(['-d', G2, '-m', str(tmp_path / 'knn'), '-sl', 'im', '-M', 'auc', 'ndcg'])
    sc, top, ranks = _oracle_scenario(G2, model, 'im', 30)
    hits = np.zeros(6, np.int64)
    for r in range(len(sc.users)):
        mine = set(sc.like_cols[sc.like_ptr[r]:sc.like_ptr[r + 1]].tolist())
        for p, col in enumerate(top[r]):
            if col in mine:
                hits[p // 5:] += 1
    assert lines[0] == 'im' + ''.join(',%.6f' % (float(h) / sc.tcount) for h in hits)
    vals = rankmetrics.finish(rankmetrics.rank_sums(ranks, sc.like_ptr, sc.rated_ptr, len(sc.teids), 5, 30), ['auc', 'ndcg'])
    assert lines[1:] == ['im.%s' % m + ''.join(',%.6f' % v for v in vals[m]) for m in ('auc', 'ndcg')]


def test_train_g4_then_compare_both_ways(tmp_path):
    import evaluate
    data = os.path.join(G4, 'data')
    _trained(data, 10, str(tmp_path / 'knn'))
    common = ['-d', data, '-sl', 'im', '-M', 'ndcg', 'acc', '--bootstrap', '50']
    one = evaluate.main(common + ['-m', str(tmp_path / 'knn'), '--compare', os.path.join(G4, 'model')])
    two = evaluate.main(common + ['-m', os.path.join(G4, 'model'), '--compare', str(tmp_path / 'knn')])
    for lines in (one, two):
        names = [ln.split(',')[0] for ln in lines]
        for name in ('im.diff.ndcg', 'im.diff.ndcg.lo', 'im.diff.ndcg.hi', 'im.diff.ndcg.p', 'im.vs.ndcg', 'im.diff.acc'):
            assert name in names, name
    row = lambda lines, name: [ln for ln in lines if ln.split(',')[0] == name][0].split(',')[1:]
    assert row(one, 'im.ndcg') == row(two, 'im.vs.ndcg') and row(two, 'im.ndcg') == row(one, 'im.vs.ndcg')
    assert two[0] == evaluate.main(['-d', data, '-sl', 'im', '-m', os.path.join(G4, 'model')])[0]      # a factor directory: as before


def test_recommend_lines_and_a_new_user(tmp_path):
    import evaluate
    import recommend
    import textio
    model = _trained(G2, 5, str(tmp_path / 'knn'))
    out = str(tmp_path / 'out.txt')
    lines = recommend.main(['-d', G2, '-m', str(tmp_path / 'knn'), '-o', out, '-t', '40'])
    uids, vids = evaluate.read_ids(os.path.join(G2, 'uid')), evaluate.read_ids(os.path.join(G2, 'vid'))
    R = textio.parse_ratings(os.path.join(G2, 'f0tr.txt'), textio.IdMap(uids), textio.IdMap(vids))
    up, uc = g2_likes()[:2]
    users = list(uids)
    rows_of_user = {uids[u]: [r] for r, u in enumerate(users)}
    rated = recommend.rated_csr(R, rows_of_user, len(users), len(vids))
    hist = evaluate._take_rows(up, uc, np.asarray([uids[u] for u in users]))
    s = O.scores(*hist, model.nbr_ids, model.nbr_w, None, len(vids))
    ids, scores = O.topk(s, O.masked_columns(rated[0], rated[1], len(users), len(vids)), 40)
    assert lines == textio.format_lines(users, ids, scores, {i: t for t, i in vids.items()})
    assert lines == open(out).read().split('\n')[:-1]
    # a new user with the history line of a model user gets that user's list
    who = [ln.split(',')[0] for ln in open(os.path.join(G2, 'f0tr.txt')) if ':1' in ln][2]
    theirs = [ln for ln in open(os.path.join(G2, 'f0tr.txt')) if ln.split(',')[0] == who][-1]
    open(str(tmp_path / 'new_uid'), 'w').write('fresh\n')
    open(str(tmp_path / 'new_hist'), 'w').write('fresh,' + theirs.split(',', 1)[1])
    open(str(tmp_path / 'some'), 'w').write(who + '\n')
    both = recommend.main(['-d', G2, '-m', str(tmp_path / 'knn'), '-o', out, '-t', '10', '-u', str(tmp_path / 'some'), '--new-uid',
                           str(tmp_path / 'new_uid'), '--new-history', str(tmp_path / 'new_hist'), '--fold-steps', '3'])
    assert len(both) == 2 and both[0].split(',')[0] == who and both[1].split(',')[0] == 'fresh'
    assert both[0].split(',')[1:] == both[1].split(',')[1:] and len(both[0].split(',')) > 5
