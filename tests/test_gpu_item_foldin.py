"""K10 (tkr_bpr_foldin_items, csrc/foldin_items.hip), foldin.fold_in_items, BPR.fold_in_items and recommend.py --new-vid on the GPU,
against tests/_item_foldin_oracle.py.  The draw is integer and compared exactly; rows, biases and losses at the project's step
tolerance (rtol 2e-4, atol 1e-5, as tests/test_gpu_foldin.py)."""
import os
import shutil
import sys
import warnings

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _item_foldin_oracle as O

from oracle import ref_np as R

import tkr_hip

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RTOL, ATOL = 2e-4, 1e-5
N_USERS, N_ITEMS = O.N_USERS, O.N_ITEMS
THRESH = np.array([1 << 31, 1 << 31, 1 << 31, 1 << 30, 3 << 30, 1 << 31, 1 << 31, 0], dtype=np.int64)
HP = dict(li=2.5e-3, lj=2.5e-4, lb=1e-3, lr=0.05)


def _dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to('cuda')


def _fold(U, V, b, uptr, ucols, lptr, lrows, thresh, **kw):
    V0, b0 = kw.pop('V0', None), kw.pop('b0', None)
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')                               # (k = 600: the one warning of the generic form)
        out = tkr_hip.fold_in_items(_dev(U), _dev(V), _dev(b), _dev(uptr), _dev(ucols), _dev(lptr), _dev(lrows), thresh, V0=_dev(V0), b0=_dev(b0), **kw)
    return tuple(t.cpu().numpy() for t in out)


@pytest.fixture(scope='module')
def data():
    uptr, ucols, rows, lptr, lrows, likers = O.shapes()
    return dict(csr=(uptr, ucols, lptr, lrows), rows=rows, likers=likers)


def _factors(k, seed=1):
    rng = np.random.Generator(np.random.PCG64(seed * 1000 + k))
    U = (rng.standard_normal((N_USERS, k)) * 0.1).astype(np.float32)
    V = (rng.standard_normal((N_ITEMS, k)) * 0.1).astype(np.float32)
    b = (rng.standard_normal(N_ITEMS) * 0.1).astype(np.float32)
    V0 = (rng.standard_normal((8, k)) * 0.1).astype(np.float32)
    b0 = (rng.standard_normal(8) * 0.1).astype(np.float32)
    return U, V, b, V0, b0


@pytest.mark.parametrize('Pn', [1, 16, 64])
def test_draw_equals_oracle_exactly(data, Pn):
    """both roles, likers without a row / without a free column, items nobody and everybody likes, threshold 0; first_row small and
    above 2^32 / steps / triplets (the second counter word moves)"""
    U, V, b, _, _ = _factors(16)
    T = 5
    for seed, first in ((7, 0), ((1 << 63) + 99, (1 << 40) + 3)):
        trip = _fold(U, V, b, *data['csr'], THRESH, steps=T, triplets=Pn, seed=seed, first_row=first, want_triplets=True, **HP)[2]
        want, _ = O.draw(*data['csr'][:2], *data['csr'][2:], THRESH, N_ITEMS, seed, T, Pn, first_row=first)
        np.testing.assert_array_equal(trip, want, err_msg=str((seed, first)))
    always = np.full(8, O.ALWAYS, dtype=np.int64)
    trip = _fold(U, V, b, *data['csr'], always, steps=T, triplets=Pn, seed=3, want_triplets=True, **HP)[2]
    np.testing.assert_array_equal(trip, O.draw(*data['csr'], always, N_ITEMS, 3, T, Pn)[0])
    assert np.all(trip[:, :, :, 0] != 0)


@pytest.mark.parametrize('k', [4, 64, 128, 600])
def test_short_run_matches_oracle(data, k):
    """three steps of 16 triplets; l2 and l1, with and without item biases, from zeros and from given rows and biases.
    k = 4: a partial row in registers, 64 / 128: the vector rows, 600: the LDS form."""
    U, V, b, V0, b0 = _factors(k)
    T, Pn = 3, 16
    trip, _ = O.draw(*data['csr'], THRESH, N_ITEMS, 11, T, Pn)
    for mode in ('l2', 'l1'):
        for bias in (None, b):
            for start in ((None, None), (V0, b0)):
                Vn, bn, loss, got_trip = _fold(U, V, bias, *data['csr'], THRESH, mode=mode, steps=T, triplets=Pn, seed=11, V0=start[0], b0=start[1],
                                               want_loss=True, want_triplets=True, **HP)
                np.testing.assert_array_equal(got_trip, trip)
                wantV, wantb, want_loss = O.fold_in_items(U, V, bias, trip, HP['li'], HP['lj'], HP['lb'], HP['lr'], mode, V0=start[0], b0=start[1])
                what = str((k, mode, bias is not None, start[0] is not None))
                print(what, 'max |V - oracle| = %.3g, |b - oracle| = %.3g, |loss - oracle| = %.3g'
                      % (np.abs(Vn - wantV).max(), np.abs(bn - wantb).max(), np.abs(loss - want_loss).max()))
                np.testing.assert_allclose(Vn, wantV, rtol=RTOL, atol=ATOL, err_msg=what)
                np.testing.assert_allclose(bn, wantb, rtol=RTOL, atol=ATOL, err_msg=what)
                np.testing.assert_allclose(loss, want_loss, rtol=RTOL, atol=ATOL, err_msg=what)
                if bias is None:                                      # no bias learnt: the start value comes back
                    np.testing.assert_array_equal(bn, np.zeros(8, np.float32) if start[1] is None else start[1])
                assert np.abs(Vn[1] - (0 if start[0] is None else start[0][1])).max() > 1e-3


@pytest.mark.parametrize('k', [50, 128])
def test_default_depth_within_measured_tolerance(data, k):
    """the default depth (foldin.ITEM_STEPS steps of ITEM_TRIPLETS triplets).  d = the largest elementwise distance between the
    direct oracle in fp32 and in fp64 on the same triplets; the kernel must lie within max(project tolerance, 4 d) of the fp64
    result (4: a wave sums in another order than NumPy), as K9's test does."""
    import foldin
    U, V, b, _, _ = _factors(k, seed=2)
    T, Pn = foldin.ITEM_STEPS, foldin.ITEM_TRIPLETS
    Vn, bn, trip = _fold(U, V, b, *data['csr'], THRESH, steps=T, triplets=Pn, seed=5, want_triplets=True, **HP)
    np.testing.assert_array_equal(trip, O.draw(*data['csr'], THRESH, N_ITEMS, 5, T, Pn)[0])
    V32, b32, _ = O.fold_in_items_direct(U, V, b, trip, HP['li'], HP['lj'], HP['lb'], HP['lr'], dtype=np.float32)
    V64, b64, _ = O.fold_in_items_direct(U, V, b, trip, HP['li'], HP['lj'], HP['lb'], HP['lr'], dtype=np.float64)
    got, w32, w64 = (np.concatenate([v.astype(np.float64), np.asarray(c, np.float64)[:, None]], axis=1) for v, c in ((Vn, bn), (V32, b32), (V64, b64)))
    d = float(np.abs(w32 - w64).max())
    dist = np.abs(got - w64)
    bound = np.maximum(ATOL + RTOL * np.abs(w64), 4 * d)
    print('k = %d: d(fp32 oracle, fp64 oracle) = %.3g, kernel to fp64 = %.3g, max |v| = %.3g, tightest bound used = %.3g'
          % (k, d, float(dist.max()), float(np.abs(w64).max()), float(bound.min())))
    assert np.all(dist <= bound), float((dist - bound).max())


@pytest.mark.parametrize('k', [128, 600])
def test_split_by_first_row_and_two_runs_are_bitwise_equal(data, k):
    U, V, b, V0, b0 = _factors(k)
    uptr, ucols, lptr, lrows = data['csr']
    kw = dict(steps=4, triplets=16, seed=9, want_loss=True, **HP)
    whole = _fold(U, V, b, uptr, ucols, lptr, lrows, THRESH, first_row=5, V0=V0, b0=b0, **kw)
    again = _fold(U, V, b, uptr, ucols, lptr, lrows, THRESH, first_row=5, V0=V0, b0=b0, **kw)
    for a, c in zip(whole, again):
        np.testing.assert_array_equal(a, c)
    cut = 3
    head = _fold(U, V, b, uptr, ucols, lptr[:cut + 1], lrows[:lptr[cut]], THRESH[:cut], first_row=5, V0=V0[:cut], b0=b0[:cut], **kw)
    tail = _fold(U, V, b, uptr, ucols, lptr[cut:] - lptr[cut], lrows[lptr[cut]:], THRESH[cut:], first_row=5 + cut, V0=V0[cut:], b0=b0[cut:], **kw)
    for a, h, t in zip(whole, head, tail):
        np.testing.assert_array_equal(a, np.concatenate([h, t]))      # bitwise: an item does not see who shares its call


@pytest.mark.parametrize('k', [16, 600])
def test_edge_items_return_and_an_item_without_triplets_keeps_its_start(data, k):
    """items with 0 and with 300 likers and a threshold of 0 come back (the scans are bounded); an item whose every triplet has no
    legal draw -- nobody likes it and it is always the positive; everybody likes it and it is never -- keeps V0, b0, loss 0"""
    U, V, b, V0, b0 = _factors(k)
    uptr, ucols, lptr, lrows = data['csr']
    for thresh in (np.zeros(8, np.int64), np.full(8, O.ALWAYS, np.int64)):
        for start in ((None, None), (V0, b0)):
            Vn, bn, loss, trip = _fold(U, V, b, uptr, ucols, lptr, lrows, thresh, steps=3, triplets=16, seed=2, V0=start[0], b0=start[1], want_loss=True,
                                       want_triplets=True, **HP)
            np.testing.assert_array_equal(trip, O.draw(uptr, ucols, lptr, lrows, thresh, N_ITEMS, 2, 3, 16)[0])
            assert np.isfinite(Vn).all() and np.isfinite(bn).all()
            for x in (6,) if thresh[0] == 0 else (5, 0):              # (item 0's only liker has no free column)
                assert np.all(trip[x] == -1)
                np.testing.assert_array_equal(Vn[x], np.zeros(k, np.float32) if start[0] is None else start[0][x])
                assert bn[x] == (0 if start[1] is None else start[1][x]) and loss[x] == 0
            assert np.abs(Vn[3] - (0 if start[0] is None else start[0][3])).max() > 1e-3


def test_wrapper_refuses_bad_arguments(data):
    U, V, b, _, _ = _factors(4)
    uptr, ucols, lptr, lrows = (_dev(a) for a in data['csr'])
    ok = dict(steps=1, triplets=4, seed=0, **HP)
    for change in (dict(triplets=0), dict(triplets=65), dict(steps=0)):
        with pytest.raises(ValueError):
            tkr_hip.fold_in_items(_dev(U), _dev(V), None, uptr, ucols, lptr, lrows, THRESH, **dict(ok, **change))
    bad_rows = lrows.clone()
    bad_rows[0] = N_USERS
    bad_cols = ucols.clone()
    bad_cols[5] = -1
    for args in ((uptr, ucols, lptr, bad_rows, THRESH), (uptr, bad_cols, lptr, lrows, THRESH), (uptr, ucols, lptr, lrows, THRESH[:7]),
                 (uptr, ucols, lptr, lrows, THRESH + (1 << 32))):
        with pytest.raises(AssertionError):
            tkr_hip.fold_in_items(_dev(U), _dev(V), None, *args, **ok)


# ---- recommend.py --new-vid and BPR.fold_in_items on golden G4 with its last five items cut out ----------------------------------
CUT = 5


def _parse_lines(path):
    out = []
    for ln in open(path).read().strip().split('\n'):
        f = ln.split(',')
        out.append((f[0], [t.split(':')[0] for t in f[1:]], [float(t.split(':')[1]) for t in f[1:]]))
    return out


@pytest.fixture()
def cut_g4(golden_dir, tmp_path):
    """G4 with the last five lines of vid and of final-V.dat cut out: data and model directories in tmp_path, the id file of the five
    items, and a ratings file that holds every user's likes of them (the train file's lines, then the out-of-matrix test lines:
    two of the five items are liked only there)"""
    src_data, src_model = os.path.join(golden_dir, 'g4', 'data'), os.path.join(golden_dir, 'g4', 'model')
    data, model = tmp_path / 'data', tmp_path / 'model'
    shutil.copytree(src_data, str(data))
    model.mkdir()
    tokens = open(os.path.join(src_data, 'vid')).read().split()
    (data / 'vid').write_text('\n'.join(tokens[:-CUT]) + '\n')
    shutil.copy(os.path.join(src_model, 'final-U.dat'), str(model / 'final-U.dat'))
    rows = open(os.path.join(src_model, 'final-V.dat')).read().strip('\n').split('\n')
    assert len(rows) == len(tokens)
    (model / 'final-V.dat').write_text('\n'.join(rows[:-CUT]) + '\n')
    (tmp_path / 'new_vid').write_text('\n'.join(tokens[-CUT:]) + '\n')
    (tmp_path / 'new_ratings').write_text(open(os.path.join(src_data, 'f0tr.txt')).read() + open(os.path.join(src_data, 'f0te.om.txt')).read())
    return dict(data=str(data), model=str(model), new_vid=str(tmp_path / 'new_vid'), new_ratings=str(tmp_path / 'new_ratings'), tokens=tokens,
                src_data=src_data, src_model=src_model)


def _cut_model_arrays(g):
    """uids, the cut vids, fue, the cut fie, the users' positives over the cut catalogue and the five items' likers"""
    uids = R.read_id_list(os.path.join(g['data'], 'uid'))
    vids = R.read_id_list(os.path.join(g['data'], 'vid'))
    new = {t: q for q, t in enumerate(g['tokens'][-CUT:])}
    umat = R.read_embed_text(os.path.join(g['model'], 'final-U.dat'), uids)
    vmat = R.read_embed_text(os.path.join(g['model'], 'final-V.dat'), vids)
    pos = [set() for _ in uids]
    for u, i in R.read_positive_pairs(os.path.join(g['data'], 'f0tr.txt'), uids, vids):
        pos[uids[u]].add(vids[i])
    likers = [set() for _ in new]
    for u, i in R.read_positive_pairs(g['new_ratings'], uids, new):
        likers[new[i]].add(uids[u])
    return uids, vids, new, umat, vmat, [sorted(p) for p in pos], [sorted(l) for l in likers]


def test_recommend_cli_folds_in_new_items(cut_g4, tmp_path):
    """the five items are folded back in through recommend.py --new-vid: every user's line is the canonical list of the product of
    final-U.dat with the cut catalogue grown by the ORACLE's rows for the five (same draw, same steps), every item on the user's
    history line or on its line of the new ratings file masked; scores within what '%f' prints.  Without the new flags the file is
    byte for byte what the code path of the parent commit writes."""
    import foldin
    import recommend
    g = cut_g4
    uids, vids, new, umat, vmat, pos, likers = _cut_model_arrays(g)
    assert all(len(l) > 0 for l in likers)
    out = tmp_path / 'rec.txt'
    recommend.main(['-d', g['data'], '-m', g['model'], '-t', '10', '-o', str(out), '--new-vid', g['new_vid'], '--new-ratings', g['new_ratings'], '--seed', '3'])
    got = _parse_lines(str(out))
    uptr, ucols = O.csr(pos)
    lptr, lrows = O.csr(likers)
    thresh = foldin.role_thresholds(uptr, lptr, lrows, len(vmat))
    np.testing.assert_array_equal(thresh, O.role_thresh(uptr, lptr, lrows, len(vmat)))
    trip, _ = O.draw(uptr, ucols, lptr, lrows, thresh, len(vmat), 3, 50, 16)
    Vo, _, _ = O.fold_in_items(umat, vmat, None, trip, 2.5e-3, 2.5e-4, 0.0, 0.05)
    grown = np.concatenate([vmat, Vo])
    tok_of = {i: v for v, i in vids.items()}
    tok_of.update({len(vmat) + q: t for t, q in new.items()})
    col_of = {t: c for c, t in tok_of.items()}
    rated = R.read_history(os.path.join(g['data'], 'f0tr.txt'))
    rated_new = R.read_history(g['new_ratings'])
    users = list(uids)
    rated_cols = [{col_of[v] for v in (rated.get(u, set()) | rated_new.get(u, set())) if v in col_of} for u in users]
    s = R.mfma_chain_scores(umat, grown, None)
    want = [R.filtered_topk(s[x], rated_cols[x], 10, canonical=True) for x in range(len(users))]
    assert [q[0] for q in got] == users
    hits = 0
    for x, (u, ids, scores) in enumerate(got):
        assert ids == [tok_of[c] for c in want[x]], u
        np.testing.assert_allclose(scores, s[x][want[x]], rtol=1e-6, atol=1.1e-6)
        hits += len(set(ids) & set(new))
    assert hits > 0                                                   # the new items are recommended under their own tokens
    # no new flag: the parent's code path, byte for byte
    recommend.main(['-d', g['src_data'], '-m', g['src_model'], '-t', '10', '-o', str(out)])
    all_uids, all_vids = recommend.read_ids(os.path.join(g['src_data'], 'uid')), recommend.read_ids(os.path.join(g['src_data'], 'vid'))
    import textio
    Rt = textio.parse_ratings(os.path.join(g['src_data'], 'f0tr.txt'), textio.IdMap(all_uids), textio.IdMap(all_vids))
    full_v = recommend.read_matrix(os.path.join(g['src_model'], 'final-V.dat'), all_vids)
    full_u = recommend.read_matrix(os.path.join(g['src_model'], 'final-U.dat'), all_uids)
    ids, scores = recommend.rank(_dev(full_u), [all_uids[u] for u in all_uids], _dev(full_v), None, Rt, 10)
    lines = recommend.format_lines(list(all_uids), ids, scores, {i: t for t, i in all_vids.items()})
    assert open(str(out), 'rb').read() == ('\n'.join(lines) + '\n').encode()


def test_append_export_and_evaluate_round_trip(cut_g4, tmp_path):
    """BPR.fold_in_items(append=True) grows the model by the five items; export_embeddings writes it; evaluate.py on the data
    directory whose vid has the five lines back runs, and the out-of-matrix scenario -- two of the five items are test columns
    there -- ranks the new columns: its figures are those of utils.evaluate's oracle on the grown factors"""
    import evaluate
    from single.bpr import BPR
    g = cut_g4
    uids, vids, new, umat, vmat, pos, likers = _cut_model_arrays(g)
    model = BPR(k=vmat.shape[1], lr=0.05)
    model.load_training_data(os.path.join(g['data'], 'uid'), os.path.join(g['data'], 'vid'), os.path.join(g['data'], 'f0tr.txt'))
    model.import_embeddings(g['model'])
    assert model.n_items == len(vmat) and model.fib is None
    model.fib = np.zeros((len(vmat), 1), np.float32)                  # (G4 was exported without biases: the new items learn theirs)
    got_ids, V_new, b_new = model.fold_in_items(g['new_vid'], g['new_ratings'], seed=3, append=True)
    assert got_ids == new and V_new.shape == (CUT, vmat.shape[1]) and b_new.shape == (CUT, 1) and b_new.all()
    assert model.n_items == len(vmat) + CUT and model.fie.shape == (len(vmat) + CUT, vmat.shape[1]) and model.fib.shape == (len(vmat) + CUT, 1)
    assert [model.iids[t] for t in g['tokens'][-CUT:]] == list(range(len(vmat), len(vmat) + CUT))
    uptr, ucols = O.csr(pos)
    lptr, lrows = O.csr(likers)
    import foldin
    trip, _ = O.draw(uptr, ucols, lptr, lrows, foldin.role_thresholds(uptr, lptr, lrows, len(vmat)), len(vmat), 3, foldin.ITEM_STEPS, foldin.ITEM_TRIPLETS)
    Vo, bo, _ = O.fold_in_items(umat, vmat, np.zeros(len(vmat), np.float32), trip, model.li, model.lj, model.lb, model.lr, model.mode)
    np.testing.assert_allclose(V_new, Vo, rtol=RTOL, atol=ATOL)
    np.testing.assert_allclose(b_new.reshape(-1), bo, rtol=RTOL, atol=ATOL)
    np.testing.assert_array_equal(model.fie[len(vmat):], V_new)
    np.testing.assert_array_equal(model.fib[len(vmat):], b_new)
    with pytest.raises(ValueError):                                   # they are in the model now
        model.fold_in_items(g['new_vid'], g['new_ratings'])
    out_model = tmp_path / 'grown'
    model.export_embeddings(str(out_model))
    shutil.copy(os.path.join(g['src_data'], 'vid'), os.path.join(g['data'], 'vid'))
    lines = evaluate.main(['-d', g['data'], '-m', str(out_model), '-f', '0', '-s', '5', '-t', '10', '-sl', 'om', 'im'])
    before = evaluate.main(['-d', g['src_data'], '-m', g['src_model'], '-f', '0', '-s', '5', '-t', '10', '-sl', 'om', 'im'])
    assert len(lines) == 2 and lines[0].startswith('om,') and lines[1].startswith('im,')
    all_vids = R.read_id_list(os.path.join(g['src_data'], 'vid'))
    grown = R.read_embed_text(os.path.join(str(out_model), 'final-V.dat'), all_vids)
    np.testing.assert_allclose(grown[len(vmat):], V_new, atol=1e-6)   # ('%f' text)
    np.testing.assert_array_equal(grown[:len(vmat)], vmat)
    print('\n'.join(['grown: ' + l for l in lines] + ['golden: ' + l for l in before]))
    # the new columns are ranked: the scenario's top-10 lists computed from the grown files hold them
    teids = R.read_id_list(os.path.join(g['src_data'], 'f0te.om.idl'))
    assert sum(t in teids for t in g['tokens'][-CUT:]) >= 2
    sc = evaluate.load_scenario(g['data'], 0, 'om', evaluate.read_ids(os.path.join(g['data'], 'uid')))
    grown_b = R.read_embed_text(os.path.join(str(out_model), 'final-B.dat'), all_vids)
    np.testing.assert_allclose(grown_b[len(vmat):], b_new, atol=1e-6)
    top = evaluate.rank_scenario(_dev(umat), grown, grown_b, all_vids, sc, 10, torch.device('cuda')).cpu().numpy()
    new_cols = [teids[t] for t in g['tokens'][-CUT:] if t in teids]
    assert np.isin(top, new_cols).any()
