"""K10 (tkr_bpr_foldin_items) without a GPU: the ABI, the oracle's draw and step (tests/_item_foldin_oracle.py), the role thresholds,
what folding items in is worth on held-out items, and the host side of recommend.py --new-vid."""
import ctypes as C
import os
import re
import sys
import time

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _foldin_oracle as O9
import _item_foldin_oracle as O
from test_foldin_cpu import _latent_data, _train_oracle

from oracle import plan_np as P
from oracle import ref_np as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

V_, I32, F_, U64 = C.c_void_p, C.c_int32, C.c_float, C.c_uint64
ARGTYPES = [V_, V_, V_, I32, I32, I32, V_, V_, V_, V_, V_, I32, V_, V_, F_, F_, F_, F_, I32, I32, I32, U64, U64, V_, V_, V_, V_, V_]

N_USERS, N_ITEMS, shapes = O.N_USERS, O.N_ITEMS, O.shapes


def test_header_binding_and_library_declare_foldin_items():
    import tkr_hip
    header = open(os.path.join(ROOT, 'include', 'tkr.h')).read()
    assert 'tkr_bpr_foldin_items' in re.findall(r'^int(?:32_t|64_t)? (tkr_\w+)\(', header, flags=re.M)
    assert re.search(r'#define TKR_VERSION 120\b', header) and tkr_hip.VERSION == 120
    assert 'tkr_bpr_foldin_items' in tkr_hip.EXPORTS and callable(tkr_hip.fold_in_items)
    lib = C.CDLL(tkr_hip.LIB_PATH)
    assert lib.tkr_version() == 120
    fn = lib.tkr_bpr_foldin_items
    fn.restype = C.c_int
    fn.argtypes = ARGTYPES
    p = 4096                                                          # never dereferenced: every call below fails its checks
    good = dict(U=p, V=p, b=None, n_users=30, n_items=50, k=8, uptr=p, ucols=p, lptr=p, lrows=p, thresh=p, m=4, V0=None, b0=None, li=2.5e-3,
                lj=2.5e-4, lb=0.0, lr=0.05, mode=0, steps=5, P=16, seed=1, first=0, Vn=p, bn=p, loss=None, trip=None, stream=None)
    assert len(good) == len(ARGTYPES)
    for change in (dict(U=None), dict(V=None), dict(uptr=None), dict(ucols=None), dict(lptr=None), dict(lrows=None), dict(thresh=None),
                   dict(Vn=None), dict(bn=None), dict(P=0), dict(P=65), dict(steps=0), dict(mode=2), dict(lr=float('nan')), dict(m=-1),
                   dict(n_users=0), dict(n_items=0), dict(k=0), dict(li=float('nan'))):
        assert fn(*dict(good, **change).values()) == -1, change
    assert fn(*dict(good, m=0).values()) == 0                         # nothing to do is not an error (and launches nothing)


def test_oracle_draw_roles_membership_first_row_and_streams():
    uptr, ucols, rows, lptr, lrows, likers = shapes()
    T, Pn, seed = 6, 16, 99
    thresh = np.array([1 << 31, 1 << 31, 1 << 31, 1 << 30, 3 << 30, 1 << 31, 1 << 31, 0], dtype=np.int64)
    before9 = O9.draw(uptr, ucols, N_ITEMS, seed, T, Pn)
    before1 = P.sample_triplets(np.flatnonzero(np.diff(uptr) > 0), uptr.astype(np.int32), ucols, ucols, N_ITEMS, seed, 0, 500)
    trip, word = O.draw(uptr, ucols, lptr, lrows, thresh, N_ITEMS, seed, T, Pn)
    assert trip.shape == (8, T, Pn, 3) and word.shape == (8, T, Pn)
    udeg = np.diff(uptr)
    seen = {1: 0, 0: 0, -1: 0}
    for x in range(8):
        L = set(likers[x].tolist())
        nonlikers_with_row = [u for u in range(N_USERS) if udeg[u] > 0 and u not in L]
        for t in range(T):
            for p in range(Pn):
                role, u, o = (int(v) for v in trip[x, t, p])
                want_pos = int(word[x, t, p]) < thresh[x]
                seen[role] += 1
                if role == 1:
                    assert want_pos and u in L and o not in rows[u] and 0 <= o < N_ITEMS
                elif role == 0:
                    assert not want_pos and u not in L and udeg[u] > 0 and o in rows[u]
                else:                                                 # only where no legal draw exists
                    assert (u, o) == (-1, -1)
                    if want_pos:                                      # no liker at all, or the drawn one's row is the catalogue
                        assert len(L) == 0 or any(udeg[q] == N_ITEMS for q in L)
                    else:
                        assert not nonlikers_with_row
    assert seen[1] > 200 and seen[0] > 200 and seen[-1] > 30
    assert np.all(trip[5, :, :, 0] <= 0) and np.all(trip[7, :, :, 0] == 0)            # no liker / threshold 0: never the positive
    assert np.all(trip[6, :, :, 0] != 0)                              # everybody likes it: no user left for the negative role
    assert not np.any(trip[0, :, :, 0] == 1) and np.any(trip[0, :, :, 0] == -1)       # its only liker has no free column
    assert np.any(trip[1, :, :, 1] == 12) and np.any(trip[1, :, :, 1] == 4)           # the liker without a row, the one with one free column
    only = int(np.setdiff1d(np.arange(N_ITEMS), rows[4])[0])
    assert np.all(trip[1][trip[1, :, :, 1] == 4][:, 2] == only)
    always = np.full(8, O.ALWAYS, dtype=np.int64)
    ta, _ = O.draw(uptr, ucols, lptr, lrows, always, N_ITEMS, seed, T, Pn)
    assert np.all(ta[:, :, :, 0] != 0) and np.all(ta[5] == -1)
    # deterministic; another seed another draw; a block of items alone (first_row = its offset) = inside the larger call
    np.testing.assert_array_equal(trip, O.draw(uptr, ucols, lptr, lrows, thresh, N_ITEMS, seed, T, Pn)[0])
    assert not np.array_equal(trip, O.draw(uptr, ucols, lptr, lrows, thresh, N_ITEMS, seed + 1, T, Pn)[0])
    l2, r2 = O.csr(likers[2:5])
    np.testing.assert_array_equal(O.draw(uptr, ucols, l2, r2, thresh[2:5], N_ITEMS, seed, T, Pn, first_row=2)[0], trip[2:5])
    np.testing.assert_array_equal(O.draw(uptr, ucols, l2, r2, thresh[2:5], N_ITEMS, seed, T, Pn, first_row=(1 << 40) + 2)[0],
                                  O.draw(uptr, ucols, lptr, lrows, thresh, N_ITEMS, seed, T, Pn, first_row=1 << 40)[0][2:5])
    assert not np.array_equal(O.draw(uptr, ucols, l2, r2, thresh[2:5], N_ITEMS, seed, T, Pn)[0], trip[2:5])
    # K1's and K9's oracle draws under the same seed are what they were, and running them changes nothing here
    np.testing.assert_array_equal(before9, O9.draw(uptr, ucols, N_ITEMS, seed, T, Pn))
    after1 = P.sample_triplets(np.flatnonzero(np.diff(uptr) > 0), uptr.astype(np.int32), ucols, ucols, N_ITEMS, seed, 0, 500)
    for a, b in zip(before1, after1):
        np.testing.assert_array_equal(a, b)
    np.testing.assert_array_equal(trip, O.draw(uptr, ucols, lptr, lrows, thresh, N_ITEMS, seed, T, Pn)[0])


def test_draw_streams_are_disjoint_and_pinned():
    """4 users, 12 items, one new item liked by users 0 and 2, seed 7: a dozen (role, u, other) triplets of stream word 2 pinned
    as literals, so that the stream cannot move unnoticed"""
    rows = [np.array([1, 5, 9], np.int32), np.array([0, 2], np.int32), np.array([3, 4, 5, 6, 11], np.int32), np.array([7], np.int32)]
    uptr, ucols = O.csr(rows)
    lptr, lrows = O.csr([np.array([0, 2], np.int32)])
    trip, _ = O.draw(uptr, ucols, lptr, lrows, [1 << 31], 12, 7, 3, 4)
    got = trip.reshape(12, 3).tolist()
    assert got == PINNED


PINNED = [[1, 0, 8], [1, 2, 8], [1, 0, 8], [1, 0, 11], [0, 1, 2], [1, 0, 7], [1, 2, 2], [0, 1, 0], [1, 2, 0], [1, 2, 7], [0, 1, 0], [0, 1, 2]]


def test_role_thresholds_equal_a_direct_loop():
    import foldin
    import tkr_hip
    uptr, ucols, rows, lptr, lrows, likers = shapes()
    got = foldin.role_thresholds(uptr, lptr, lrows, N_ITEMS)
    want = O.role_thresh(uptr, lptr, lrows, N_ITEMS)
    print(got.tolist())
    np.testing.assert_array_equal(got, want)
    assert got[5] == 0 and got[6] == tkr_hip.ROLE_ALWAYS_POSITIVE and 0 < got[7] < got[2] < got[3] < got[4] < 2 ** 32
    assert np.all(foldin.role_thresholds(uptr, lptr, lrows, N_ITEMS, roles='positive') == tkr_hip.ROLE_ALWAYS_POSITIVE)
    with pytest.raises(ValueError):
        foldin.role_thresholds(uptr, lptr, lrows, N_ITEMS, roles='negative')
    # nobody but the likers has a row: always the positive, whatever the weights
    p2, _ = O.csr([[1, 2], [], [3]])
    l2, r2 = O.csr([[0, 2], [0], []])
    assert foldin.role_thresholds(p2, l2, r2, 10).tolist() == [O.ALWAYS, int(2 ** 32 * (1 / 3) / (1 / 3 + 1 / 10)), 0]
    np.testing.assert_array_equal(foldin.role_thresholds(p2, l2, r2, 10), O.role_thresh(p2, l2, r2, 10))


def _state(rng, n_users, n_items, k):
    U = (rng.standard_normal((n_users, k)) * 0.1).astype(np.float32)
    V = (rng.standard_normal((n_items, k)) * 0.1).astype(np.float32)
    b = (rng.standard_normal(n_items) * 0.1).astype(np.float32)
    return U, V, b


@pytest.mark.parametrize('mode', ['l2', 'l1'])
def test_one_oracle_step_is_bpr_step_with_the_item_appended(mode):
    """the new row after one step is bit for bit the row bpr_step gives the appended item; U, V, b and their slots are unchanged;
    the written-out formulas (sums in the order p) agree to rounding, in both modes, with and without biases"""
    uptr, ucols, rows, lptr, lrows, likers = shapes()
    rng = np.random.Generator(np.random.PCG64(3))
    k, Pn = 24, 16
    U, V, b = _state(rng, N_USERS, N_ITEMS, k)
    thresh = np.array([1 << 31] * 7 + [0], dtype=np.int64)
    trip, _ = O.draw(uptr, ucols, lptr, lrows, thresh, N_ITEMS, 21, 1, Pn)
    V0 = (rng.standard_normal((8, k)) * 0.1).astype(np.float32)
    b0 = (rng.standard_normal(8) * 0.1).astype(np.float32)
    hp = dict(lu=0.0, li=2.5e-3, lj=2.5e-4, lb=1e-3, lr=0.05, mode=mode)
    Vn, bn, loss = O.fold_in_items(U, V, b, trip, hp['li'], hp['lj'], hp['lb'], hp['lr'], mode, V0=V0, b0=b0)
    for x in range(8):
        tr = trip[x, 0][trip[x, 0, :, 0] >= 0]
        if len(tr) == 0:
            np.testing.assert_array_equal(Vn[x], V0[x])
            assert bn[x] == b0[x] and loss[x] == 0
            continue
        st = dict(U=U.copy(), V=np.concatenate([V, V0[x:x + 1]]), b=np.concatenate([b, b0[x:x + 1]]), msU=np.ones_like(U),
                  msV=np.ones((N_ITEMS + 1, k), np.float32), msb=np.ones(N_ITEMS + 1, np.float32))
        pos = tr[:, 0] == 1
        R.bpr_step(st, tr[:, 1], np.where(pos, N_ITEMS, tr[:, 2]), np.where(pos, tr[:, 2], N_ITEMS), hp)
        np.testing.assert_array_equal(Vn[x], st['V'][N_ITEMS])
        assert bn[x] == st['b'][N_ITEMS] and not np.array_equal(Vn[x], V0[x])
        assert not np.array_equal(st['V'][:N_ITEMS], V)              # ... which the plain step did change
    Vd, bd, lossd = O.fold_in_items_direct(U, V, b, trip, hp['li'], hp['lj'], hp['lb'], hp['lr'], mode, V0=V0, b0=b0)
    np.testing.assert_allclose(Vd, Vn, rtol=2e-5, atol=1e-7)
    np.testing.assert_allclose(bd, bn, rtol=2e-5, atol=1e-7)
    np.testing.assert_allclose(lossd, loss, rtol=2e-5, atol=1e-6)
    # without biases: none learnt, the start bias comes back; three steps from zeros
    trip3, _ = O.draw(uptr, ucols, lptr, lrows, thresh, N_ITEMS, 21, 3, Pn)
    Vn, bn, loss = O.fold_in_items(U, V, None, trip3, hp['li'], hp['lj'], hp['lb'], hp['lr'], mode, b0=b0)
    Vd, bd, lossd = O.fold_in_items_direct(U, V, None, trip3, hp['li'], hp['lj'], hp['lb'], hp['lr'], mode, b0=b0)
    np.testing.assert_array_equal(bn, b0)
    np.testing.assert_array_equal(bd, b0)
    np.testing.assert_allclose(Vd, Vn, rtol=1e-4, atol=1e-6)
    np.testing.assert_allclose(lossd, loss, rtol=1e-4, atol=1e-6)
    assert np.abs(Vn[1]).max() > 1e-3


def _held_item_data(seed=17, n_users=600, n_items=300, n_held=30):
    """the planted low-rank data of the K9 test; n_held items (about 10 %) leave the catalogue.  -> the users' likes over all items,
    the same over the kept catalogue (re-indexed), the held items, old -> new column map"""
    train, _ = _latent_data(seed, n_users, n_items)
    rng = np.random.Generator(np.random.PCG64(seed + 1))
    held = np.sort(rng.choice(n_items, n_held, replace=False))
    new_of = np.full(n_items, -1, dtype=np.int64)
    kept = np.setdiff1d(np.arange(n_items), held)
    new_of[kept] = np.arange(len(kept))
    part = [np.sort(new_of[t][new_of[t] >= 0]) for t in train]
    return train, part, held, kept


def test_folded_in_items_rank_like_trained_in_items():
    """600 x 300 planted low-rank data, k = 16, 30 items (10 %) held out of training entirely.  For every (held item x, liker u): the
    share of the items u has not rated that x outranks for u, averaged -- with (a) the zero row and bias (untrained), (b) x folded
    in at the defaults against a model trained on the other 270 items, (c) x trained in by a model that saw all 300.
    Required: (b) >= (a) + half of (c) - (a).
    Measured with the oracle alone (data seed 17, defaults steps 50, triplets 16, lr 0.05, which this measurement chose):
    untrained 0.6633, folded in 0.9427, trained in 0.9642 (required: >= 0.8138).  roles='positive' gives 0.9741 for the likers, but
    the users who do NOT like x then see it above 0.7314 of their unrated items, against 0.6913 with both roles."""
    import foldin
    t0 = time.time()
    n_users, n_items, k = 600, 300, 16
    train, part, held, kept = _held_item_data()
    hp = dict(lu=2.5e-3, li=2.5e-3, lj=2.5e-4, lb=0.0, lr=0.05, mode='l2')
    full = _train_oracle(train, np.arange(n_users), n_users, n_items, k, hp, 750, 256, 1)
    model = _train_oracle(part, np.arange(n_users), n_users, len(kept), k, hp, 750, 256, 1)
    likers = [np.flatnonzero([x in set(t.tolist()) for t in train]).astype(np.int32) for x in held]
    uptr, ucols = O.csr(part)
    lptr, lrows = O.csr(likers)
    rated_full = [np.searchsorted(kept, t[np.isin(t, kept)]) for t in train]
    share_trained = O.outrank_share(full['U'], full['V'][held], full['b'][held], full['V'][kept], full['b'][kept], likers, rated_full)
    share_zero = O.outrank_share(model['U'], np.zeros((len(held), k), np.float32), np.zeros(len(held), np.float32), model['V'], model['b'], likers, part)
    shares = {}
    for roles in ('both', 'positive'):
        thresh = foldin.role_thresholds(uptr, lptr, lrows, len(kept), roles)
        trip, _ = O.draw(uptr, ucols, lptr, lrows, thresh, len(kept), 0, foldin.ITEM_STEPS, foldin.ITEM_TRIPLETS)
        Vn, bn, _ = O.fold_in_items(model['U'], model['V'], model['b'], trip, hp['li'], hp['lj'], hp['lb'], foldin.ITEM_LR, 'l2')
        shares[roles] = O.outrank_share(model['U'], Vn, bn, model['V'], model['b'], likers, part)
        # the other side of the coin: how high x ranks for the users who do NOT like it (lower is better)
        non = [np.setdiff1d(np.arange(n_users), L)[::7] for L in likers]
        shares[roles + ' non-likers'] = O.outrank_share(model['U'], Vn, bn, model['V'], model['b'], non, part)
    print('share of unrated items outranked: untrained %.4f, folded in %.4f (positive role only %.4f), trained in %.4f; for non-likers: '
          'folded in %.4f, positive role only %.4f  (%.1f s)' % (share_zero, shares['both'], shares['positive'], share_trained,
                                                                shares['both non-likers'], shares['positive non-likers'], time.time() - t0))
    assert shares['both'] >= share_zero + 0.5 * (share_trained - share_zero)


def test_recommend_new_item_argument_errors(golden_dir, tmp_path):
    """refused on the host, before anything asks for a GPU"""
    import recommend
    d = os.path.join(golden_dir, 'g4')
    base = ['-d', os.path.join(d, 'data'), '-m', os.path.join(d, 'model'), '-o', str(tmp_path / 'out.txt')]
    some = tmp_path / 'vid'
    some.write_text('brand-new\n')
    for half in (['--new-vid', str(some)], ['--new-ratings', str(some)]):
        with pytest.raises(SystemExit):
            recommend.main(base + half)
    known = tmp_path / 'known'
    known.write_text('brand-new\n%s\n' % open(os.path.join(d, 'data', 'vid')).read().split()[2])
    with pytest.raises(KeyError, match='in the model already'):
        recommend.main(base + ['--new-vid', str(known), '--new-ratings', os.path.join(d, 'data', 'f0tr.txt')])
    assert not (tmp_path / 'out.txt').exists()
