"""K9 (tkr_bpr_foldin) without a GPU: the ABI, the oracle's draw and step (tests/_foldin_oracle.py), what fold-in is worth on
held-out users, and the host side of recommend.py."""
import ctypes as C
import os
import re
import sys
import time

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _foldin_oracle as O

from oracle import plan_np as P
from oracle import ref_np as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

FOLDIN_ARGTYPES = [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_float, C.c_float,
                   C.c_int32, C.c_int32, C.c_int32, C.c_uint64, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]


def test_header_binding_and_library_declare_foldin():
    import tkr_hip
    header = open(os.path.join(ROOT, 'include', 'tkr.h')).read()
    assert 'tkr_bpr_foldin' in re.findall(r'^int(?:32_t|64_t)? (tkr_\w+)\(', header, flags=re.M)
    assert re.search(r'#define TKR_VERSION 120\b', header) and tkr_hip.VERSION == 120
    assert 'tkr_bpr_foldin' in tkr_hip.EXPORTS and callable(tkr_hip.fold_in)
    lib = C.CDLL(tkr_hip.LIB_PATH)
    assert lib.tkr_version() == 120
    fn = lib.tkr_bpr_foldin
    fn.restype = C.c_int
    fn.argtypes = FOLDIN_ARGTYPES
    # arguments are checked before any device access: this runs on a machine without a GPU
    assert fn(None, None, 0, 0, None, None, 0, None, 0.0, 0.0, 0, 0, 0, 0, 0, None, None, None, None) == -1
    p = 4096                                                          # never dereferenced: every call below fails its checks
    good = dict(V=p, b=None, n_items=50, k=8, ptr=p, cols=p, m=4, U0=None, lu=2.5e-3, lr=0.05, mode=0, steps=5, P=16, seed=1, first=0,
                U=p, loss=None, trip=None, stream=None)
    for change in (dict(P=0), dict(P=65), dict(P=-1), dict(V=None), dict(ptr=None), dict(cols=None), dict(U=None), dict(n_items=0), dict(k=0),
                   dict(m=-1), dict(steps=0), dict(mode=2), dict(lr=float('nan'))):
        assert fn(*dict(good, **change).values()) == -1, change
    assert fn(*dict(good, m=0).values()) == 0                         # nothing to do is not an error (and launches nothing)


def _histories(rng, n_items, degrees):
    return [np.sort(rng.choice(n_items, d, replace=False)).astype(np.int32) for d in degrees]


def test_oracle_draw_membership_determinism_and_first_row():
    rng = np.random.Generator(np.random.PCG64(5))
    n_items, T, Pn = 400, 6, 16
    hist = _histories(rng, n_items, [1, 2, 37, 200, 399, 0, 400, 12])
    ptr, cols = O.csr(hist)
    trip = O.draw(ptr, cols, n_items, 99, T, Pn)
    assert trip.shape == (8, T, Pn, 2)
    for x, h in enumerate(hist):
        if len(h) in (0, n_items):                                    # no positive / no negative: no triplet
            assert np.all(trip[x] == -1)
            continue
        assert np.all(np.isin(trip[x, :, :, 0], h)) and not np.any(np.isin(trip[x, :, :, 1], h))
        assert trip[x, :, :, 1].min() >= 0 and trip[x, :, :, 1].max() < n_items
    only = np.setdiff1d(np.arange(n_items), hist[4])
    assert np.all(trip[4, :, :, 1] == only[0])                        # one column left: the rounds or the cyclic scan find it
    assert len(np.unique(trip[3, :, :, 0])) > 20 and len(np.unique(trip[3, :, :, 1])) > 20
    np.testing.assert_array_equal(trip, O.draw(ptr, cols, n_items, 99, T, Pn))
    assert not np.array_equal(trip, O.draw(ptr, cols, n_items, 100, T, Pn))
    # a block of users draws the same alone (first_row = its offset) as inside the larger call
    p2, c2 = O.csr(hist[2:5])
    np.testing.assert_array_equal(O.draw(p2, c2, n_items, 99, T, Pn, first_row=2), trip[2:5])
    np.testing.assert_array_equal(O.draw(ptr, cols, n_items, 99, T, Pn, first_row=7)[:1], O.draw(*O.csr(hist[:1]), n_items, 99, T, Pn, first_row=7))
    assert not np.array_equal(O.draw(p2, c2, n_items, 99, T, Pn, first_row=0), trip[2:5])


def test_oracle_draw_is_disjoint_from_training_stream_and_pinned():
    """one user with 5 positives of 40 items, seed 7: counter g of the fold-in stream is triplet g of K1's stream with another fourth
    counter word -- the pairs differ, and a dozen of them are pinned here as literals"""
    hist = [np.array([3, 11, 17, 29, 38], np.int32)]
    ptr, cols = O.csr(hist)
    trip = O.draw(ptr, cols, 40, 7, 3, 4)
    _, ti, tj = P.sample_triplets([0], ptr.astype(np.int32), cols, cols, 40, 7, 0, 12)
    k1 = np.stack([ti, tj], axis=1)
    got = trip.reshape(12, 2)
    assert np.sum(np.all(got == k1, axis=1)) <= 2                     # equal pairs only by chance (5 x 35 possible pairs)
    assert got.tolist() == [[3, 25], [29, 12], [29, 2], [29, 5], [38, 39], [11, 33], [17, 6], [3, 14], [38, 34], [38, 8], [29, 35], [38, 19]]


def _state(rng, m, n_items, k):
    st = R.init_bpr_state(m, n_items, k, rng)
    st['U'] = (rng.standard_normal((m, k)) * 0.1).astype(np.float32)
    st['V'] = (rng.standard_normal((n_items, k)) * 0.1).astype(np.float32)
    st['b'] = (rng.standard_normal(n_items) * 0.1).astype(np.float32)
    return st


@pytest.mark.parametrize('mode', ['l2', 'l1'])
def test_one_oracle_step_is_bpr_step_on_copies_of_the_user(mode):
    """bit for bit on the user row; V, b, msV, msb unchanged; several users in one call = each alone; the written-out formulas
    (the fp64 run of the GPU tests uses them) give the same bits in fp32"""
    rng = np.random.Generator(np.random.PCG64(3))
    m, n_items, k, Pn = 5, 60, 24, 16
    hist = _histories(rng, n_items, [4, 9, 30, 1, 17])
    ptr, cols = O.csr(hist)
    trip = O.draw(ptr, cols, n_items, 21, 1, Pn)
    st = _state(rng, m, n_items, k)
    hp = dict(lu=2.5e-3, li=0.0, lj=0.0, lb=0.0, lr=0.05, mode=mode)
    for x in range(m):                                                # the reference's step, by hand
        ref = {n: v.copy() for n, v in st.items()}
        want_loss = R.bpr_step(ref, np.full(Pn, x), trip[x, 0, :, 0], trip[x, 0, :, 1], hp)
        got = {n: v.copy() for n, v in st.items()}
        loss = O.step_ref(got, [x], trip[[x], 0], hp)
        assert loss == want_loss
        np.testing.assert_array_equal(got['U'][x], ref['U'][x])
        np.testing.assert_array_equal(got['msU'][x], ref['msU'][x])
        assert not np.array_equal(got['U'][x], st['U'][x])
        for n in ('V', 'b', 'msV', 'msb'):
            np.testing.assert_array_equal(got[n], st[n])
            assert not np.array_equal(ref[n], st[n])                # ... which the plain step did change
        others = [y for y in range(m) if y != x]
        np.testing.assert_array_equal(got['U'][others], st['U'][others])
    U, loss = O.fold_in(st['V'], st['b'], ptr, cols, trip, 2.5e-3, 0.05, mode, U0=st['U'])
    for x in range(m):
        ref = {n: v.copy() for n, v in st.items()}
        want_loss = R.bpr_step(ref, np.full(Pn, x), trip[x, 0, :, 0], trip[x, 0, :, 1], hp)
        np.testing.assert_array_equal(U[x], ref['U'][x])
        assert loss[x] == want_loss
    Ud, lossd = O.fold_in_direct(st['V'], st['b'], ptr, cols, trip, 2.5e-3, 0.05, mode, U0=st['U'], dtype=np.float32)
    np.testing.assert_array_equal(Ud, U)
    np.testing.assert_allclose(lossd, loss, rtol=1e-6)
    # several steps in one bpr_step per step (fold_in) = user by user
    trip3 = O.draw(ptr, cols, n_items, 21, 3, Pn)
    U3, _ = O.fold_in(st['V'], st['b'], ptr, cols, trip3, 2.5e-3, 0.05, mode)
    for x in range(m):
        one = dict(st, U=np.zeros((m, k), np.float32), msU=np.ones((m, k), np.float32))
        one = {n: v.copy() for n, v in one.items()}
        for t in range(3):
            O.step_ref(one, [x], trip3[[x], t], hp)
        np.testing.assert_array_equal(U3[x], one['U'][x])


def _latent_data(seed, n_users=600, n_items=300, k_true=8, n_like=40, n_held=10):
    """users and items from a latent-factor model plus an item popularity term; every user likes its n_like best items by a noisy
    score, n_held of them (drawn at random) are held out"""
    rng = np.random.Generator(np.random.PCG64(seed))
    pu, qi = rng.standard_normal((n_users, k_true)), rng.standard_normal((n_items, k_true))
    score = pu @ qi.T + 1.5 * rng.standard_normal(n_items)[None, :] + 0.5 * rng.standard_normal((n_users, n_items))
    likes = np.argsort(-score, axis=1)[:, :n_like]
    train, held = [], []
    for x in range(n_users):
        perm = rng.permutation(n_like)
        held.append(np.sort(likes[x, perm[:n_held]]))
        train.append(np.sort(likes[x, perm[n_held:]]))
    return train, held


def _train_oracle(train, users, n_users, n_items, k, hp, n_batches, B, seed):
    """BPR with the NumPy oracle on the listed users: u uniform over them, i uniform over its positives, j rejected while rated"""
    rng = np.random.Generator(np.random.PCG64(seed))
    st = R.init_bpr_state(n_users, n_items, k, rng)
    rated = np.zeros((n_users, n_items), dtype=bool)
    for x in users:
        rated[x, train[x]] = True
    users = np.asarray(users)
    for _ in range(n_batches):
        ub = users[rng.integers(0, len(users), B)]
        ib = np.array([train[x][rng.integers(0, len(train[x]))] for x in ub])
        jb = rng.integers(0, n_items, B)
        while True:
            bad = rated[ub, jb]
            if not bad.any():
                break
            jb[bad] = rng.integers(0, n_items, int(bad.sum()))
        R.bpr_step(st, ub, ib, jb, hp)
    return st


def test_folded_in_users_rank_like_trained_in_users():
    """600 x 300 latent-factor data, k = 16, the last 100 users held out of training.  AUC of their held-out likes (against the
    items they have not seen) with (a) rows trained in by a model that saw all 600 users, (b) rows folded in from zero vectors
    against a model that saw the other 500, (c) untrained rows = zero vectors, i.e. ranked by the item bias of that model.
    Required: (a) - (b) <= 0.02 and (b) - (c) >= 0.15."""
    t0 = time.time()
    n_users, n_items, k = 600, 300, 16
    train, held = _latent_data(17, n_users, n_items)
    hp = dict(lu=2.5e-3, li=2.5e-3, lj=2.5e-4, lb=0.0, lr=0.05, mode='l2')
    new = np.arange(500, 600)
    full = _train_oracle(train, np.arange(n_users), n_users, n_items, k, hp, 750, 256, 1)
    part = _train_oracle(train, np.arange(500), n_users, n_items, k, hp, 750, 256, 1)
    tr_new, held_new = [train[x] for x in new], [held[x] for x in new]
    auc_trained = O.auc_of(full['U'][new], full['V'], full['b'], tr_new, held_new)
    ptr, cols = O.csr(tr_new)
    trip = O.draw(ptr, cols, n_items, 0, 50, 16)
    U, _ = O.fold_in(part['V'], part['b'], ptr, cols, trip, hp['lu'], 0.05, 'l2')
    auc_folded = O.auc_of(U, part['V'], part['b'], tr_new, held_new)
    auc_untrained = O.auc_of(np.zeros_like(U), part['V'], part['b'], tr_new, held_new)
    print('AUC of held-out likes: trained-in %.4f, folded-in %.4f, untrained %.4f  (%.1f s)' % (auc_trained, auc_folded, auc_untrained, time.time() - t0))
    assert auc_trained - auc_folded <= 0.02
    assert auc_folded - auc_untrained >= 0.15


def test_recommend_line_formatter():
    import recommend
    items = {0: 'a', 1: 'b', 2: 'c10'}
    ids = np.array([[2, 0, 1], [1, -1, -1], [-1, -1, -1]], np.int32)
    scores = np.array([[1.5, 0.25, -0.125], [1e-7, -np.inf, -np.inf], [-np.inf] * 3], np.float32)
    assert recommend.format_lines(['u1', '77', 'x'], ids, scores, items) == ['u1,c10:1.500000,a:0.250000,b:-0.125000', '77,b:0.000000', 'x']
    assert recommend.format_lines([], ids[:0], scores[:0], items) == []


def test_recommend_argument_errors(golden_dir, tmp_path):
    """refused on the host, before anything asks for a GPU"""
    import recommend
    d = os.path.join(golden_dir, 'g4')
    base = ['-d', os.path.join(d, 'data'), '-m', os.path.join(d, 'model'), '-o', str(tmp_path / 'out.txt')]
    users = tmp_path / 'users'
    users.write_text('1\nnobody\n')
    with pytest.raises(KeyError, match='nobody'):
        recommend.main(base + ['-u', str(users)])
    for half in (['--new-uid', str(users)], ['--new-history', str(users)]):
        with pytest.raises(SystemExit):
            recommend.main(base + half)
    known = tmp_path / 'known'
    known.write_text('fresh\n2\n')
    with pytest.raises(KeyError, match="'2'"):                         # a "new" user the model already has
        recommend.main(base + ['--new-uid', str(known), '--new-history', os.path.join(d, 'data', 'f0tr.txt')])
    assert not (tmp_path / 'out.txt').exists()
    assert recommend.read_user_list(str(known), {'fresh': 0, '2': 1}) == ['fresh', '2']


def test_history_csr_sorts_and_removes_duplicates():
    import foldin
    ptr, cols = foldin.history_csr([[5, 1, 5, 3], [], [2]], 6)
    assert ptr.tolist() == [0, 3, 3, 4] and cols.tolist() == [1, 3, 5, 2] and ptr.dtype == np.int64 and cols.dtype == np.int32
    with pytest.raises(ValueError):
        foldin.history_csr([[6]], 6)
