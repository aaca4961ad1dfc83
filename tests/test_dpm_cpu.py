"""K22 (MLP, DPM) without a GPU: the oracle of tests/_dpm_oracle.py against the objective it is said to descend, and everything of
als.MLP, als.DPM and the C ABI that is checked before a device is touched."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import _cer_oracle as CO
import _dpm_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _small_net(seed=3):
    rng = np.random.Generator(np.random.PCG64(seed))
    params = O.copy_params(O.start((7, 5, 3, 2), seed))
    for layer in params:
        layer['bias'][...] = rng.standard_normal(layer['bias'].shape) / 4         # (the start has zero biases: their gradient is tested off it)
    return params, rng.standard_normal((6, 7)), rng.standard_normal((6, 2))


def test_gradients_are_those_of_the_objective():
    """central finite differences of the float64 objective, every parameter of a 7 -> 5 -> 3 -> 2 network"""
    params, X, Y = _small_net()
    obj, grads = O.gradients(params, X, Y)
    assert abs(obj - O.objective(params, X, Y)) <= 1e-14 * obj
    step = 1e-6
    for layer, (gW, gb) in zip(params, grads):
        for name, g in (('W', gW), ('bias', gb)):
            p = layer[name]
            assert g.shape == p.shape
            for at in np.ndindex(p.shape):
                keep = p[at]
                p[at] = keep + step
                up = O.objective(params, X, Y)
                p[at] = keep - step
                down = O.objective(params, X, Y)
                p[at] = keep
                assert abs((up - down) / (2 * step) - g[at]) <= 1e-7 * max(1.0, abs(g[at])), (name, at)


def test_rmsprop_step_by_hand():
    """w = 2, ms = 1, g = 3, lr = 1/4 (exact in fp32): q = 9, ms' = 1 + 8 * fl(1 - 0.9f), w' = 2 - 0.75 / sqrt(ms' + 1e-10f)"""
    one_minus_rho = float(np.float32(1) - np.float32(0.9))
    for dtype in (np.float64, np.float32):
        dt = np.dtype(dtype).type
        w, ms = np.full((2, 2), 2, dtype), np.ones((2, 2), dtype)
        O.rmsprop(w, ms, np.full((2, 2), 3, dtype), 0.25, dtype)
        ms1 = dt(1) + dt(8) * dt(one_minus_rho)
        assert (ms == ms1).all() and abs(float(ms1) - 1.8000001907) < 1e-9
        assert (w == dt(2) - dt(0.75) / np.sqrt(ms1 + dt(np.float32(1e-10)))).all()
        assert w.dtype == dtype and abs(float(w[0, 0]) - (2 - 0.75 / np.sqrt(1.8000001907))) < 1e-6
    # ... and a second step on the slot the first one left; a zero gradient moves the slot and not the weight
    w, ms = np.full(1, 2.0), np.full(1, 1.8)
    O.rmsprop(w, ms, np.zeros(1), 0.25)
    assert w[0] == 2.0 and abs(ms[0] - 1.8 * (1 - one_minus_rho)) < 1e-15
    # one batch of mlp_batch is gradients + rmsprop on every parameter, from the parameters before the batch
    params, X, Y = _small_net()
    before = O.copy_params(params)
    obj, grads = O.gradients(before, X, Y)
    assert O.mlp_batch(params, X, Y, 0.01) == obj
    for layer, old, (gW, gb) in zip(params, before, grads):
        for name, slot, g in (('W', 'msW', gW), ('bias', 'msb', gb)):
            w, ms = old[name].copy(), old[slot].copy()
            O.rmsprop(w, ms, g, 0.01)
            np.testing.assert_array_equal(layer[name], w)
            np.testing.assert_array_equal(layer[slot], ms)


def test_fit_falls_and_chunks():
    """an epoch in two calls split on a batch boundary is the epoch; repeated epochs lower the objective"""
    params, X, Y, order = O.net_inputs(9, (6,), 3, n=40)
    one, two = O.copy_params(params), O.copy_params(params)
    l1 = O.mlp_fit(one, X, Y, order, 8, 1e-2)
    l2 = O.mlp_fit(two, X, Y, order[:16], 8, 1e-2) + O.mlp_fit(two, X, Y, order[16:], 8, 1e-2)
    assert l1 == l2 and len(l1) == 5
    for a, b in zip(one, two):
        for name in O.PARTS:
            np.testing.assert_array_equal(a[name], b[name])
    first = O.objective(params, X, Y)
    for _ in range(30):
        O.mlp_fit(one, X, Y, order, 8, 1e-2)
    assert O.objective(one, X, Y) < 0.9 * first


class _Frozen:
    def __init__(self, E):
        self.E = E

    def out(self, F):
        return np.asarray(F, dtype=np.float64) @ self.E

    def fit(self, F, V):
        return 0.0


def test_dpm_iteration_with_a_frozen_linear_encoder_is_cers_item_step():
    rng = np.random.Generator(np.random.PCG64(9))
    n_u, n_i, k, d = 11, 13, 4, 6
    F, E = rng.random((n_i, d)), rng.standard_normal((d, k))
    U0, V0 = rng.random((n_u, k)), rng.random((n_i, k))
    user_likes = [rng.permutation(n_i - 2)[:m] for m in rng.integers(0, 5, n_u)]               # the last two items: no like
    user_likes[0] = np.asarray([0, 1, 2])
    item_likes = [np.asarray([u for u, l in enumerate(user_likes) if j in l], dtype=np.int64) for j in range(n_i)]
    hyper = dict(a=1.0, b=0.01, lu=0.1, lv=0.7)
    U1, V1, loss = O.dpm_iteration(U0, V0, F, user_likes, item_likes, _Frozen(E), **hyper)
    Fe = F @ E
    u_rated = [u for u, l in enumerate(user_likes) if len(l)]
    i_rated = [i for i, l in enumerate(item_likes) if len(l)]
    assert len(i_rated) < n_i
    Ue, _ = CO.half_step(U0, Fe, user_likes, i_rated, a=1.0, b=0.01, ridge_in_G=0.1, ridge=0.0)
    Ve, rl = CO.half_step_prior(V0, Ue, item_likes, u_rated, Fe, a=1.0, b=0.01, ridge_in_G=0.0, ridge=0.7, w_prior=0.7)
    np.testing.assert_array_equal(U1, Ue)
    np.testing.assert_array_equal(V1, Ve)                                                       # every row is solved: V0 does not matter
    assert loss == rl.sum() + 0.5 * 0.1 * (Ue ** 2).sum()
    # ... which is cer_iteration's item step when its user step saw the same item table
    _, Vc, _, _ = CO.cer_iteration(U0, Fe, E, F, user_likes, item_likes, a=1.0, b=0.01, lu=0.1, lv=0.7, le=1.0)
    np.testing.assert_array_equal(V1, Vc)
    Ut, Vt, losses = O.dpm_train(U0, V0, F, user_likes, item_likes, _Frozen(E), max_iter=2, **hyper)
    assert len(losses) == 2 and losses[0] == loss
    cold = [j for j in range(n_i) if j not in i_rated]
    np.testing.assert_array_equal(Vt[cold], Fe[cold])


def test_library_exports_the_mlp_entry_points():
    import tkr_hip
    header = open(os.path.join(ROOT, 'include', 'tkr.h')).read()
    declared = set(re.findall(r'^int(?:32_t|64_t)? (tkr_\w+)\(', header, flags=re.M))
    for name in ('tkr_mlp_forward', 'tkr_mlp_fit', 'tkr_mlp_workspace_bytes'):
        assert name in declared and name in tkr_hip.EXPORTS + tkr_hip.EXPORTS_I64
    for name, value in (('MAX_LAYERS', tkr_hip.MLP_MAX_LAYERS), ('MAX_BATCH', tkr_hip.MLP_MAX_BATCH), ('SLAB', tkr_hip.MLP_SLAB),
                        ('FORWARD_CHUNK', tkr_hip.MLP_FORWARD_CHUNK)):
        assert int(re.search(r'#define TKR_MLP_%s (\d+)' % name, header).group(1)) == value
    lib = C.CDLL(tkr_hip.LIB_PATH)
    for name in ('tkr_mlp_forward', 'tkr_mlp_fit', 'tkr_mlp_workspace_bytes'):
        getattr(lib, name)


def _abi():
    import tkr_hip
    lib = C.CDLL(tkr_hip.LIB_PATH)
    size, fwd, fit = lib.tkr_mlp_workspace_bytes, lib.tkr_mlp_forward, lib.tkr_mlp_fit
    size.restype, fwd.restype, fit.restype = C.c_int64, C.c_int, C.c_int
    size.argtypes = [C.c_void_p, C.c_int64, C.c_int32]
    fwd.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p]
    fit.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, C.c_float, C.c_void_p, C.c_void_p, C.c_int64,
                    C.c_void_p, C.c_void_p]
    return tkr_hip, size, fwd, fit


def _net(tkr_hip, widths=(7, 5, 3), pointer=0x1000):
    net = tkr_hip.MlpNet()
    net.n_layers = len(widths) - 1
    for l, w in enumerate(widths):
        net.width[l] = w
    for l in range(len(widths) - 1):
        for name in ('W', 'bias', 'msW', 'msb'):
            getattr(net, name)[l] = pointer
    return net


def test_workspace_bytes():
    tkr_hip, size, _, _ = _abi()
    assert C.sizeof(tkr_hip.MlpNet) == 4 * 8 + 4 * 5 * 8                                        # 7 ints padded to 8, 20 pointers
    net = _net(tkr_hip)
    ref = lambda n: C.byref(n)
    assert size(None, 4, 4) == -1 and size(ref(net), -1, 4) == -1 and size(ref(net), 4, -1) == -1 and size(ref(net), 4, 257) == -1
    for widths in ((7,), (7, 0, 3), (7, 5, -1), (1, 2, 3, 4, 5, 6, 7)):
        bad = _net(tkr_hip, widths) if 2 <= len(widths) <= 6 else _net(tkr_hip)
        if not 2 <= len(widths) <= 6:
            bad.n_layers = len(widths) - 1
        assert size(ref(bad), 4, 4) == -1, widths
    assert size(ref(_net(tkr_hip, pointer=0)), 4, 4) > 0                                        # the shape alone sizes it
    # forward: two buffers of min(m, CHUNK) x the widest hidden layer and the slab partials; fit: activations and deltas of every layer
    # and the partials of both directions
    up = lambda floats: (floats + 3) // 4 * 4
    slab, chunk = tkr_hip.MLP_SLAB, tkr_hip.MLP_FORWARD_CHUNK
    assert size(ref(net), 10, 0) == 4 * (2 * up(10 * 5) + up(max(10 * 5, 10 * 3)))
    assert size(ref(net), 10 ** 6, 0) == size(ref(net), chunk, 0) == 4 * (2 * up(chunk * 5) + up(chunk * 5))
    assert size(ref(net), 0, 9) == 4 * (2 * up(9 * 5) + 2 * up(9 * 3) + up(max(9 * 5, 9 * 3, 9 * 5)))
    wide = _net(tkr_hip, (2 * slab + 5, slab + 1, 2))
    assert size(ref(wide), 0, 64) == 4 * (2 * up(64 * (slab + 1)) + 2 * up(64 * 2) + up(max(3 * 64 * (slab + 1), 2 * 64 * 2, 1 * 64 * (slab + 1))))
    assert size(ref(wide), 3, 64) == size(ref(wide), 0, 64) and size(ref(wide), 3, 0) % 16 == 0
    ref_shape = _net(tkr_hip, (20000, 2000, 1000, 50))
    assert size(ref(ref_shape), 10380, 64) == 4 * (2 * chunk * 2000 + 40 * chunk * 2000)       # the forward over all items is the larger


def test_every_refusal_of_the_two_entry_points_needs_no_device():
    """TKR_E_INVAL (-1) / TKR_E_UNSUPPORTED (-2) before any device access: the pointers below are never followed"""
    tkr_hip, size, fwd, fit = _abi()
    net = _net(tkr_hip)
    p, ws_bytes = 0x2000, 1 << 20
    good_fwd = [C.addressof(net), p, 9, p, 4, p, p, ws_bytes, p, None]
    good_fit = [C.addressof(net), p, 9, p, p, 4, 2, 0.01, p, p, ws_bytes, p, None]

    def nets():
        for change in ('n_layers=0', 'n_layers=6', 'width0', 'widthL', 'W', 'bias'):
            bad = _net(tkr_hip)
            if change.startswith('n_layers'):
                bad.n_layers = int(change[-1])
            elif change == 'width0':
                bad.width[0] = 0
            elif change == 'widthL':
                bad.width[2] = -3
            else:
                getattr(bad, change)[1] = 0 if change == 'W' else 0x1002
            yield change, bad, -1
        huge = _net(tkr_hip)
        huge.width[1] = (1 << 21) + 1
        yield 'width above 2^21', huge, -2

    for what, bad, rc in nets():
        assert fwd(*([C.addressof(bad)] + good_fwd[1:])) == rc, what
        assert fit(*([C.addressof(bad)] + good_fit[1:])) == rc, what
    no_slots = _net(tkr_hip)
    no_slots.msW[0] = 0
    assert fit(*([C.addressof(no_slots)] + good_fit[1:])) == -1
    odd_slot = _net(tkr_hip)
    odd_slot.msb[1] = 0x1001
    assert fit(*([C.addressof(odd_slot)] + good_fit[1:])) == -1
    # forward: net, X, n, rows, m, out, workspace, workspace_bytes, status
    for at, bad in ((0, None), (1, None), (1, p + 2), (2, 0), (3, p + 1), (4, -1), (5, None), (5, p + 1), (6, None), (6, p + 8), (7, 8), (7, -1),
                    (8, None), (8, p + 4)):
        args = list(good_fwd)
        args[at] = bad
        assert fwd(*args) == -1, at
    args = list(good_fwd)
    args[3], args[4] = None, 10                                                                 # rows NULL: the rows 0 .. m - 1 of n = 9
    assert fwd(*args) == -1
    # fit: net, X, n, Y, order, m, batch, lr, batch_loss, workspace, workspace_bytes, status
    for at, bad, rc in ((0, None, -1), (1, None, -1), (1, p + 1, -1), (2, 0, -1), (3, None, -1), (3, p + 2, -1), (4, None, -1), (4, p + 2, -1),
                        (5, -1, -1), (6, 0, -1), (6, -4, -1), (6, 257, -2), (7, -0.5, -1), (7, float('nan'), -1), (7, float('inf'), -1),
                        (8, None, -1), (8, p + 4, -1), (9, None, -1), (9, p + 8, -1), (10, 8, -1), (10, -1, -1), (11, None, -1), (11, p + 4, -1)):
        args = list(good_fit)
        args[at] = bad
        assert fit(*args) == rc, at


def test_mlp_argument_checks_and_state():
    import als
    for bad in (dict(k=129), dict(k=0), dict(d=0), dict(d=2.5), dict(hidden_layers=(3, 0)), dict(hidden_layers=(3, -1)), dict(hidden_layers=(2.5,)),
                dict(hidden_layers=(2, 2, 2, 2, 2)), dict(lr=-1.0), dict(lr=float('nan')), dict(seed=-1)):
        with pytest.raises(ValueError):
            als.MLP(**{**dict(k=4, d=3), **bad})
    m = als.MLP(50, 20, seed=1, hidden_layers=[])
    assert (m.k, m.d, m.lr, m.lbd, m.hidden_layers, m.widths, m.epochs_done) == (50, 20, 1e-4, 1e-4, (), (20, 50), 0)
    assert als.MLP(4, 3, hidden_layers=(9, 8, 7, 6), seed=1).widths == (3, 9, 8, 7, 6, 4)
    assert als.MLP.__init__.__defaults__[2] == (2000, 1000)
    for batch_size in (0, 257, 2.0):
        with pytest.raises(ValueError, match='batch_size'):
            m.fit(np.zeros((3, 20), np.float32), np.zeros((3, 50), np.float32), batch_size=batch_size)
    with pytest.raises(ValueError, match='X'):
        m.out(np.zeros((3, 21), np.float32))
    with pytest.raises(ValueError, match='Y'):
        m.fit(np.zeros((3, 20), np.float32), np.zeros((3, 49), np.float32))
    m.pretrain(None, None)
    m.pertrain(None, None)
    # the start: the oracle's, from the seed alone; a seed that is not given is drawn, and kept
    m = als.MLP(5, 7, hidden_layers=(6, 4), seed=11)
    state = m.state()
    for l, layer in enumerate(O.start((7, 6, 4, 5), 11)):
        for name in O.PARTS:
            assert state['%s%d' % (name, l)].dtype == np.float32
            np.testing.assert_array_equal(state['%s%d' % (name, l)], layer[name])
        limit = np.sqrt(6.0 / sum(layer['W'].shape))
        assert np.abs(layer['W']).max() <= limit and np.abs(layer['W']).max() > 0.8 * limit and not layer['bias'].any() and (layer['msW'] == 1).all()
    assert als.MLP(5, 7, seed=None).seed != als.MLP(5, 7, seed=None).seed
    # state() -> load_state() is the identity, on an encoder of another shape and history too
    m.epochs_done = 3
    state = m.state()
    other = als.MLP(5, 7, lr=0.5, hidden_layers=(2,), seed=99)
    other.load_state(state)
    again = other.state()
    assert sorted(again) == sorted(state) and (other.seed, other.epochs_done, other.lr, other.hidden_layers) == (11, 3, 1e-4, (6, 4))
    for name in state:
        assert again[name].dtype == state[name].dtype
        np.testing.assert_array_equal(again[name], state[name])
    with pytest.raises(ValueError, match='widths'):
        als.MLP(5, 8, seed=1).load_state(state)
    broken = dict(state, W1=state['W1'].astype(np.float64))
    with pytest.raises(ValueError, match='W1'):
        other.load_state(broken)


def test_epoch_orders_come_from_seed_and_epoch():
    import als
    for seed, e, n in ((0, 0, 10), (5, 3, 150), (2 ** 40, 7, 33)):
        order = als.epoch_order(seed, e, n)
        assert order.dtype == np.int32 and sorted(order.tolist()) == list(range(n))
        np.testing.assert_array_equal(order, np.random.Generator(np.random.PCG64(np.random.SeedSequence([seed, e]))).permutation(n))
        np.testing.assert_array_equal(order, O.epoch_order(seed, e, n))
    assert (als.epoch_order(5, 0, 150) != als.epoch_order(5, 1, 150)).any() and (als.epoch_order(5, 0, 150) != als.epoch_order(6, 0, 150)).any()


def _g2_model(golden_dir, **over):
    import als
    d = os.path.join(golden_dir, 'g2')
    hyper = dict(k=O.E2E['k'], d=O.E2E['d'], lu=O.E2E['lu'], lv=O.E2E['lv'], a=O.E2E['a'], b=O.E2E['b'])
    hyper.update(over)
    m = als.DPM(**hyper)
    m.load_training_data(os.path.join(d, 'uid'), os.path.join(d, 'vid'), os.path.join(d, 'f0tr.txt'), seed=O.E2E['seed'])
    return m


def test_dpm_argument_checks_need_no_gpu(golden_dir, tmp_path):
    import als
    for bad in (dict(d=0), dict(d=2.5), dict(lv=0.0), dict(lv=-1.0), dict(k=129), dict(a=0.01, b=0.01), dict(b=0.0), dict(lu=-1.0)):
        with pytest.raises(ValueError):
            als.DPM(**{**dict(k=4, d=3), **bad})
    m = als.DPM(k=4, d=3)
    assert (m.k, m.d, m.lu, m.lv, m.le, m.a, m.b) == (4, 3, 0.01, 10.0, 10e3, 1.0, 0.01) and m.encoder is None and isinstance(m, als.WMF)
    with pytest.raises(ValueError, match='load_training_data'):
        m.train(als.MLP)
    with pytest.raises(ValueError, match='train'):
        m.embed_items(np.zeros((2, 3), np.float32))
    m = _g2_model(golden_dir)
    with pytest.raises(ValueError, match='load_content_data'):
        m.train(als.MLP)
    m.feat = CO.e2e_features(m.n_items)
    for batch_size in (0, 257):
        with pytest.raises(ValueError, match='batch_size'):
            m.train(als.MLP, batch_size=batch_size)
    with pytest.raises(ValueError, match='encoder'):
        m.train(als.MLP(O.E2E['k'], O.E2E['d'] + 1, hidden_layers=(3,), seed=1))
    with pytest.raises(ValueError, match='encoder'):
        m.train(object())
    # export_model / import_model: mlp.npz holds the encoder's state exactly; an encoder of another shape is refused
    enc = als.MLP(O.E2E['k'], O.E2E['d'], lr=O.E2E['lr'], hidden_layers=O.E2E['hidden'], seed=O.E2E['mlp_seed'])
    enc.epochs_done = 2
    m.encoder = enc
    out = str(tmp_path / 'model')
    m.export_embeddings(out)
    assert sorted(os.listdir(out)) == ['final-U.dat', 'final-V.dat', 'mlp.npz']
    fresh = _g2_model(golden_dir)
    fresh.import_embeddings(out)
    state, again = enc.state(), fresh.encoder.state()
    for name in state:
        np.testing.assert_array_equal(again[name], state[name])
    assert (fresh.encoder.epochs_done, fresh.encoder.seed, fresh.encoder.lr, fresh.encoder.hidden_layers) == (2, O.E2E['mlp_seed'], O.E2E['lr'], O.E2E['hidden'])
    wrong = _g2_model(golden_dir, k=O.E2E['k'] - 1)
    with pytest.raises(ValueError, match='widths'):
        wrong.import_model(out)
    # the memory arithmetic
    f, t, e = als.dpm_train_bytes(7, 5, 3, 2, (2, 4, 3), 8)
    tkr_hip, size, _, _ = _abi()
    assert (f, t) == (4 * 5 * 2, 4 * 3 * (7 + 10)) and e == 16 * (2 * 4 + 4 + 4 * 3 + 3) + size(C.byref(_net(tkr_hip, (2, 4, 3))), 5, 8)


def test_single_dpm_still_raises():
    import single
    for name in ('DPM', 'ENCODER', 'MLP'):
        with pytest.raises(NotImplementedError):
            getattr(single, name)(4, 3)


def test_train_als_takes_the_encoder_options_with_dpm_only(tmp_path):
    import train_als
    for argv in (['--model', 'dpm'], ['--model', 'dpm', '--content', 'x.pkl'], ['--model', 'wmf', '--hidden', '5'], ['--model', 'cer', '--content', 'x.pkl', '--dim', '3', '--batch', '8'],
                 ['--model', 'wmf', '--mlp-lr', '0.1'], ['--model', 'dpm', '--content', 'x.pkl', '--dim', '3', '--batch', '257'],
                 ['--model', 'dpm', '--content', 'x.pkl', '--dim', '3', '--hidden', '1', '2', '3', '4', '5']):
        with pytest.raises(SystemExit):
            train_als.main(argv + ['-d', str(tmp_path)])


def test_float64_premises_of_the_gpu_end_to_end_test(golden_dir):
    """g2 with E2E: 30 items, 4 without a training like; over the 4 iterations of the float64 run the encoder moves by far more than
    the tolerance of the GPU test and every loss is finite (the printed loss is no objective that one step descends: the users are solved
    against the encoder's output, the items pulled towards it, then the encoder moves: dpm.py:31-60)"""
    m = _g2_model(golden_dir)
    assert (m.n_items, len(m.i_rated)) == (30, 26)
    F = CO.e2e_features(m.n_items)
    up, uc, ip, ic = m._csr
    likes = (CO.csr_rows(up, uc), CO.csr_rows(ip, ic))
    widths = (O.E2E['d'],) + O.E2E['hidden'] + (O.E2E['k'],)
    params = O.start(widths, O.E2E['mlp_seed'])
    orders = [O.epoch_order(O.E2E['mlp_seed'], e, m.n_items) for e in range(O.E2E['iters'])]
    enc = O.Net(params, O.E2E['lr'], O.E2E['batch'], orders)
    U, V, losses = O.dpm_train(m.fue, m.fie, F, *likes, enc, a=m.a, b=m.b, lu=m.lu, lv=m.lv, max_iter=O.E2E['iters'])
    assert len(losses) == 4 and np.isfinite(losses).all() and min(losses) > 0 and len(set(losses)) == 4, losses
    assert enc.epochs_done == 4 and np.abs(enc.params[0]['W'] - params[0]['W']).max() > 1e-3
    cold = [j for j in range(m.n_items) if j not in m.i_rated]
    np.testing.assert_array_equal(V[cold], enc.out(F)[cold])
