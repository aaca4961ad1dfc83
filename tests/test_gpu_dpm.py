"""K22 on the GPU (csrc/mlp.hip tkr_mlp_forward / tkr_mlp_fit, top-k-rec_amd/als.py MLP and DPM) against tests/_dpm_oracle.py.

Exact inputs are compared bit for bit.  Everything else by K20's yardstick (tests/test_gpu_als.py): with x64 the float64 oracle on the
same fp32 inputs and x32 the float32 one, e32 = max|x32 - x64| / max|x64| per quantity, and the kernels have to stay within
F * max(e32, 2^-23).  F is set by K20's rule, the next power of two above twice the worst ratio measured on an MI355X (7.46, the one
bias of a single linear layer at d = 1,029, k = 1, batch 64, where e32 lies 1.1 x above the floor; out 3.17, batch_loss 2.14, W 1.96,
msW 2.58, msb 4.75, als.DPM end to end 1.69 at worst: DESIGN.md section 4 K22); F <= 16 is a condition of the design, not a knob."""
import functools
import os
import pickle
import shutil

import numpy as np
import pytest
import torch

import _cer_oracle as CO
import _dpm_oracle as O

pytestmark = pytest.mark.gpu

F = 16.0
FLOOR = 2.0 ** -23
SLAB = 512


def _dev(a):
    return torch.from_numpy(np.array(a, order='C')).cuda()


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.int32 if a.dtype == np.float32 else np.int64)


def _ratio(got, x64, x32):
    scale = np.abs(x64).max()
    err, e32 = np.abs(got - x64).max() / scale, np.abs(x32 - x64).max() / scale
    return err / max(e32, FLOOR), err, e32


def _net(params):
    """fp32 host parameters -> (MlpNet, the device tensors behind it)"""
    import tkr_hip
    layers = [{name: _dev(np.asarray(layer[name], dtype=np.float32)) for name in O.PARTS} for layer in params]
    return tkr_hip.mlp_net(layers), layers


def _down(layers):
    return [{name: t.cpu().numpy() for name, t in layer.items()} for layer in layers]


def _same_bits(got, exp, what=''):
    for l, (a, b) in enumerate(zip(got, exp)):
        for name in O.PARTS:
            np.testing.assert_array_equal(_bits(a[name]), _bits(np.asarray(b[name], dtype=np.float32)), err_msg='%s %s of layer %d' % (what, name, l))


def _eighths(rng, shape, most=8):
    return (rng.integers(-most, most + 1, shape) / 8).astype(np.float32)


def _layer(W, bias):
    return dict(W=W, bias=bias, msW=np.ones_like(W), msb=np.ones_like(bias))


# ---- 1. forward, exact ---------------------------------------------------------------------------------------------------------------------
M_CASES = (1, 63, 64, 65, 200)


@pytest.mark.parametrize('d,out', [(1, 1), (31, 33), (64, 64), (65, 1), (2 * SLAB + 5, 33)])
def test_forward_is_exact_on_exact_inputs(d, out):
    """one linear layer, everything a multiple of 1/8: every product and every partial sum is exact in fp32, in any order.  Any slip of
    a tile edge, a slab's end, a gathered row or the bias moves an element"""
    import tkr_hip
    assert tkr_hip.MLP_SLAB == SLAB
    rng = np.random.Generator(np.random.PCG64([50, d, out]))
    n = 200
    X, W, b = _eighths(rng, (n, d)), _eighths(rng, (d, out)), _eighths(rng, out, 24)
    net, _ = _net([_layer(W, b)])
    exp = X @ W + b
    assert exp.dtype == np.float32 and (exp.astype(np.float64) == X.astype(np.float64) @ W.astype(np.float64) + b).all()
    Xd = _dev(X)
    for m in M_CASES:
        got = tkr_hip.mlp_forward(net, Xd[:m]).cpu().numpy()                    # rows NULL: the rows 0 .. m - 1
        np.testing.assert_array_equal(_bits(got), _bits(exp[:m]), err_msg='m = %d' % m)
        rows = rng.integers(0, n, m).astype(np.int32)                           # a list with repeats
        rows[0] = n - 1
        got = tkr_hip.mlp_forward(net, Xd, _dev(rows)).cpu().numpy()
        np.testing.assert_array_equal(_bits(got), _bits(exp[rows]), err_msg='gathered, m = %d' % m)


def test_forward_through_a_hidden_layer_is_exact_on_exact_inputs():
    """70 -> 65 -> 33: the hidden layer has W = 0 and biases 0 or 64, so its sigmoid gives exactly 1/2 (1 / (1 + 1)) or exactly 1
    (expf(-64) vanishes beside 1); the linear last layer behind it is exact as above"""
    import tkr_hip
    rng = np.random.Generator(np.random.PCG64(51))
    n, d, hid, k = 200, 70, 65, 33
    X = _eighths(rng, (n, d))
    b0 = (64 * rng.integers(0, 2, hid)).astype(np.float32)
    W1, b1 = _eighths(rng, (hid, k)), _eighths(rng, k, 24)
    net, _ = _net([_layer(np.zeros((d, hid), np.float32), b0), _layer(W1, b1)])
    h = np.where(b0 > 0, np.float32(1), np.float32(0.5)).astype(np.float32)
    assert 0 < (b0 > 0).sum() < hid
    exp = np.broadcast_to(h @ W1 + b1, (n, k)).astype(np.float32)
    Xd = _dev(X)
    for m in M_CASES:
        np.testing.assert_array_equal(_bits(tkr_hip.mlp_forward(net, Xd[:m]).cpu().numpy()), _bits(exp[:m]), err_msg='m = %d' % m)


# ---- 2. gradient + update, exact -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('d,k', [(1, 1), (33, 5), (70, 50), (257, 128)])
@pytest.mark.parametrize('batch', [1, 2, 63, 64, 65, 256])
def test_one_batch_is_exact_on_exact_inputs(batch, d, k):
    """a one-layer linear net on multiples of 1/4: F, delta and the gradient (at most 256 terms below 2^9 in 1/64ths) are exact in any
    order, so W, bias and both slots have to be the float32 NumPy sequence q = g g; ms' = ms + (q - ms) fl(1 - rho); w' = w - (lr g) /
    sqrt(ms' + eps) bit for bit -- from unit slots, and in a second batch from the slots a first one left (lr = 0 there: the weights
    stay exact, the slots move)"""
    import tkr_hip
    rng = np.random.Generator(np.random.PCG64([52, batch, d, k]))
    n = 300
    X = (rng.integers(-4, 5, (n, d)) / 4).astype(np.float32)
    Y = (rng.integers(-8, 9, (n, k)) / 4).astype(np.float32)
    W, b = (rng.integers(-2, 3, (d, k)) / 4).astype(np.float32), (rng.integers(-4, 5, k) / 4).astype(np.float32)
    first, second = rng.integers(0, n, batch).astype(np.int32), rng.integers(0, n, batch).astype(np.int32)
    Xd, Yd = _dev(X), _dev(Y)
    lr = 0.01

    def loss64(rows):
        f = X[rows] @ W + b
        return 0.5 * ((Y[rows].astype(np.float64) - f.astype(np.float64)) ** 2).sum()

    # from unit slots
    exp = O.copy_params([_layer(W, b)], np.float32)
    O.mlp_batch(exp, X[first], Y[first], lr, np.float32)
    net, layers = _net([_layer(W, b)])
    loss = tkr_hip.mlp_fit(net, Xd, Yd, _dev(first), batch, lr).cpu().numpy()
    _same_bits(_down(layers), exp, 'first batch:')
    assert (exp[0]['W'] != W).any() and (exp[0]['msW'] != 1).any()
    np.testing.assert_array_equal(_bits(loss), _bits(np.asarray([loss64(first)])))
    # a batch at lr = 0 moves the slots alone; the next one starts from them
    exp = O.copy_params([_layer(W, b)], np.float32)
    O.mlp_batch(exp, X[first], Y[first], 0.0, np.float32)
    np.testing.assert_array_equal(exp[0]['W'], W)
    net, layers = _net([_layer(W, b)])
    tkr_hip.mlp_fit(net, Xd, Yd, _dev(first), batch, 0.0)
    _same_bits(_down(layers), exp, 'lr = 0:')
    O.mlp_batch(exp, X[second], Y[second], lr, np.float32)
    loss = tkr_hip.mlp_fit(net, Xd, Yd, _dev(second), batch, lr).cpu().numpy()
    _same_bits(_down(layers), exp, 'second batch:')
    np.testing.assert_array_equal(_bits(loss), _bits(np.asarray([loss64(second)])))


# ---- 3. the whole network against the oracle ------------------------------------------------------------------------------------------------
N_ROWS, LR = 150, 1e-2


def _order(order, batch):
    """five batches, the last one short: the permutation of the rows taken twice"""
    return np.concatenate([order, order])[:4 * batch + 22].astype(np.int32)


@functools.lru_cache(maxsize=None)
def _oracle_case(d, hidden, k, batch):
    params, X, Y, order = O.net_inputs(d, hidden, k, n=N_ROWS)
    order = _order(order, batch)
    out = []
    for dtype in (np.float64, np.float32):
        p = O.copy_params(params, dtype)
        losses = np.asarray(O.mlp_fit(p, X, Y, order, batch, LR, dtype), dtype=np.float64)
        out.append((p, losses, np.asarray(O.mlp_forward(p, X, dtype), dtype=np.float64)))
    return out


@pytest.mark.parametrize('batch', [64, 37])
@pytest.mark.parametrize('k', [1, 5, 50, 128])
@pytest.mark.parametrize('hidden', [(33,), (65, 31), ()])
@pytest.mark.parametrize('d', [70, 2 * SLAB + 5])
def test_fit_and_forward_against_the_oracle(d, hidden, k, batch):
    import tkr_hip
    params, X, Y, order = O.net_inputs(d, hidden, k, n=N_ROWS)
    order = _order(order, batch)
    (p64, l64, f64), (p32, l32, f32) = _oracle_case(d, hidden, k, batch)
    assert len(l64) == 5 and len(order) % batch == 22
    net, layers = _net(params)
    Xd = _dev(X)
    loss = tkr_hip.mlp_fit(net, Xd, _dev(Y), _dev(order), batch, LR).cpu().numpy()
    got = _down(layers)
    out = tkr_hip.mlp_forward(net, Xd).cpu().numpy()
    assert np.isfinite(loss).all() and np.isfinite(out).all()
    assert np.abs(p64[0]['W'] - params[0]['W']).max() > 1e-3                   # the steps are visible
    quantities = [('out', out, f64, f32), ('batch_loss', loss, l64, l32)]
    for l in range(len(params)):
        quantities += [('%s%d' % (name, l), got[l][name], p64[l][name], p32[l][name]) for name in O.PARTS]
    for name, g, x64, x32 in quantities:
        ratio, err, e32 = _ratio(np.asarray(g, dtype=np.float64), np.asarray(x64, dtype=np.float64), np.asarray(x32, dtype=np.float64))
        print('K22 net d=%d hidden=%s k=%d batch=%d %s: err %.3g e32 %.3g ratio %.3g' % (d, hidden, k, batch, name, err, e32, ratio))
        assert ratio <= F, (name, err, e32)


# ---- 4. repeatable, chunk-independent -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('d,hidden,k,batch', [(2 * SLAB + 5, (65, 31), 50, 37), (70, (), 128, 64)])
def test_fit_is_repeatable_and_splits_on_a_batch_boundary(d, hidden, k, batch):
    import tkr_hip
    params, X, Y, order = O.net_inputs(d, hidden, k, n=N_ROWS)
    order = _order(order, batch)
    Xd, Yd = _dev(X), _dev(Y)
    runs = []
    for pieces in ((order,), (order,), (order[:2 * batch], order[2 * batch:])):
        net, layers = _net(params)
        losses = [tkr_hip.mlp_fit(net, Xd, Yd, _dev(piece), batch, LR).cpu().numpy() for piece in pieces]
        runs.append((_down(layers), np.concatenate(losses), tkr_hip.mlp_forward(net, Xd).cpu().numpy()))
    for got, loss, out in runs[1:]:
        _same_bits(got, runs[0][0])
        np.testing.assert_array_equal(_bits(loss), _bits(runs[0][1]))
        np.testing.assert_array_equal(_bits(out), _bits(runs[0][2]))
    # a row's output does not depend on how many rows are asked for, or where it stands among them
    rows = np.asarray([149, 0, 77, 77, 3], dtype=np.int32)
    np.testing.assert_array_equal(_bits(tkr_hip.mlp_forward(net, Xd, _dev(rows)).cpu().numpy()), _bits(runs[0][2][rows]))


# ---- 5. refusals ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('bad', [N_ROWS, -1])
def test_an_index_outside_the_table_refuses_the_whole_call(bad):
    import tkr_hip
    batch = 37
    params, X, Y, order = O.net_inputs(70, (33,), 5, n=N_ROWS)
    order = _order(order, batch)
    net, layers = _net(params)
    Xd, Yd = _dev(X), _dev(Y)
    for position in (0, 40, len(order) - 1):
        broken = order.copy()
        broken[position] = bad
        broken[-1] = bad                                                        # (the smallest position is the one reported)
        loss, status = tkr_hip.mlp_fit(net, Xd, Yd, _dev(broken), batch, LR, check=False)
        assert int(status.item()) == 4 * position + 1
        _same_bits(_down(layers), params, 'refused fit:')
        assert not loss.cpu().numpy().any()                                     # (allocated as zeros: never written)
        with pytest.raises(tkr_hip.MlpRefused) as info:
            tkr_hip.mlp_fit(net, Xd, Yd, _dev(broken), batch, LR)
        assert info.value.position == position
        rows = broken[:position + 1]
        out = torch.full((len(rows), 5), 7.0, dtype=torch.float32, device='cuda')
        _, status = tkr_hip.mlp_forward(net, Xd, _dev(rows), out=out, check=False)
        assert int(status.item()) == 4 * position + 1
        assert (out.cpu().numpy() == 7.0).all()
    _same_bits(_down(layers), params, 'after every refusal:')
    # m = 0: status -1 and nothing else
    empty = torch.zeros(0, dtype=torch.int32, device='cuda')
    loss, status = tkr_hip.mlp_fit(net, Xd, Yd, empty, batch, LR, check=False)
    assert int(status.item()) == -1 and loss.numel() == 0
    out, status = tkr_hip.mlp_forward(net, Xd, empty, check=False)
    assert int(status.item()) == -1 and tuple(out.shape) == (0, 5)
    _same_bits(_down(layers), params, 'm = 0:')
    # ... and the net still works
    good, status = tkr_hip.mlp_fit(net, Xd, Yd, _dev(order), batch, LR, check=False)
    assert int(status.item()) == -1 and good.cpu().numpy().all()


# ---- 6. als.MLP -----------------------------------------------------------------------------------------------------------------------------
def test_mlp_draws_its_orders_from_seed_and_epoch():
    import als
    import tkr_hip
    d, hidden, k, n = 70, (33,), 5, N_ROWS
    _, X, Y, _ = O.net_inputs(d, hidden, k, n=n)
    a = als.MLP(k, d, lr=LR, hidden_layers=hidden, seed=17)
    b = als.MLP(k, d, lr=LR, hidden_layers=hidden, seed=17)
    la = [a.fit(X, Y, batch_size=37), a.fit(X, Y, batch_size=37)]
    lb = [b.fit(X, Y, batch_size=37, order=als.epoch_order(17, e, n)) for e in (0, 1)]
    assert la == lb and a.epochs_done == b.epochs_done == 2 and la[0] != la[1]
    sa, sb = a.state(), b.state()
    for name in sa:
        np.testing.assert_array_equal(sa[name], sb[name])
    assert (sa['W0'] != O.start((d,) + hidden + (k,), 17)[0]['W']).any()
    # the sum fit returns is the sum of the kernel's batch objectives; against the oracle on the same orders
    p64 = O.copy_params(O.start((d,) + hidden + (k,), 17))
    l64 = [float(np.sum(O.mlp_fit(p64, X, Y, O.epoch_order(17, e, n), 37, LR))) for e in (0, 1)]
    np.testing.assert_allclose(la, l64, rtol=1e-5)
    # out() after fit() is tkr_mlp_forward on the downloaded state, for a host array and for a device tensor
    layers = [{name: sa['%s%d' % (name, l)] for name in O.PARTS} for l in range(2)]
    net, _ = _net(layers)
    exp = tkr_hip.mlp_forward(net, _dev(X)).cpu().numpy()
    got = a.out(X)
    assert isinstance(got, np.ndarray) and got.dtype == np.float32 and got.shape == (n, k)
    np.testing.assert_array_equal(_bits(got), _bits(exp))
    on_device = a.out(_dev(X[:7]))
    assert isinstance(on_device, torch.Tensor) and on_device.is_cuda
    np.testing.assert_array_equal(_bits(on_device.cpu().numpy()), _bits(exp[:7]))
    with pytest.raises(tkr_hip.MlpRefused):
        a.fit(X, Y, batch_size=37, order=[0, 1, n])
    with pytest.raises(FloatingPointError):
        bad = Y.copy()
        bad[3, 2] = np.inf
        a.fit(X, bad, batch_size=37)


# ---- 7. als.DPM end to end ------------------------------------------------------------------------------------------------------------------
def _g2(golden_dir):
    return os.path.join(golden_dir, 'g2')


def _model(golden_dir):
    import als
    d = _g2(golden_dir)
    m = als.DPM(k=O.E2E['k'], d=O.E2E['d'], lu=O.E2E['lu'], lv=O.E2E['lv'], a=O.E2E['a'], b=O.E2E['b'])
    m.load_training_data(os.path.join(d, 'uid'), os.path.join(d, 'vid'), os.path.join(d, 'f0tr.txt'), seed=O.E2E['seed'])
    m.feat = CO.e2e_features(m.n_items)                                         # what load_content_data leaves (the driver below goes through a pickle)
    return m


def _encoder():
    import als
    return als.MLP(O.E2E['k'], O.E2E['d'], lr=O.E2E['lr'], hidden_layers=O.E2E['hidden'], seed=O.E2E['mlp_seed'])


def _state_layers(state):
    n_layers = len(state['widths']) - 1
    return [{name: state['%s%d' % (name, l)] for name in O.PARTS} for l in range(n_layers)]


def _oracle_run(m, U0, V0, params, first_epoch, iters):
    """-> per dtype (U, V, losses, the encoder's parameters afterwards)"""
    up, uc, ip, ic = m._csr
    likes = (CO.csr_rows(up, uc), CO.csr_rows(ip, ic))
    orders = [O.epoch_order(O.E2E['mlp_seed'], first_epoch + e, m.n_items) for e in range(iters)]
    out = []
    for dtype in (np.float64, np.float32):
        enc = O.Net(params, O.E2E['lr'], O.E2E['batch'], orders, dtype)
        U, V, losses = O.dpm_train(U0, V0, m.feat, *likes, enc, a=m.a, b=m.b, lu=m.lu, lv=m.lv, max_iter=iters, dtype=dtype)
        out.append((U, V, losses, enc.params))
    return out


def _compare_run(tag, m, t64, t32):
    (U64, V64, l64, p64), (U32, V32, l32, p32) = t64, t32
    assert len(m.losses) == len(l64)
    got = _state_layers(m.encoder.state())
    quantities = [('fue', m.fue, U64, U32), ('fie', m.fie, V64, V32)]
    quantities += [('loss %d' % i, np.asarray([m.losses[i]]), np.asarray([l64[i]]), np.asarray([l32[i]])) for i in range(len(l64))]
    for l in range(len(got)):
        quantities += [('%s%d' % (name, l), got[l][name], p64[l][name], p32[l][name]) for name in O.PARTS]
    for name, g, x64, x32 in quantities:
        ratio, err, e32 = _ratio(np.asarray(g, dtype=np.float64), np.asarray(x64, dtype=np.float64), np.asarray(x32, dtype=np.float64))
        print('K22 DPM %s %s: err %.3g e32 %.3g ratio %.3g' % (tag, name, err, e32, ratio))
        assert ratio <= F, (name, err, e32)


@functools.lru_cache(maxsize=None)
def _trained(golden_dir, iters):
    m = _model(golden_dir)
    U0, V0 = m.fue.copy(), m.fie.copy()
    m.train(_encoder(), max_iter=iters, batch_size=O.E2E['batch'], verbose=False)
    params = O.start((O.E2E['d'],) + O.E2E['hidden'] + (O.E2E['k'],), O.E2E['mlp_seed'])
    return m, _oracle_run(m, U0, V0, params, 0, iters)


def test_dpm_trains_as_the_oracle(golden_dir):
    m, (t64, t32) = _trained(golden_dir, O.E2E['iters'])
    assert len(m.losses) == O.E2E['iters'] == 4 and m.encoder.epochs_done == 4
    assert m.fue.dtype == m.fie.dtype == np.float32 and m.fie.shape == (30, O.E2E['k'])
    _compare_run('after 4 iterations', m, t64, t32)
    # an item without a training like ends with its row of encoder.out(feat), bit for bit; embed_items is the same call
    cold = [j for j in range(m.n_items) if j not in m.i_rated]
    assert len(cold) == 4
    Fe = m.encoder.out(m.feat)
    np.testing.assert_array_equal(_bits(m.fie[cold]), _bits(Fe[cold]))
    warm = [j for j in range(m.n_items) if j in m.i_rated]
    assert (m.fie[warm] != Fe[warm]).any()
    got = m.embed_items(m.feat[:3])
    assert got.dtype == np.float32 and got.shape == (3, m.k)
    np.testing.assert_array_equal(_bits(got), _bits(Fe[:3]))


def test_dpm_model_directory(golden_dir, tmp_path):
    import als
    import evaluate as E
    import train_als
    from oracle import ref_np as R
    m, _ = _trained(golden_dir, 2)
    assert m.encoder.epochs_done == 2
    out = str(tmp_path / 'dpm')
    m.export_embeddings(out)
    assert sorted(os.listdir(out)) == ['final-U.dat', 'final-V.dat', 'mlp.npz']
    saved = m.encoder.state()
    fresh = _model(golden_dir)
    fresh.import_embeddings(out)
    loaded = fresh.encoder.state()
    for name in saved:
        np.testing.assert_array_equal(loaded[name], saved[name])               # the encoder's round trip is exact
    assert np.abs(fresh.fue - m.fue).max() <= 5.1e-7 * max(1.0, np.abs(m.fue).max())      # '%f' keeps 6 decimals
    U1, V1 = fresh.fue.copy(), fresh.fie.copy()
    fresh = _model(golden_dir)
    fresh.train(als.MLP, max_iter=2, model_path=out, batch_size=O.E2E['batch'], verbose=False)    # a fresh object, the class as in train.py:36
    assert fresh.encoder.epochs_done == 4 and fresh.encoder.seed == O.E2E['mlp_seed'] and fresh.encoder.hidden_layers == O.E2E['hidden']
    t64, t32 = _oracle_run(fresh, U1, V1, _state_layers(saved), 2, 2)           # the orders of epochs 2 and 3, not 0 and 1
    _compare_run('two more iterations from the model directory', fresh, t64, t32)
    again = _oracle_run(fresh, U1, V1, _state_layers(saved), 0, 2)[0]
    assert np.abs(again[3][0]['W'] - t64[3][0]['W']).max() > 1e-4               # ... which the comparison can tell apart

    # evaluate.py -sl im om: g2's own om files are empty, so the four items without a training like become the out-of-matrix scenario
    data = str(tmp_path / 'data')
    shutil.copytree(_g2(golden_dir), data)
    vids = [line.strip() for line in open(os.path.join(data, 'vid'))]
    uids = [line.strip() for line in open(os.path.join(data, 'uid'))]
    cold = [vids[j] for j in range(m.n_items) if j not in m.i_rated]
    with open(os.path.join(data, 'f0te.om.idl'), 'w') as fh:
        fh.write(''.join(v + '\n' for v in cold))
    with open(os.path.join(data, 'f0te.om.txt'), 'w') as fh:
        for t, u in enumerate(uids[:12]):
            fh.write('%s,%s:1,%s:0,%s:%d\n' % (u, cold[t % 4], cold[(t + 1) % 4], cold[(t + 2) % 4], t % 2))
    got = E.main(['-d', data, '-m', out, '-sl', 'im', 'om'])
    exp = R.evaluate_cli(data, out, scenarios=('im', 'om'))
    assert len(got) == len(exp) == 2 and got[0].startswith('im,') and got[1].startswith('om,')
    for g, e in zip(got, exp):
        assert g.split(',')[0] == e.split(',')[0]
        assert [float(x) for x in g.split(',')[1:]] == [float(x) for x in e.split(',')[1:]]

    # the driver, the content through a pickle as load_content_data reads it
    pkl = str(tmp_path / 'meta.pkl')
    with open(pkl, 'wb') as fh:
        pickle.dump(m.feat, fh)
    out2 = str(tmp_path / 'dpm2')
    argv = ['-d', _g2(golden_dir), '-o', out2, '--model', 'dpm', '--content', pkl, '--dim', str(O.E2E['d']), '--iters', '2', '-k', str(m.k),
            '--lu', str(m.lu), '--lv', str(m.lv), '--seed', str(O.E2E['seed']), '--mlp-seed', str(O.E2E['mlp_seed']), '--mlp-lr', str(O.E2E['lr']),
            '--batch', str(O.E2E['batch']), '--hidden'] + [str(h) for h in O.E2E['hidden']]
    model = train_als.main(argv)
    assert type(model).__name__ == 'DPM' and sorted(os.listdir(out2)) == ['final-U.dat', 'final-V.dat', 'mlp.npz']
    np.testing.assert_array_equal(model.feat, m.feat)
    np.testing.assert_array_equal(_bits(model.fie), _bits(m.fie))               # the same seeds, the same run, the same bits
    np.testing.assert_array_equal(_bits(model.fue), _bits(m.fue))
    assert model.losses == m.losses
