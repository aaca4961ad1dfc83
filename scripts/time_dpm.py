"""K22 (the MLP encoder of DPM: als.MLP.out, als.MLP.fit, and one iteration of als.DPM.train's loop) at the ML-10M shape (69,878 users x
10,380 items, likes drawn as scripts/time_cer.py draws them, every fifth item cold), dense standard-normal features of d = 1,024 and
20,000, k = 50 and 128, hidden layers (2000, 1000), batches of 64:
  out     the encoder over all items (tkr_mlp_forward)
  fit     one epoch (tkr_mlp_fit: 163 batches), and its time per batch
  legs    of out and fit: K22, and torch on the same device -- index_select, addmm, sigmoid, a hand-written backward with mm and the
          same RMSProp formula in elementwise operations (dW is materialised, the optimiser is several passes).  Both legs start from
          the same parameters; what they leave is compared first.
  phases  of one DPM iteration: out, the user half-step (K20), the item half-step (K21), fit
  bytes   the model of a batch: per layer 4 |W| * 5 (W read by the forward pass, W and its slot read and written by the step) plus the
          activations, partials and deltas; the share of the HBM rate (6.29 TB/s, a float4 copy) one batch of fit reaches
python scripts/time_dpm.py [repeats] [k ...]      (TIME_DPM_D=1024,20000 picks the feature widths; TIME_DPM_ONLY=fit runs one warm and
one timed epoch of K22 and nothing else: the run to put under a kernel trace, whose per-kernel sums split a batch into forward
(mlp_gemm_kernel<false>, mlp_reduce_kernel), deltas (mlp_loss_kernel, mlp_gemm_kernel<true>) and update (mlp_update_kernel))
Warm-up of every leg, then `repeats` rounds that alternate the legs in this one process; each pass is timed by a pair of device events;
medians with min and max beside them."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'top-k-rec_amd')]
import numpy as np
import torch

import als
import synth
import tkr_hip
from time_als import SHAPES, timed
from time_cer import csr_of, report

A, B, LU, LV = 1.0, 0.01, 0.01, 10.0
HIDDEN, BATCH, LR = (2000, 1000), 64, 1e-4
RHO, EPS = 0.9, 1e-10
HBM = 6.29e12


def torch_forward(P, x):
    hs = [x]
    for l, (W, b) in enumerate(zip(P['W'], P['bias'])):
        z = torch.addmm(b, hs[-1], W)
        hs.append(z if l + 1 == len(P['W']) else torch.sigmoid(z))
    return hs


def torch_out(P, X, chunk=tkr_hip.MLP_FORWARD_CHUNK):
    return torch.cat([torch_forward(P, X[c:c + chunk])[-1] for c in range(0, X.shape[0], chunk)])


def torch_fit(P, X, Y, order, batch, lr):
    """one epoch, in place on P (lists W, bias, msW, msb) -> the sum of the batch objectives (a device scalar)"""
    total = torch.zeros((), dtype=torch.float64, device=X.device)
    one_minus_rho = float(np.float32(1) - np.float32(RHO))
    for t in range(0, order.numel(), batch):
        rows = order[t:t + batch]
        hs = torch_forward(P, X.index_select(0, rows))
        delta = hs[-1] - Y.index_select(0, rows)
        total += 0.5 * delta.double().square().sum()
        grads = [None] * len(P['W'])
        for l in range(len(P['W']) - 1, -1, -1):
            grads[l] = (torch.mm(hs[l].t(), delta), delta.sum(dim=0))
            if l:
                delta = torch.mm(delta, P['W'][l].t()) * (hs[l] * (1 - hs[l]))
        for l, (gW, gb) in enumerate(grads):
            for w, ms, g in ((P['W'][l], P['msW'][l], gW), (P['bias'][l], P['msb'][l], gb)):
                ms.add_((g * g - ms) * one_minus_rho)
                w.sub_(lr * g / torch.sqrt(ms + EPS))
    return total


def batch_bytes(widths, batch):
    """the bytes one batch of tkr_mlp_fit moves, by the model of the docstring -> (parameters' part, the rest)"""
    params = rest = 0
    slabs = lambda n: (n + tkr_hip.MLP_SLAB - 1) // tkr_hip.MLP_SLAB
    for l, (n_in, n_out) in enumerate(zip(widths, widths[1:])):
        params += 4 * (n_in * n_out + n_out) * 5
        rest += 4 * batch * (n_in + 2 * slabs(n_in) * n_out + 2 * n_out)      # the input read, the partials written and read, the activation written
        rest += 4 * batch * (n_in + n_out)                                    # the step reads the input and the deltas
        if l:
            params += 4 * n_in * n_out                                        # the delta carried back reads W once more
            rest += 4 * batch * (n_out + 2 * slabs(n_out) * n_in + 2 * n_in)
    return params, rest


def clone_params(enc):
    P = {name: [layer[name].clone() for layer in enc._dev] for name in ('W', 'bias', 'msW', 'msb')}
    return P


def worst(enc, P):
    return max(float((layer[name] - P[name][l]).abs().max() / layer[name].abs().max()) for l, layer in enumerate(enc._dev) for name in P)


def main():
    args = sys.argv[1:]
    repeats = int(args[0]) if args else 3
    ks = [int(x) for x in args[1:]] or [50, 128]
    ds = [int(x) for x in os.environ.get('TIME_DPM_D', '1024,20000').split(',')]
    only_fit = os.environ.get('TIME_DPM_ONLY') == 'fit'
    if not torch.cuda.is_available():
        raise SystemExit('time_dpm.py measures on the GPU; none is visible')
    dev = torch.device('cuda', 0)
    n_users, n_items = SHAPES['ml10m']
    d_ = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    if not only_fit:
        row_ptr, pos, _, _ = synth.train_csr_shape(n_users, n_items)
        users = np.repeat(np.arange(n_users, dtype=np.int64), np.diff(row_ptr))
        items = np.asarray(pos, dtype=np.int64)
        keep = items % 5 != 0                                         # every fifth item loses its likes
        users, items = users[keep], items[keep]
        up, uc = csr_of(users, items, n_users)
        ip, ic = csr_of(items, users, n_items)
        u_rated, i_rated = np.flatnonzero(np.diff(up) > 0).astype(np.int32), np.flatnonzero(np.diff(ip) > 0).astype(np.int32)
        print('ml10m: %d users x %d items, %d likes; %d items with likes' % (n_users, n_items, len(uc), len(i_rated)), flush=True)
        upd, ucd, ipd, icd, urd, ird = d_(up), d_(uc), d_(ip), d_(ic), d_(u_rated), d_(i_rated)
    for dd in ds:
        g = torch.Generator(device=dev)
        g.manual_seed(22)
        F = torch.randn((n_items, dd), device=dev, generator=g)
        for k in ks:
            widths = (dd,) + HIDDEN + (k,)
            V0 = torch.rand((n_items, k), device=dev, generator=g)
            order = d_(als.epoch_order(0, 0, n_items))
            n_batches = (n_items + BATCH - 1) // BATCH
            enc = als.MLP(k, dd, lr=LR, hidden_layers=HIDDEN, seed=0)
            enc.out(F[:1])                                            # the parameters go to the device
            start = clone_params(enc)
            pb, rest = batch_bytes(widths, BATCH)
            tag = 'd %-5d k %-4d' % (dd, k)

            def reset():
                for l, layer in enumerate(enc._dev):
                    for name in start:
                        layer[name].copy_(start[name][l])

            fit_k22 = lambda: enc._fit_device(F, V0, BATCH, order)
            if only_fit:
                fit_k22()
                reset()
                ms = timed(fit_k22)
                print('%s one epoch of K22, %d batches: %.3f ms' % (tag, n_batches, ms), flush=True)
                continue
            P = clone_params(enc)
            # the two legs from one start: what they leave, compared
            loss_k = float(fit_k22()[0].sum())
            loss_t = float(torch_fit(P, F, V0, order.long(), BATCH, LR))
            out_k, out_t = enc.out(F), torch_out(P, F)
            print('%s K22 against torch after one epoch: parameters and slots max |d| / max = %.3g, out %.3g, objective %.9g against %.9g (%.3g)'
                  % (tag, worst(enc, P), float((out_k - out_t).abs().max() / out_t.abs().max()), loss_k, loss_t, abs(loss_k - loss_t) / loss_t), flush=True)
            U, V, w = torch.rand((n_users, k), device=dev, generator=g), V0.clone(), als.Work()
            st = {}
            legs = {
                'out over all items (K22)': lambda: st.__setitem__('Fe', enc.out(F)),
                'out over all items, torch addmm': lambda: torch_out(P, F),
                'user half-step (K20)': lambda: als.half_step(U, st['Fe'], upd, ucd, ird, w=w, ridge_in_G=LU, ridge=0.0, a=A, b=B),
                'item half-step (K21)': lambda: als.half_step(V, U, ipd, icd, urd, w=w, ridge_in_G=0.0, ridge=LV, a=A, b=B, want_loss=True,
                                                              prior=st['Fe'], w_prior=LV),
                'fit, one epoch (K22)': fit_k22,
                'fit, one epoch, torch': lambda: torch_fit(P, F, V0, order.long(), BATCH, LR),
            }
            for fn in legs.values():
                fn()
            torch.cuda.synchronize()
            times = {label: [] for label in legs}
            for _ in range(repeats):
                for label, fn in legs.items():
                    times[label].append(timed(fn))
            med = {label: report('%s %s' % (tag, label), ms) for label, ms in times.items()}
            per_batch = med['fit, one epoch (K22)'] / n_batches
            print('%s fit per batch: K22 %.3f ms, torch %.3f ms (torch / K22 = %.2f); out: torch / K22 = %.2f'
                  % (tag, per_batch, med['fit, one epoch, torch'] / n_batches, med['fit, one epoch, torch'] / med['fit, one epoch (K22)'],
                     med['out over all items, torch addmm'] / med['out over all items (K22)']), flush=True)
            print('%s bytes per batch by the model: %.1f MB of parameters and slots + %.1f MB of activations, partials and deltas = %.2f us at %.2f TB/s: '
                  'K22 reaches %.1f %% of the HBM rate' % (tag, pb / 1e6, rest / 1e6, (pb + rest) / HBM * 1e6, HBM / 1e12,
                                                           100 * (pb + rest) / HBM / (per_batch * 1e-3)), flush=True)
            total = sum(med[x] for x in ('out over all items (K22)', 'user half-step (K20)', 'item half-step (K21)', 'fit, one epoch (K22)'))
            print('%s one DPM iteration = %.3f ms: out %.1f %%, users %.1f %%, items %.1f %%, fit %.1f %%'
                  % (tag, total, 100 * med['out over all items (K22)'] / total, 100 * med['user half-step (K20)'] / total,
                     100 * med['item half-step (K21)'] / total, 100 * med['fit, one epoch (K22)'] / total), flush=True)
            del enc, P, start, st, w
        del F
        torch.cuda.empty_cache()


if __name__ == '__main__':
    main()
