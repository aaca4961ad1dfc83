"""K16 (tkr_fusion_*: the weights of a fusion of several models) at the ML-10M shape (69,878 x 10,380; synth.train_csr_shape's
training likes), M = 3 and 8 models at k = 128 and k = 50, the reference's 10,000,000 samples in batches of 10,000 (999 batches run),
beside the same computation in torch on the same device:
  features     tkr_fusion_features over a chunk of whole batches (D <= 256 MB)   | torch: index_select of the rows + products + sums
  sgd          tkr_fusion_sgd over that chunk's batches, one workgroup           | torch: a per-batch loop (matmul, sigmoid, matmul)
  pairwise     fusion.learn_pairwise, all 999 batches end to end
  per-user     tkr_fusion_user_weights over the shape's training likes           | torch: index_select + products, index_add per user
  K4           one score_topk pass (top 30) on fused tables of width 400 and 1,032
python scripts/time_fusion.py [repeats]
Warm-up of every leg, then `repeats` rounds that alternate the legs in this one process; each pass is timed by a pair of device
events.  Prints min / median / max per leg in ms.  (One thread mapping of the features kernel is built: a lane per triplet.)"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'top-k-rec_amd')]
import numpy as np
import torch

import fusion
import synth
import tkr_hip
from single import _engine

N_USERS, N_ITEMS = 69878, 10380
SAMPLES, BATCH = 10_000_000, 10_000
LR, LAMBDA_W = 1e-4, 0.0025


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def make_models(M, k, dev, seed=3):
    g = torch.Generator(device=dev)
    g.manual_seed(seed)
    rnd = lambda *shape: ((torch.randn(shape, device=dev, generator=g) * 0.1 * 1e6).round() / 1e6).contiguous()
    return [(rnd(N_USERS, k), rnd(N_ITEMS, k), rnd(N_ITEMS) if m % 2 else None) for m in range(M)]


def torch_features(models, trip):
    u, i, j = (trip[:, c].long() for c in range(3))
    cols = []
    for U, V, b in models:
        d = (U.index_select(0, u) * (V.index_select(0, i) - V.index_select(0, j))).sum(dim=1)
        cols.append(d if b is None else d + (b.index_select(0, i) - b.index_select(0, j)))
    return torch.stack(cols, dim=1)


def torch_sgd(D, nb, W):
    for z in range(nb):
        d = D[z * BATCH:(z + 1) * BATCH]
        W += LR * (torch.sigmoid(-(d @ W)) @ d - LAMBDA_W * W)
    return W


def torch_user_weights(models, like_ptr, like_cols):
    n_like = (like_ptr[1:] - like_ptr[:-1])
    rows = torch.repeat_interleave(torch.arange(N_USERS, device=like_cols.device), n_like)
    cols = like_cols.long()
    r = []
    for U, V, b in models:
        s = (U.index_select(0, rows) * V.index_select(0, cols)).sum(dim=1)
        if b is not None:
            s = s + b.index_select(0, cols)
        sq = torch.zeros(N_USERS, device=s.device).index_add_(0, rows, (s - 1) ** 2)
        r.append(torch.sqrt(sq / n_like.clamp(min=1)))
    r = torch.stack(r, dim=1)
    return r, torch.exp(-(r - r.mean(dim=1, keepdim=True)))


def report(name, legs, repeats):
    for _, fn in legs:                                               # warm-up: code objects, the allocator's blocks
        fn()
        fn()
    torch.cuda.synchronize()
    times = {label: [] for label, _ in legs}
    for _ in range(repeats):
        for label, fn in legs:
            times[label].append(timed(fn))
    for label, _ in legs:
        t = times[label]
        print('%-22s %-28s min %9.3f  median %9.3f  max %9.3f ms' % (name, label, min(t), float(np.median(t)), max(t)), flush=True)
    return {label: float(np.median(t)) for label, t in times.items()}


def main():
    repeats = int(sys.argv[1]) if len(sys.argv) > 1 else 5
    if not torch.cuda.is_available():
        raise SystemExit('time_fusion.py measures on the GPU; none is visible')
    dev = torch.device('cuda', 0)
    row_ptr, pos, srt, tr_users = synth.train_csr_shape(N_USERS, N_ITEMS)
    csr = _engine.TrainingCSR.from_arrays(row_ptr, pos, tr_users, dev)
    like_ptr = torch.from_numpy(row_ptr.astype(np.int64)).to(dev)
    like_cols = torch.from_numpy(srt).to(dev)
    nb = fusion.n_batches_of(SAMPLES, BATCH)
    print('shape %d x %d, %d training likes; %d samples, batch %d: %d batches' % (N_USERS, N_ITEMS, csr.nnz, SAMPLES, BATCH, nb), flush=True)
    for M in (3, 8):
        for k in (128, 50):
            models = make_models(M, k, dev)
            name = 'M = %d, k = %d' % (M, k)
            chunk = min(nb, max(1, fusion.CHUNK_BYTES // (4 * M * BATCH)))          # batches per chunk, as learn_pairwise cuts them
            rows = chunk * BATCH
            D, trip = tkr_hip.fusion_features(models, csr, N_ITEMS, 0, 0, rows, want_triplets=True)
            Dt = torch_features(models, trip)
            print('%-22s chunk of %d batches (%d rows, D %.0f MB); max |D - torch D| = %.2g' %
                  (name, chunk, rows, rows * M * 4 / 2 ** 20, float((D - Dt).abs().max())), flush=True)
            del Dt
            W = torch.zeros(M, device=dev)
            report(name, [('features (chunk)', lambda: tkr_hip.fusion_features(models, csr, N_ITEMS, 0, 0, rows)),
                          ('torch features (chunk)', lambda: torch_features(models, trip)),
                          ('sgd (chunk)', lambda: tkr_hip.fusion_sgd(D, BATCH, chunk, LR, LAMBDA_W, W.zero_())),
                          ('torch sgd (chunk)', lambda: torch_sgd(D, chunk, W.zero_()))], repeats)
            del D, trip
            report(name, [('learn_pairwise (999 b.)', lambda: fusion.learn_pairwise(models, csr, N_ITEMS, n_samples=SAMPLES, batch_size=BATCH,
                                                                                   lr=LR, lambda_w=LAMBDA_W))], max(2, repeats // 2))
            rk, wk = tkr_hip.fusion_user_weights(models, like_ptr, like_cols)
            rt, wt = torch_user_weights(models, like_ptr, like_cols)
            print('%-22s per-user: max |rmse - torch| = %.2g, max |w - torch| = %.2g' %
                  (name, float((rk - rt).abs().max()), float((wk - wt).abs().max())), flush=True)
            del rk, wk, rt, wt
            report(name, [('user_weights', lambda: tkr_hip.fusion_user_weights(models, like_ptr, like_cols)),
                          ('torch user weights', lambda: torch_user_weights(models, like_ptr, like_cols))], repeats)
            del models
    for n, kk, biased in ((8, 50, False), (8, 128, True)):            # fused widths 400 and 1,032 (8 x 128 + 8 bias columns)
        g = torch.Generator(device=dev)
        g.manual_seed(5)
        ms = [(torch.randn((N_USERS, kk), device=dev, generator=g) * 0.1, torch.randn((N_ITEMS, kk), device=dev, generator=g) * 0.1,
               torch.randn(N_ITEMS, device=dev, generator=g) * 0.1 if biased else None) for _ in range(n)]
        Uf, Vf = fusion.fuse(ms, fusion.fixed_weights(n, 'a'))
        del ms
        report('K4 fused width %d' % Uf.shape[1], [('score_topk top 30', lambda: tkr_hip.score_topk(Uf, Vf, 30))], repeats)
        del Uf, Vf


if __name__ == '__main__':
    main()
