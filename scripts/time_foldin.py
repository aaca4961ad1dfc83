"""K9 (tkr_bpr_foldin: user vectors folded in against frozen item factors) at the two benchmark shapes, beside the training rate of
BPR.train's step at batch 256 on the same shape and in the same process.
python scripts/time_foldin.py [ml10m|netflix|both] [repeats]
Every user of the shape is folded in from ~36 positives: k = 128, T = 50 steps of P = 16 triplets.  Warm-up, then `repeats` passes,
each timed by a pair of device events.  Prints users/s, triplets/s and the bytes of item rows gathered (m T P 2 k 4) over the time,
then the triplets/s of BprEngine.run_batches (K1 + the persistent step + the loss, what BPR.train runs per epoch) at batch 256, and
their ratio: fold-in does strictly less per triplet (no item update, no plan, no versions), so it must not be the slower one."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'top-k-rec_amd')]
import numpy as np
import torch

import synth
import tkr_hip
from single import _engine

which = sys.argv[1] if len(sys.argv) > 1 else 'both'
repeats = int(sys.argv[2]) if len(sys.argv) > 2 else 5
if not torch.cuda.is_available():
    raise SystemExit('time_foldin.py measures on the GPU; none is visible')
dev = torch.device('cuda', 0)
shapes = [('ml10m', 69878, 10380), ('netflix', 480189, 17770)]
k, T, P, B, mean_pos = 128, 50, 16, 256, 36.0


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


for name, n_users, n_items in shapes:
    if which not in ('both', name):
        continue
    row_ptr, pos, srt, tr_users = synth.train_csr_shape(n_users, n_items, mean_pos=mean_pos, seed=42)
    g = torch.Generator(device=dev)
    g.manual_seed(11)
    V = torch.randn((n_items, k), device=dev, generator=g) * 0.1
    b = torch.randn(n_items, device=dev, generator=g) * 0.1
    ptr = torch.from_numpy(row_ptr.astype(np.int64)).to(dev)
    cols = torch.from_numpy(srt).to(dev)
    run = lambda: tkr_hip.fold_in(V, b, ptr, cols, lu=2.5e-3, lr=0.05, steps=T, triplets=P, seed=1)
    for _ in range(2):
        U = run()
    torch.cuda.synchronize()
    live = int(((np.diff(row_ptr) > 0) & (np.diff(row_ptr) < n_items)).sum())
    print('%-8s %d users x %d items, k = %d, %.1f positives per user, T = %d, P = %d; mean |u| after fold-in %.3f'
          % (name, n_users, n_items, k, len(srt) / n_users, T, P, float(U.norm(dim=1).mean())), flush=True)
    t = [timed(run) for _ in range(repeats)]
    med = float(np.median(t)) * 1e-3
    trip = live * T * P
    fold_rate = trip / med
    print('%-8s K9 fold-in     min %8.2f  median %8.2f  max %8.2f ms   %.2f M users/s  %.1f M triplets/s  %.0f GB/s of item rows gathered'
          % (name, min(t), med * 1e3, max(t), live / med / 1e6, fold_rate / 1e6, trip * 2.0 * k * 4 / med / 1e9), flush=True)
    del U
    hp = dict(lu=2.5e-3, li=2.5e-3, lj=2.5e-4, lb=0.0, lr=1e-4, mode='l2')
    csr = _engine.TrainingCSR.from_arrays(row_ptr, pos, tr_users, dev)
    eng = _engine.BprEngine(n_users, n_items, k, hp, dev, seed=1)
    nb = 3906                                                       # 10^6 triplets, the epoch of the reference's train.py
    eng.run_batches(csr, nb, B, want_loss=True)
    torch.cuda.synchronize()
    tt = [timed(lambda: eng.run_batches(csr, nb, B, want_loss=True)) for _ in range(repeats)]
    eng.check()
    train_rate = nb * B / (float(np.median(tt)) * 1e-3)
    print('%-8s BPR.train step min %8.2f  median %8.2f  max %8.2f ms   %.1f M triplets/s at batch %d (%s)'
          % (name, min(tt), float(np.median(tt)), max(tt), train_rate / 1e6, B, getattr(eng, 'layout', '?')), flush=True)
    print('%-8s fold-in / training = %.2f per triplet (the bar: >= 1)' % (name, fold_rate / train_rate), flush=True)
    del eng, csr, V, b, ptr, cols
