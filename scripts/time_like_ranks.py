"""K8 (tkr_like_ranks: the filtered rank of every liked column, one full-rank pass) beside K4 (tkr_score_topk, K = 30, fp32 MFMA: the
same U x V^T products with selection in place of counting) on the same inputs, at the two benchmark shapes.
python scripts/time_like_ranks.py [ml10m|netflix|both] [repeats]
Warm-up of both kernels at every shape, then `repeats` rounds that alternate the two; each pass is timed by a pair of device events.
Prints min / median / max per kernel, the ratio of the medians and the fp32 rate 2 k n_rows n_cols / time of each."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'top-k-rec_amd')]
import numpy as np
import torch

import tkr_hip

which = sys.argv[1] if len(sys.argv) > 1 else 'both'
repeats = int(sys.argv[2]) if len(sys.argv) > 2 else 7
if not torch.cuda.is_available():
    raise SystemExit('time_like_ranks.py measures on the GPU; none is visible')
dev = torch.device('cuda', 0)
shapes = [('ml10m', 69878, 10380, 130, 12), ('netflix', 480189, 17770, 150, 12)]      # rows, columns, rated per row, likes per row
k, K = 128, 30


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


for name, n_rows, n_cols, deg, n_like in shapes:
    if which not in ('both', name):
        continue
    g = torch.Generator(device=dev)
    g.manual_seed(11)
    U = (torch.randn((n_rows, k), device=dev, generator=g) * 0.01 * 1e6).round() / 1e6
    V = (torch.randn((n_cols, k), device=dev, generator=g) * 0.01 * 1e6).round() / 1e6
    rptr = torch.arange(0, (n_rows + 1) * deg, deg, dtype=torch.int64, device=dev)
    rcols = torch.randint(0, n_cols, (n_rows * deg,), device=dev, generator=g, dtype=torch.int32)
    mask, pitch = tkr_hip.build_rated_mask(rptr, rcols, n_rows, n_cols)
    # n_like distinct ascending columns per row: one draw inside each of n_like equal strides of the catalogue
    stride = n_cols // n_like
    lcols = (torch.randint(0, stride, (n_rows, n_like), device=dev, generator=g, dtype=torch.int32)
             + torch.arange(n_like, device=dev, dtype=torch.int32) * stride).reshape(-1).contiguous()
    lptr = torch.arange(0, (n_rows + 1) * n_like, n_like, dtype=torch.int64, device=dev)
    tkr_hip.set_topk_math('fp32')
    run_k8 = lambda: tkr_hip.like_ranks(U, V, lptr, lcols, mask=mask, mask_pitch=pitch)
    run_k4 = lambda: tkr_hip.score_topk(U, V, K, mask=mask, mask_pitch=pitch)
    for _ in range(2):                                              # warm-up: code objects, workspaces, the item table of K4
        ranks, ids = run_k8(), run_k4()
    torch.cuda.synchronize()
    ranks = ranks.cpu().numpy()
    print('%-8s %d x %d, k = %d, %d likes per row: %.1f %% of them rated, median rank %d' %
          (name, n_rows, n_cols, k, n_like, 100.0 * np.mean(ranks < 0), int(np.median(ranks[ranks >= 0]))), flush=True)
    t8, t4 = [], []
    for _ in range(repeats):
        t8.append(timed(run_k8))
        t4.append(timed(run_k4))
    flop = 2.0 * k * n_rows * n_cols
    for label, t in (('K8 like_ranks', t8), ('K4 top-%d fp32' % K, t4)):
        print('%-8s %-16s min %8.2f  median %8.2f  max %8.2f ms   %6.1f TFLOP/s fp32 (median)' %
              (name, label, min(t), float(np.median(t)), max(t), flop / float(np.median(t)) / 1e9), flush=True)
    print('%-8s K8 / K4 = %.2f' % (name, float(np.median(t8)) / float(np.median(t4))), flush=True)
    tkr_hip.set_topk_math(tkr_hip.TOPK_MATH_DEFAULT)
    del U, V, mask, rcols, lcols
