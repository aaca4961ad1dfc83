"""K18 (tkr_line_metrics, tkr_bootstrap_sums) at step = 5, total = 30 (23 columns per model) beside what a user can do without it.

  the line table   at the like counts of ML-10M (69,878 lines x 12 likes, 10,380 columns) and Netflix (480,189 x 12, 17,770), synthetic
                   ranks already on the device, as K8 leaves them:
                     K18 line table           significance.line_table (the two small tables uploaded, the kernel, the status word read back)
                     download + rank_sums     what evaluate.py -M does today: the ranks to the host, rankmetrics.rank_sums (sums only)
  the bootstrap    R = 1000 resamples of n = 69,878 and 480,189 lines, C = 23 and 46 (two models side by side):
                     K18 bootstrap            tkr_hip.bootstrap_sums: the table copied to a row pitch of whole cache lines (32 / 48 doubles), the kernels
                     K18 own pitch            the same without the copy (pad=False): rows of 184 / 368 bytes; the same bits
                     torch gather             randint + index_select + sum, in blocks of replicates
                     torch bincount matmul    per block of replicates a count matrix [block, n] (scatter_add of ones), times X in float64
python scripts/time_significance.py [repeats]
Warm-up of every leg, then `repeats` (5) rounds that alternate the legs in this one process; wall time around a device synchronise
(the host legs are host work).  Prints min / median / max per leg, K18's row-read rate (R * n * C * 8 bytes) and the ratios of medians.
The torch legs draw with torch's generator, not K18's stream: the legs do the same work on different lines."""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'top-k-rec_amd')]
import numpy as np
import torch

import rankmetrics
import significance
import tkr_hip

STEP, TOTAL, R = 5, 30, 1000
SHAPES = [('ml10m', 69878, 10380, 130, 12), ('netflix', 480189, 17770, 150, 12)]      # lines, columns, rated per line, likes per line
GATHER_BLOCK_BYTES = 2 << 30                                        # what the gather leg materialises per block of replicates
COUNT_BLOCK = 50                                                    # replicates per count matrix


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def synthetic(n_lines, n_cols, rated, likes, dev, g):
    """ranks K8 could have produced: ascending distinct ranks from random gaps (about a third of them below 30), one like in twenty rated"""
    gaps = torch.randint(1, 60, (n_lines, likes), device=dev, generator=g)
    ranks = (gaps.cumsum(1) - 1).to(torch.int32)
    assert int(ranks.max()) < n_cols - rated
    ranks[torch.rand((n_lines, likes), device=dev, generator=g) < 0.05] = -1
    like_ptr = torch.arange(n_lines + 1, device=dev, dtype=torch.int64) * likes
    rated_ptr = torch.arange(n_lines + 1, device=dev, dtype=torch.int64) * rated
    return ranks.reshape(-1).contiguous(), like_ptr, rated_ptr


def torch_gather(X, n_rep, g):
    n, C = X.shape
    block = max(1, GATHER_BLOCK_BYTES // (n * C * 8))
    out = torch.empty((n_rep, C), dtype=torch.float64, device=X.device)
    for lo in range(0, n_rep, block):
        hi = min(n_rep, lo + block)
        idx = torch.randint(n, ((hi - lo) * n,), device=X.device, generator=g)
        out[lo:hi] = X.index_select(0, idx).view(hi - lo, n, C).sum(1)
    return out


def torch_counts(X, n_rep, g):
    n, C = X.shape
    out = torch.empty((n_rep, C), dtype=torch.float64, device=X.device)
    ones = torch.ones((COUNT_BLOCK, n), dtype=torch.float64, device=X.device)
    for lo in range(0, n_rep, COUNT_BLOCK):
        hi = min(n_rep, lo + COUNT_BLOCK)
        idx = torch.randint(n, (hi - lo, n), device=X.device, generator=g)
        counts = torch.zeros((hi - lo, n), dtype=torch.float64, device=X.device).scatter_add_(1, idx, ones[:hi - lo])
        out[lo:hi] = counts @ X
    return out


def report(tag, legs, repeats, rate_of=None):
    for _, fn in legs:                                                # warm-up: code objects, the allocator's blocks
        fn()
        fn()
    times = {label: [] for label, _ in legs}
    for _ in range(repeats):
        for label, fn in legs:
            times[label].append(timed(fn))
    med = {label: float(np.median(t)) for label, t in times.items()}
    for label, _ in legs:
        t = times[label]
        extra = ''
        if rate_of and label == rate_of[0]:
            extra = '   %.2f TB/s of row reads' % (rate_of[1] / med[label] / 1e9)
        print('%-22s %-22s min %9.2f  median %9.2f  max %9.2f ms%s' % (tag, label, min(t), med[label], max(t), extra), flush=True)
    first = legs[0][0]
    for label, _ in legs[1:]:
        print('%-22s %s / %s = %.2f' % (tag, label, first, med[label] / med[first]), flush=True)


def main():
    repeats = int(sys.argv[1]) if len(sys.argv) > 1 else 5
    if not torch.cuda.is_available():
        raise SystemExit('time_significance.py measures on the GPU; none is visible')
    dev = torch.device('cuda', 0)
    g = torch.Generator(device=dev)
    g.manual_seed(18)
    for name, n_lines, n_cols, rated, likes in SHAPES:
        ranks, like_ptr, rated_ptr = synthetic(n_lines, n_cols, rated, likes, dev, g)
        lp, rp = like_ptr.cpu().numpy(), rated_ptr.cpu().numpy()
        X = significance.line_table(ranks, like_ptr, rated_ptr, n_cols, STEP, TOTAL)
        sums = rankmetrics.rank_sums(ranks.cpu().numpy(), lp, rp, n_cols, STEP, TOTAL)
        col = X.sum(0).cpu().numpy()
        assert np.array_equal(col[:6], sums['acc'][0]) and col[6] == sums['acc'][1] and col[10] == sums['mrr'][1]
        assert abs(col[9] - sums['mrr'][0]) <= n_lines * 2.0 ** -52 * col[9]
        report('%s table, %d ranks' % (name, ranks.numel()),
               [('K18 line table', lambda: significance.line_table(ranks, like_ptr, rated_ptr, n_cols, STEP, TOTAL)),
                ('download + rank_sums', lambda: rankmetrics.rank_sums(ranks.cpu().numpy(), lp, rp, n_cols, STEP, TOTAL))], repeats)
        for models in (1, 2):
            Xm = X if models == 1 else torch.cat([X, X.flip(0)], dim=1).contiguous()
            C = Xm.shape[1]
            a, b = tkr_hip.bootstrap_sums(Xm, R, 1), tkr_hip.bootstrap_sums(Xm, R, 1, pad=False)
            assert torch.equal(a, b) and bool((a[:, 6] == likes * n_lines).all())           # every line has `likes` likes
            del a, b
            report('%s n = %d, C = %d' % (name, n_lines, C),
                   [('K18 bootstrap', lambda: tkr_hip.bootstrap_sums(Xm, R, 1)), ('K18 own pitch', lambda: tkr_hip.bootstrap_sums(Xm, R, 1, pad=False)),
                    ('torch gather', lambda: torch_gather(Xm, R, g)),
                    ('torch bincount matmul', lambda: torch_counts(Xm, R, g))], repeats, ('K18 bootstrap', R * n_lines * C * 8.0))
        del X, Xm, ranks


if __name__ == '__main__':
    main()
