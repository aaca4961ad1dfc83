"""K17 (tkr_mmr_select: greedy MMR over a pool per row) at the ML-10M shape (69,878 users x 10,380 items, k = 128), pool 100 -> 30 and
pool 500 -> 30, beside what a user can do without it on the same device:
  legs   K17 select            tkr_hip.mmr_select alone, on a prepared S and rel
         K17 prepare+rerank    diversity.prepare + diversity.rerank: the normalised table, the relevances, the select, the gathers
         K4 pool + K17         the K4 pass that makes the pool (score_topk, K = pool) in front of that
         torch greedy          index_select of the pool's rows of S -> bmm Gram [rows, N, N] -> a t-step greedy loop of torch ops, in
                               blocks of rows (K4 excluded, as 'K17 prepare+rerank')
         K4 top-30             one K4 pass for the plain lists, for scale
python scripts/time_diversity.py [100|500|both] [repeats]
Warm-up of every leg, then `repeats` rounds that alternate the legs in this one process; each pass is timed by a pair of device events.
Prints min / median / max per leg, K17's share of the gather roofline (rows * N * 4 k bytes, every pool row of S once, at the 8.6 TB/s
measured for random rows of an Infinity-Cache-resident table) and the ratio of the medians.  The two selections are compared first: they
must agree on every row outside those where some pick's two best objectives lie within 2^-20 of each other (the torch leg sums the
similarities in BLAS order, K17 in the library's chain order)."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'top-k-rec_amd')]
import numpy as np
import torch

import diversity
import tkr_hip

GATHER_TBS = 8.6
N_USERS, N_COLS, K_FACTORS, TOTAL, LAM = 69878, 10380, 128, 30, 0.7
GAP = 2.0 ** -20
BLOCK = {100: 16384, 500: 2048}                                     # rows per block of the torch leg: the Gram is block * N * N * 4 bytes


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def torch_mmr(S, ids, rel, lam, t, block):
    """the same greedy selection with torch alone -> (sel_pos int64 [n, t], ambiguous bool [n]); every pool entry valid"""
    n, N = ids.shape
    lam32 = torch.tensor(lam, dtype=torch.float32, device=S.device)
    mu32 = 1.0 - lam32
    sel = torch.empty((n, t), dtype=torch.int64, device=S.device)
    amb = torch.zeros(n, dtype=torch.bool, device=S.device)
    for lo in range(0, n, block):
        hi = min(n, lo + block)
        rows = S.index_select(0, ids[lo:hi].reshape(-1).long()).view(hi - lo, N, -1)
        G = torch.bmm(rows, rows.transpose(1, 2))
        a = lam32 * rel[lo:hi]
        pen = torch.full_like(a, float('-inf'))
        taken = torch.zeros_like(a, dtype=torch.bool)
        for r in range(t):
            obj = (a if r == 0 else a - mu32 * pen).masked_fill(taken, float('-inf'))
            top = obj.topk(2, dim=1)
            p = top.indices[:, :1]
            if r + 1 < N:
                amb[lo:hi] |= (top.values[:, 0] - top.values[:, 1]) <= GAP
            sel[lo:hi, r] = p[:, 0]
            taken.scatter_(1, p, True)
            pen = torch.maximum(pen, G.gather(2, p.unsqueeze(1).expand(-1, N, 1)).squeeze(2))
    return sel, amb


def main():
    which = sys.argv[1] if len(sys.argv) > 1 else 'both'
    repeats = int(sys.argv[2]) if len(sys.argv) > 2 else 5
    if not torch.cuda.is_available():
        raise SystemExit('time_diversity.py measures on the GPU; none is visible')
    dev = torch.device('cuda', 0)
    g = torch.Generator(device=dev)
    g.manual_seed(17)
    U = (torch.randn((N_USERS, K_FACTORS), device=dev, generator=g) * 0.01 * 1e6).round() / 1e6
    V = (torch.randn((N_COLS, K_FACTORS), device=dev, generator=g) * 0.01 * 1e6).round() / 1e6
    wrong = 0
    for pool in (100, 500):
        if which not in ('both', str(pool)):
            continue
        ids, scores = tkr_hip.score_topk(U, V, pool, want_scores=True)
        S, rel = diversity.prepare(V, ids, scores, 'cosine')
        legs = [('K17 select', lambda: tkr_hip.mmr_select(S, ids, rel, LAM, TOTAL)),
                ('K17 prepare+rerank', lambda: diversity.rerank(*diversity.prepare(V, ids, scores, 'cosine'), ids, scores, LAM, TOTAL)),
                ('K4 pool + K17', lambda: (lambda i, s: diversity.rerank(*diversity.prepare(V, i, s, 'cosine'), i, s, LAM, TOTAL))(
                    *tkr_hip.score_topk(U, V, pool, want_scores=True))),
                ('torch greedy', lambda: torch_mmr(S, ids, rel, LAM, TOTAL, BLOCK[pool])),
                ('K4 top-30', lambda: tkr_hip.score_topk(U, V, TOTAL))]
        out = [fn() for _, fn in legs for _ in range(2)]            # warm-up: code objects, workspaces, the allocator's blocks
        torch.cuda.synchronize()
        mine, (theirs, amb) = out[1].long(), out[7]
        differ = (mine != theirs).any(dim=1)
        bad = int((differ & ~amb).sum())
        wrong += bad
        print('pool %d -> %d: %d rows, k = %d; ambiguous rows %d, rows that differ %d, of them not ambiguous %d; rows whose picks are not '
              'the score order %.1f %%' % (pool, TOTAL, N_USERS, K_FACTORS, int(amb.sum()), int(differ.sum()), bad,
                                           100.0 * float((mine != torch.arange(TOTAL, device=dev)).any(dim=1).float().mean())), flush=True)
        del out, mine, theirs, amb, differ
        times = {label: [] for label, _ in legs}
        for _ in range(repeats):
            for label, fn in legs:
                times[label].append(timed(fn))
        gather = N_USERS * pool * 4.0 * K_FACTORS
        for label, _ in legs:
            t = times[label]
            extra = ''
            if label == 'K17 select':
                tbs = gather / float(np.median(t)) / 1e9
                extra = '   gather %.3f TB/s = %.1f %% of %.1f TB/s' % (tbs, 100.0 * tbs / GATHER_TBS, GATHER_TBS)
            print('pool %-4d %-20s min %9.2f  median %9.2f  max %9.2f ms%s' % (pool, label, min(t), float(np.median(t)), max(t), extra), flush=True)
        for a, b in (('torch greedy', 'K17 prepare+rerank'), ('torch greedy', 'K17 select'), ('K4 pool + K17', 'K4 top-30')):
            print('pool %-4d %s / %s = %.2f' % (pool, a, b, float(np.median(times[a])) / float(np.median(times[b]))), flush=True)
        del ids, scores, S, rel
    assert wrong == 0, '%d rows differ between K17 and the torch leg without being ambiguous' % wrong


if __name__ == '__main__':
    main()
