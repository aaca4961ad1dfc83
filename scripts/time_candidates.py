"""K12 (tkr_rank_candidates: score and rank per-user candidate lists) at the ML-10M shape (69,878 x 10,380, k = 128), beside what a user
can do without it on the same device:
  negatives   101 candidates for each of 12 likes per user (838,536 rows): the sampled-negatives protocol
  rerank      500 candidates per user (69,878 rows): re-ranking a shortlist
  legs        K12 | torch: index-select of the item rows + bmm + sort, in blocks of rows | (rerank only) one K4 top-30 pass over the
              whole catalogue, for scale
python scripts/time_candidates.py [negatives|rerank|both] [repeats]
Warm-up of every leg, then `repeats` rounds that alternate the legs in this one process; each pass is timed by a pair of device events.
Prints min / median / max per leg, K12's share of the gather roofline (nnz * 4 k bytes at the 8.6 TB/s measured for random rows of an
Infinity-Cache-resident table) and the ratio of the medians."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'top-k-rec_amd')]
import numpy as np
import torch

import tkr_hip

GATHER_TBS = 8.6
N_USERS, N_COLS, K_FACTORS = 69878, 10380, 128
SHAPES = {'negatives': (12, 101), 'rerank': (1, 500)}               # rows per user, candidates per row


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def make_inputs(name, dev, seed=11):
    """-> U, V, user_idx [n_rows], cand_ptr, cand_cols: `per_row` distinct ascending columns per row, one draw inside each of per_row
    equal strides of the catalogue"""
    per_user, per_row = SHAPES[name]
    g = torch.Generator(device=dev)
    g.manual_seed(seed)
    U = (torch.randn((N_USERS, K_FACTORS), device=dev, generator=g) * 0.01 * 1e6).round() / 1e6
    V = (torch.randn((N_COLS, K_FACTORS), device=dev, generator=g) * 0.01 * 1e6).round() / 1e6
    n_rows = N_USERS * per_user
    user_idx = torch.arange(N_USERS, device=dev, dtype=torch.int32).repeat_interleave(per_user).contiguous()
    stride = N_COLS // per_row
    cols = (torch.randint(0, stride, (n_rows, per_row), device=dev, generator=g, dtype=torch.int32)
            + torch.arange(per_row, device=dev, dtype=torch.int32) * stride).reshape(-1).contiguous()
    ptr = torch.arange(0, (n_rows + 1) * per_row, per_row, dtype=torch.int64, device=dev)
    return U, V, user_idx, ptr, cols


def torch_rank(U, V, user_idx, cols, per_row, block=65536):
    """the same scores (BLAS order) and ranks with torch alone: gather the item rows, one batched product, a sort; `block` rows at a
    time (the gathered rows of a block are block * per_row * 4 k bytes)"""
    n_rows = user_idx.numel()
    scores = torch.empty((n_rows, per_row), dtype=torch.float32, device=U.device)
    ranks = torch.empty((n_rows, per_row), dtype=torch.int64, device=U.device)
    place = torch.arange(per_row, device=U.device).expand(block, per_row)
    c2 = cols.view(n_rows, per_row)
    for lo in range(0, n_rows, block):
        hi = min(n_rows, lo + block)
        rows = V.index_select(0, c2[lo:hi].reshape(-1).long()).view(hi - lo, per_row, -1)
        s = torch.bmm(rows, U.index_select(0, user_idx[lo:hi].long()).unsqueeze(2)).squeeze(2)
        scores[lo:hi] = s
        ranks[lo:hi].scatter_(1, torch.argsort(s, dim=1, descending=True), place[:hi - lo])
    return scores, ranks


def main():
    which = sys.argv[1] if len(sys.argv) > 1 else 'both'
    repeats = int(sys.argv[2]) if len(sys.argv) > 2 else 5
    if not torch.cuda.is_available():
        raise SystemExit('time_candidates.py measures on the GPU; none is visible')
    dev = torch.device('cuda', 0)
    for name, (per_user, per_row) in SHAPES.items():
        if which not in ('both', name):
            continue
        U, V, user_idx, ptr, cols = make_inputs(name, dev)
        n_rows, nnz = user_idx.numel(), cols.numel()
        legs = [('K12 rank_candidates', lambda: tkr_hip.rank_candidates(U, V, ptr, cols, user_idx=user_idx)),
                ('torch gather+bmm+sort', lambda: torch_rank(U, V, user_idx, cols, per_row))]
        if name == 'rerank':
            legs.append(('K4 top-30, catalogue', lambda: tkr_hip.score_topk(U, V, 30)))
        out = [fn() for _, fn in legs for _ in range(2)]            # warm-up: code objects, workspaces, the allocator's blocks
        torch.cuda.synchronize()
        s12, r12 = out[1]
        st, rt = out[3]
        print('%-9s %d rows x %d candidates (nnz %d), k = %d; K12 and torch give the same rank for %.3f %% of the entries, max |score '
              'difference| %.2g' % (name, n_rows, per_row, nnz, K_FACTORS, 100.0 * float((r12.view(n_rows, per_row) == rt).float().mean()),
                                    float((s12.view(n_rows, per_row) - st).abs().max())), flush=True)
        del out, s12, r12, st, rt
        times = {label: [] for label, _ in legs}
        for _ in range(repeats):
            for label, fn in legs:
                times[label].append(timed(fn))
        gather = nnz * 4.0 * K_FACTORS
        for label, _ in legs:
            t = times[label]
            extra = ''
            if label.startswith('K12'):
                tbs = gather / float(np.median(t)) / 1e9
                extra = '   gather %.2f TB/s = %.0f %% of %.1f TB/s' % (tbs, 100.0 * tbs / GATHER_TBS, GATHER_TBS)
            print('%-9s %-22s min %8.2f  median %8.2f  max %8.2f ms%s' % (name, label, min(t), float(np.median(t)), max(t), extra), flush=True)
        k12 = float(np.median(times[legs[0][0]]))
        for label, _ in legs[1:]:
            print('%-9s %s / K12 = %.2f' % (name, label, float(np.median(times[label])) / k12), flush=True)
        del U, V, user_idx, ptr, cols


if __name__ == '__main__':
    main()
