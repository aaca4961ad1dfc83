"""K19 (tkr_nearest_anchors: the e nearest anchors of every list entry) at the ML-10M shape (69,878 users x 10,380 items, k = 128), e = 3,
lists of t = 30 and of t = 100, the anchors of a row being a training history drawn as synth.train_csr_shape draws them (lognormal
lengths, items by popularity, repeats dropped: 190 draws leave ML-10M's mean of about 140 likes), beside what a user can do without it on the same device:
  legs   K19 nearest        tkr_hip.nearest_anchors alone, on a prepared S
         K19 explain        explain.explain: that and the gather that turns positions into columns
         torch bmm+topk     index_select of the lists' rows and of the (padded) histories' rows of S -> bmm [rows, t, longest] -> masks ->
                            topk, in blocks of rows
python scripts/time_explain.py [30|100|both] [repeats]
Warm-up of every leg, then `repeats` rounds that alternate the legs in this one process; each pass is timed by a pair of device events.
Prints min / median / max per leg, K19's share of the gather roofline (every list row and every anchor row of S once: (rows * t +
anchors) * 4 k bytes, at the 8.6 TB/s measured for random rows of an Infinity-Cache-resident table, as DESIGN.md section 4 K12) and the
ratio of the medians.  The two results are compared first: the nearest anchor must be the same for every entry outside those whose
best e + 1 similarities hold two within 2^-20 of each other (the torch leg sums in BLAS order, K19 in the library's chain order)."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'top-k-rec_amd')]
import numpy as np
import torch

import diversity
import explain
import synth
import tkr_hip

GATHER_TBS = 8.6
N_USERS, N_COLS, K_FACTORS, E, MEAN_DRAWS = 69878, 10380, 128, 3, 190.0
GAP = 2.0 ** -20
BLOCK = {30: 2048, 100: 1024}                                       # rows per block of the torch leg: the padded histories' rows are block * longest * 4 k bytes


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def torch_nearest(S, ids, ptr, cols, e, block):
    """the same with torch alone -> (pos int64 [n, t, e], sim fp32 [n, t, e], ambiguous bool [n, t]); every list entry valid"""
    n, t = ids.shape
    lens = ptr[1:] - ptr[:-1]
    pos = torch.full((n, t, e), -1, dtype=torch.int64, device=S.device)
    sim = torch.full((n, t, e), float('-inf'), dtype=torch.float32, device=S.device)
    amb = torch.zeros((n, t), dtype=torch.bool, device=S.device)
    for lo in range(0, n, block):
        hi = min(n, lo + block)
        h = int(lens[lo:hi].max())
        if h == 0:
            continue
        at = torch.arange(h, device=S.device).unsqueeze(0)
        valid = at < lens[lo:hi].unsqueeze(1)
        a = torch.where(valid, cols[(ptr[lo:hi].unsqueeze(1) + at).clamp(max=cols.numel() - 1)], torch.zeros_like(at, dtype=cols.dtype))
        L = S.index_select(0, ids[lo:hi].reshape(-1).long()).view(hi - lo, t, -1)
        A = S.index_select(0, a.reshape(-1).long()).view(hi - lo, h, -1)
        G = torch.bmm(L, A.transpose(1, 2))
        G.masked_fill_(~valid.unsqueeze(1) | (a.unsqueeze(1) == ids[lo:hi].unsqueeze(2)), float('-inf'))
        top = G.topk(min(e + 1, h), dim=2)
        m = min(e, h)
        sim[lo:hi, :, :m] = top.values[:, :, :m]
        pos[lo:hi, :, :m] = torch.where(top.values[:, :, :m] > float('-inf'), top.indices[:, :, :m], torch.full_like(top.indices[:, :, :m], -1))
        gaps = top.values[:, :, :-1] - top.values[:, :, 1:]         # (-inf) - (-inf) is nan: not <= GAP
        amb[lo:hi] = (gaps <= GAP).any(dim=2)
    return pos, sim, amb


def main():
    which = sys.argv[1] if len(sys.argv) > 1 else 'both'
    repeats = int(sys.argv[2]) if len(sys.argv) > 2 else 5
    if not torch.cuda.is_available():
        raise SystemExit('time_explain.py measures on the GPU; none is visible')
    dev = torch.device('cuda', 0)
    g = torch.Generator(device=dev)
    g.manual_seed(19)
    U = (torch.randn((N_USERS, K_FACTORS), device=dev, generator=g) * 0.01 * 1e6).round() / 1e6
    V = (torch.randn((N_COLS, K_FACTORS), device=dev, generator=g) * 0.01 * 1e6).round() / 1e6
    row_ptr, _, cols_sorted, _ = synth.train_csr_shape(N_USERS, N_COLS, mean_pos=MEAN_DRAWS)
    ptr = torch.from_numpy(row_ptr.astype(np.int64)).to(dev)
    cols = torch.from_numpy(np.ascontiguousarray(cols_sorted, dtype=np.int32)).to(dev)
    lens = np.diff(row_ptr)
    print('%d rows, %d items, k = %d, e = %d; %d anchors: mean %.1f, median %d, longest %d per row' %
          (N_USERS, N_COLS, K_FACTORS, E, int(row_ptr[-1]), lens.mean(), int(np.median(lens)), int(lens.max())), flush=True)
    S = diversity.similarity_table(V, 'cosine')
    wrong = 0
    for t in (30, 100):
        if which not in ('both', str(t)):
            continue
        ids = tkr_hip.score_topk(U, V, t)
        legs = [('K19 nearest', lambda: tkr_hip.nearest_anchors(S, ids, ptr, cols, E)),
                ('K19 explain', lambda: explain.explain(S, ids, ptr, cols, E)),
                ('torch bmm+topk', lambda: torch_nearest(S, ids, ptr, cols, E, BLOCK[t]))]
        out = [fn() for _, fn in legs for _ in range(2)]            # warm-up: code objects, the allocator's blocks
        torch.cuda.synchronize()
        mine, (theirs, _, amb) = out[1][0][:, :, 0].long(), out[5]
        differ = mine != theirs[:, :, 0]
        bad = int((differ & ~amb).sum())
        wrong += bad
        print('t = %d: ambiguous entries %d of %d, entries whose nearest anchor differs %d, of them not ambiguous %d' %
              (t, int(amb.sum()), amb.numel(), int(differ.sum()), bad), flush=True)
        del out, mine, theirs, amb, differ
        times = {label: [] for label, _ in legs}
        for _ in range(repeats):
            for label, fn in legs:
                times[label].append(timed(fn))
        gather = (N_USERS * t + int(row_ptr[-1])) * 4.0 * K_FACTORS
        for label, _ in legs:
            ms = times[label]
            extra = ''
            if label == 'K19 nearest':
                tbs = gather / float(np.median(ms)) / 1e9
                chains = float((lens * t).sum())
                extra = '   gather %.3f TB/s = %.1f %% of %.1f TB/s; %.2f T chain-fma/s' % (tbs, 100.0 * tbs / GATHER_TBS, GATHER_TBS,
                                                                                        chains * K_FACTORS / float(np.median(ms)) / 1e9)
            print('t %-4d %-16s min %9.2f  median %9.2f  max %9.2f ms%s' % (t, label, min(ms), float(np.median(ms)), max(ms), extra), flush=True)
        for a, b in (('torch bmm+topk', 'K19 explain'), ('torch bmm+topk', 'K19 nearest')):
            print('t %-4d %s / %s = %.2f' % (t, a, b, float(np.median(times[a])) / float(np.median(times[b]))), flush=True)
        del ids
    assert wrong == 0, '%d entries differ between K19 and the torch leg without being ambiguous' % wrong


if __name__ == '__main__':
    main()
