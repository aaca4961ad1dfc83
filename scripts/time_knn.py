"""K28 / K29: building and serving the item-neighbourhood model at the shapes of scripts/time_als.py: the ML-10M shape (69,878 users x
10,380 items) and the Netflix shape (480,189 x 17,770), likes drawn as synth.train_csr_shape draws them, N = 100 neighbours.

K28 (tkr_hip.knn_build, cosine) is timed with the default heavy_from and with no row split, beside two torch legs on the same device:
torch.sparse.mm(X^T, X) to dense, the similarity and topk in row chunks; and a dense bf16 X^T X (fp32 accumulation inside the product,
the result rounded to bf16: a yardstick for the time, not for the bits), similarity and topk, where X fits.  A torch leg that the
installed torch cannot run is reported as such.  K29 (tkr_hip.knn_score: lists of 30 and the ranks of five likes per line, the
training likes masked) is timed beside torch.sparse.mm(hist, W) with W the dense table, mask and topk in row chunks, and beside K4 + K8
(tkr_hip.score_topk, tkr_hip.like_ranks) on a k = 128 factor model of the same shape.  The legs alternate in this one process, medians
of `repeats` passes (3) after a warm-up of each.  Also printed: sum n_u^2 (the LDS adds of a build), the share of rows that were split.
python scripts/time_knn.py [ml10m|netflix|both] [repeats]"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'top-k-rec_amd'), os.path.join(ROOT, 'scripts')]
import numpy as np
import torch

import synth
import tkr_hip
from time_als import SHAPES, timed, transpose_csr
from time_lmf import CHUNK_BYTES, show

N, K, LIKES = 100, 30, 5
NO_HEAVY = 1 << 60


def torch_topn(C, norm, out_ids, out_w):
    """similarity and topk of a dense count matrix, in row chunks, the diagonal left out"""
    n = C.shape[0]
    rows = max(1, CHUNK_BYTES // (8 * n))
    for first in range(0, n, rows):
        block = C[first:first + rows].float()
        sim = block / (norm[first:first + rows, None] * norm[None, :])
        sim[torch.arange(block.shape[0], device=C.device), torch.arange(first, first + block.shape[0], device=C.device)] = 0
        w, ids = torch.topk(sim, N, dim=1)
        out_w[first:first + rows], out_ids[first:first + rows] = w, ids


def main():
    args = sys.argv[1:]
    which = args[0] if args else 'both'
    repeats = int(args[1]) if len(args) > 1 else 3
    if not torch.cuda.is_available():
        raise SystemExit('time_knn.py measures on the GPU; none is visible')
    dev = torch.device('cuda', 0)
    for name, (n_users, n_items) in SHAPES.items():
        if which not in ('both', name):
            continue
        row_ptr, _, srt, _ = synth.train_csr_shape(n_users, n_items)
        up, uc = row_ptr.astype(np.int64), np.ascontiguousarray(srt, dtype=np.int32)     # ascending inside a row
        ip, ir = transpose_csr(up, uc, n_items)
        n_u, n_i = np.diff(up), np.diff(ip)
        work = np.add.reduceat(np.r_[n_u[ir], 0], np.minimum(ip[:-1], len(ir))) * (n_i > 0)
        print('%s: %d users x %d items, %d likes, most likes of a user %d, of an item %d; sum n_u^2 = %.4g; the longest row\'s work %.4g; '
              '%.1f %% of the rows are split at heavy_from = %d' % (name, n_users, n_items, len(uc), n_u.max(), n_i.max(), float((n_u.astype(np.float64) ** 2).sum()),
                                                                  float(work.max()), 100.0 * (work > tkr_hip.KNN_HEAVY_FROM).mean(), tkr_hip.KNN_HEAVY_FROM), flush=True)
        d = lambda a: torch.from_numpy(a).to(dev)
        upd, ucd, ipd, ird = d(up), d(uc), d(ip), d(ir)
        norm64 = torch.sqrt(torch.clamp(d(n_i).double(), min=1.0))
        norm32 = norm64.float()
        table = (torch.empty((n_items, N), dtype=torch.int32, device=dev), torch.empty((n_items, N), dtype=torch.float32, device=dev))
        ws = tkr_hip.workspace_room(None, tkr_hip.knn_build_workspace_bytes(n_items), dev)
        t_ids, t_w = torch.empty((n_items, N), dtype=torch.int64, device=dev), torch.empty((n_items, N), dtype=torch.float32, device=dev)
        X = torch.sparse_csr_tensor(upd, ucd.long(), torch.ones(len(uc), dtype=torch.float32, device=dev), size=(n_users, n_items))
        Xt = torch.sparse_csr_tensor(ipd, ird.long(), torch.ones(len(uc), dtype=torch.float32, device=dev), size=(n_items, n_users))

        def sparse_leg():
            torch_topn(torch.sparse.mm(Xt, X).to_dense(), norm32, t_ids, t_w)

        Xb = None
        if 2 * n_users * n_items < 48 << 30:
            Xb = torch.zeros((n_users, n_items), dtype=torch.bfloat16, device=dev)
            Xb[torch.repeat_interleave(torch.arange(n_users, device=dev), d(n_u)), ucd.long()] = 1

        def dense_leg():
            torch_topn(Xb.T @ Xb, norm32, t_ids, t_w)

        phases = [('K28 build', lambda: tkr_hip.knn_build(upd, ucd, ipd, ird, norm64, N, workspace=ws, out=table, check=False)),
                  ('K28 build, no row split', lambda: tkr_hip.knn_build(upd, ucd, ipd, ird, norm64, N, heavy_from=NO_HEAVY, workspace=ws, out=table, check=False)),
                  ('torch sparse X^T X, similarity, topk', sparse_leg)]
        if Xb is not None:
            phases.append(('torch dense bf16 X^T X, similarity, topk', dense_leg))
        # K29: every user a line, the training likes masked, five likes per line to rank
        rng = np.random.Generator(np.random.PCG64(29))
        lp = np.arange(0, (n_users + 1) * LIKES, LIKES, dtype=np.int64)
        lc = np.sort(rng.integers(0, n_items, (n_users, LIKES)), axis=1).astype(np.int32).reshape(-1)
        lpd, lcd = d(lp), d(lc)
        mask, pitch = tkr_hip.build_rated_mask(upd, ucd, n_users, n_items)
        tkr_hip.knn_build(upd, ucd, ipd, ird, norm64, N, workspace=ws, out=table)
        W = torch.zeros((n_items, n_items), dtype=torch.float32, device=dev)
        W[torch.arange(n_items, device=dev)[:, None].expand(-1, N)[table[0] >= 0], table[0][table[0] >= 0].long()] = table[1][table[0] >= 0]
        rated = torch.zeros(0)

        def serve_torch():
            rows = max(1, CHUNK_BYTES // (8 * n_items))
            for first in range(0, n_users, rows):
                last = min(n_users, first + rows)
                lo, hi = int(up[first]), int(up[last])
                H = torch.sparse_csr_tensor(upd[first:last + 1] - lo, ucd[lo:hi].long(), torch.ones(hi - lo, dtype=torch.float32, device=dev),
                                            size=(last - first, n_items))
                S = torch.sparse.mm(H, W)
                S[torch.repeat_interleave(torch.arange(last - first, device=dev), upd[first + 1:last + 1] - upd[first:last]), ucd[lo:hi].long()] = -float('inf')
                torch.topk(S, K, dim=1)

        g = torch.Generator(device=dev)
        g.manual_seed(28)
        U = torch.randn((n_users, 128), device=dev, generator=g) * 0.1
        V = torch.randn((n_items, 128), device=dev, generator=g) * 0.1

        def serve_k4():
            tkr_hip.score_topk(U, V, K, mask=mask, mask_pitch=pitch)
            tkr_hip.like_ranks(U, V, lpd, lcd, mask=mask, mask_pitch=pitch)

        phases += [('K29 lists of 30 and ranks', lambda: tkr_hip.knn_score(upd, ucd, table[0], table[1], K, mask=mask, mask_pitch=pitch, like_ptr=lpd, like_cols=lcd)),
                   ('torch sparse hist @ W, mask, topk', serve_torch), ('K4 + K8 on a k = 128 factor model', serve_k4)]
        times, dead = {label: [] for label, _ in phases}, {}
        for round_ in range(repeats + 1):                         # round 0 warms every leg up; the legs alternate within a round
            for label, fn in phases:
                if label in dead:
                    continue
                try:
                    t = timed(fn)
                except RuntimeError as e:                          # a torch leg this torch cannot run
                    dead[label] = str(e).split('\n')[0][:160]
                    continue
                if round_:
                    times[label].append(t)
        for label, _ in phases:
            if label in dead:
                print('%s %s: not run: %s' % (name, label, dead[label]), flush=True)
            else:
                show('%s %s' % (name, label), times[label])
        del X, Xt, Xb, W, U, V, table, mask


if __name__ == '__main__':
    main()
