"""K25: one LMF iteration by phase (dense user, step user, dense item with sp, step item with the row loss) at the shapes of
scripts/time_als.py: the ML-10M shape (69,878 users x 10,380 items) and the Netflix shape (480,189 x 17,770), likes drawn as
synth.train_csr_shape draws them, k = 30 / 50 / 128 (tables of k + 2 columns).
The dense phase is timed beside the same quantity in torch on the same device, torch.sigmoid(X @ Y.T) @ Y in row chunks whose score
block stays under CHUNK_BYTES; the two legs alternate in this one process, medians of `repeats` passes (3) after a warm-up of each.
The dense kernel's rate is 4 n_x n_y K flop per call over its time, beside the 157 TF fp32-matrix peak.
python scripts/time_lmf.py [ml10m|netflix|both] [repeats] [k ...]"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'top-k-rec_amd'), os.path.join(ROOT, 'scripts')]
import numpy as np
import torch

import synth
import tkr_hip
from time_als import SHAPES, timed, transpose_csr

PEAK = 157e12
CHUNK_BYTES = 2 << 30
ALPHA, LAM, LR = 20.0, 0.6, 1.0


def show(tag, ms):
    print('%-64s min %9.2f  median %9.2f  max %9.2f ms' % (tag, min(ms), float(np.median(ms)), max(ms)), flush=True)
    return float(np.median(ms))


def torch_dense(X, Y, out):
    rows = max(1, CHUNK_BYTES // (4 * Y.shape[0]))
    for first in range(0, X.shape[0], rows):
        torch.matmul(torch.sigmoid(X[first:first + rows] @ Y.T), Y, out=out[first:first + rows])
    return out


def main():
    args = sys.argv[1:]
    which = args[0] if args else 'both'
    repeats = int(args[1]) if len(args) > 1 else 3
    ks = [int(x) for x in args[2:]] or [30, 50, 128]
    if not torch.cuda.is_available():
        raise SystemExit('time_lmf.py measures on the GPU; none is visible')
    dev = torch.device('cuda', 0)
    for name, (n_users, n_items) in SHAPES.items():
        if which not in ('both', name):
            continue
        row_ptr, pos, _, _ = synth.train_csr_shape(n_users, n_items)
        up, uc = row_ptr.astype(np.int64), np.ascontiguousarray(pos, dtype=np.int32)
        ip, ic = transpose_csr(up, uc, n_items)
        print('%s: %d users x %d items, %d likes, most likes of a user %d, of an item %d' % (name, n_users, n_items, len(uc), np.diff(up).max(), np.diff(ip).max()),
              flush=True)
        d = lambda a: torch.from_numpy(a).to(dev)
        upd, ucd, ipd, icd = d(up), d(uc), d(ip), d(ic)
        for k in ks:
            K = k + 2
            g = torch.Generator(device=dev)
            g.manual_seed(25)
            Xa = torch.randn((n_users, K), device=dev, generator=g) * 0.1
            Ya = torch.randn((n_items, K), device=dev, generator=g) * 0.1
            Xa[:, k + 1] = 1
            Ya[:, k] = 1
            Hx, Hy = torch.ones_like(Xa), torch.ones_like(Ya)
            ws = tkr_hip.workspace_room(None, max(tkr_hip.lmf_workspace_bytes(n_users, k, n_items), tkr_hip.lmf_workspace_bytes(n_items, k, n_users)), dev)
            Du, Di, Tu, Ti = torch.empty_like(Xa), torch.empty_like(Ya), torch.empty_like(Xa), torch.empty_like(Ya)
            words = []
            phases = [
                ('dense user', lambda: tkr_hip.lmf_dense_rows(Xa, Ya, workspace=ws, out=Du)),
                ('dense user, torch', lambda: torch_dense(Xa, Ya, Tu)),
                ('step user', lambda: words.append(tkr_hip.lmf_step_rows(Ya, Du, upd, ucd, Xa, Hx, fixed=k + 1, alpha=ALPHA, lam=LAM, lr=LR, workspace=ws, check=False)[1])),
                ('dense item (with sp)', lambda: tkr_hip.lmf_dense_rows(Ya, Xa, want_loss=True, workspace=ws, out=Di)),
                ('dense item, torch', lambda: torch_dense(Ya, Xa, Ti)),
                ('step item (with the row loss)', lambda: words.append(tkr_hip.lmf_step_rows(Xa, Di, ipd, icd, Ya, Hy, fixed=k, alpha=ALPHA, lam=LAM, lr=LR, want_loss=True,
                                                                                             workspace=ws, check=False)[1])),
            ]
            times = {label: [] for label, _ in phases}
            for round_ in range(repeats + 1):                     # round 0 warms every leg up; the legs alternate within a round
                for label, fn in phases:
                    t = timed(fn)
                    if round_:
                        times[label].append(t)
            assert all(int(w) == -1 for w in torch.cat(words).cpu().numpy())
            print('%s k %-4d max |D - torch| / max |torch|: users %.3g, items %.3g' % (name, k, float((Du - Tu).abs().max() / Tu.abs().max()),
                                                                                      float((Di - Ti).abs().max() / Ti.abs().max())), flush=True)
            med = {label: show('%s k %-4d %s' % (name, k, label), times[label]) for label, _ in phases}
            for side, n_x, n_y in (('user', n_users, n_items), ('item', n_items, n_users)):
                ours = med['dense %s' % side if side == 'user' else 'dense item (with sp)']
                flop = 4.0 * n_x * n_y * K
                print('%s k %-4d dense %s: %.1f TF = %.1f %% of the %.0f TF fp32-matrix peak; torch / kernel = %.2f' %
                      (name, k, side, flop / ours / 1e9, 100 * flop / (ours * 1e-3) / PEAK, PEAK / 1e12, med['dense %s, torch' % side] / ours), flush=True)
            print('%s k %-4d one iteration (the four phases): %.2f ms' % (name, k, med['dense user'] + med['step user'] + med['dense item (with sp)']
                                                                         + med['step item (with the row loss)']), flush=True)
            del Xa, Ya, Hx, Hy, Du, Di, Tu, Ti, ws


if __name__ == '__main__':
    main()
