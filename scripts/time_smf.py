"""K27: one SMF iteration by phase (lse user, dense user, step user, lse again, dense item, step item) at the shapes of
scripts/time_als.py: the ML-10M shape (69,878 users x 10,380 items) and the Netflix shape (480,189 x 17,770), likes drawn as
synth.train_csr_shape draws them, k = 30 / 50 / 128 (tables of k + 1 columns).
Each dense pass is timed beside tkr_lmf_dense_rows on the same tables (the same MFMA work with sigma in place of exp) and beside the same
quantity in torch on the same device, torch.softmax(X @ Y.T, 1) @ Y in row chunks whose score block stays under CHUNK_BYTES (on the
item side the softmax over the users' axis: exp(S^T - off) @ X); the legs alternate in this one process, medians of `repeats` passes
(3) after a warm-up of each.  A dense kernel's rate is 4 n_x n_y K flop per call over its time, the lse pass's 2 n_x n_y K, beside
the 157 TF fp32-matrix peak.
python scripts/time_smf.py [ml10m|netflix|both] [repeats] [k ...]"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'top-k-rec_amd'), os.path.join(ROOT, 'scripts')]
import numpy as np
import torch

import smf
import synth
import tkr_hip
from time_als import SHAPES, timed, transpose_csr
from time_lmf import CHUNK_BYTES, PEAK, show

LAM, LR = 0.01, 1e-30             # a step too small to move a value: every pass of every leg sees the same tables


def torch_user(X, Y, out):
    rows = max(1, CHUNK_BYTES // (4 * Y.shape[0]))
    for first in range(0, X.shape[0], rows):
        torch.matmul(torch.softmax(X[first:first + rows] @ Y.T, 1), Y, out=out[first:first + rows])
    return out


def torch_item(Y, X, off, out):
    """D[i] = sum_u exp(s_ui - off[u]) X[u]: the users are the columns, so the chunks are over the items and off is a row vector"""
    rows = max(1, CHUNK_BYTES // (4 * X.shape[0]))
    for first in range(0, Y.shape[0], rows):
        torch.matmul(torch.exp(Y[first:first + rows] @ X.T - off), X, out=out[first:first + rows])
    return out


def main():
    args = sys.argv[1:]
    which = args[0] if args else 'both'
    repeats = int(args[1]) if len(args) > 1 else 3
    ks = [int(x) for x in args[2:]] or [30, 50, 128]
    if not torch.cuda.is_available():
        raise SystemExit('time_smf.py measures on the GPU; none is visible')
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
        log_n = torch.log((upd[1:] - upd[:-1]).float())
        for k in ks:
            K = k + 1
            g = torch.Generator(device=dev)
            g.manual_seed(27)
            Xa = torch.randn((n_users, K), device=dev, generator=g) * 0.1
            Ya = torch.randn((n_items, K), device=dev, generator=g) * 0.1
            Xa[:, k] = 1
            Hx, Hy = torch.ones_like(Xa), torch.ones_like(Ya)
            Xl = torch.cat([Xa, torch.ones_like(Xa[:, :1])], 1).contiguous()       # the same tables one column wider: K25's k + 2
            Yl = torch.cat([Ya, torch.ones_like(Ya[:, :1])], 1).contiguous()
            ws = tkr_hip.workspace_room(None, max(tkr_hip.lmf_workspace_bytes(n_users, k, n_items), tkr_hip.lmf_workspace_bytes(n_items, k, n_users),
                                                  tkr_hip.smf_workspace_bytes(n_users, k, n_items), tkr_hip.smf_workspace_bytes(n_items, k, n_users)), dev)
            Du, Di, Tu, Ti = torch.empty_like(Xa), torch.empty_like(Ya), torch.empty_like(Xa), torch.empty_like(Ya)
            Lu, Li = torch.empty_like(Xl), torch.empty_like(Yl)
            lse = torch.empty(n_users, dtype=torch.float32, device=dev)
            off = tkr_hip.smf_lse_rows(Xa, Ya, workspace=ws) - log_n             # for the item side's legs: fixed, the tables do not move below
            words = []
            hyper = dict(lam=LAM, lr=LR, workspace=ws, check=False)
            phases = [
                ('lse user', lambda: tkr_hip.smf_lse_rows(Xa, Ya, workspace=ws, out=lse)),
                ('dense user', lambda: tkr_hip.smf_dense_rows(Xa, Ya, row_off=lse, workspace=ws, out=Du)),
                ('dense user, K25 sigma', lambda: tkr_hip.lmf_dense_rows(Xl, Yl, workspace=ws, out=Lu)),
                ('dense user, torch', lambda: torch_user(Xa, Ya, Tu)),
                ('step user (with the row loss)', lambda: words.append(tkr_hip.smf_step_rows(Ya, Du, upd, ucd, Xa, Hx, fixed=k, scale_by_likes=True, want_loss=True,
                                                                                             **hyper)[1])),
                ('dense item', lambda: tkr_hip.smf_dense_rows(Ya, Xa, col_off=off, workspace=ws, out=Di)),
                ('dense item, K25 sigma', lambda: tkr_hip.lmf_dense_rows(Yl, Xl, workspace=ws, out=Li)),
                ('dense item, torch', lambda: torch_item(Ya, Xa, off, Ti)),
                ('step item', lambda: words.append(tkr_hip.smf_step_rows(Xa, Di, ipd, icd, Ya, Hy, fixed=-1, scale_by_likes=False, **hyper)[1])),
            ]
            work = {}

            def iteration():
                _, rows, su = smf.user_step(Xa, Hx, Ya, upd, ucd, lam=LAM, lr=LR, want_loss=True, work=work)
                words.extend([su, smf.item_step(Ya, Hy, Xa, log_n, ipd, icd, lam=LAM, lr=LR, work=work)])
            phases.append(('one iteration (smf.user_step + smf.item_step)', iteration))
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
            flop = 2.0 * n_users * n_items * K
            print('%s k %-4d lse user: %.1f TF = %.1f %% of the %.0f TF fp32-matrix peak' % (name, k, flop / med['lse user'] / 1e9,
                                                                                             100 * flop / (med['lse user'] * 1e-3) / PEAK, PEAK / 1e12), flush=True)
            for side in ('user', 'item'):
                ours = med['dense %s' % side]
                print('%s k %-4d dense %s: %.1f TF = %.1f %% of the %.0f TF fp32-matrix peak; K25 sigma / kernel = %.2f; torch / kernel = %.2f' %
                      (name, k, side, 2 * flop / ours / 1e9, 100 * 2 * flop / (ours * 1e-3) / PEAK, PEAK / 1e12, med['dense %s, K25 sigma' % side] / ours,
                       med['dense %s, torch' % side] / ours), flush=True)
            parts = 2 * med['lse user'] + med['dense user'] + med['step user (with the row loss)'] + med['dense item'] + med['step item']
            print('%s k %-4d one iteration: %.2f ms measured whole, %.2f ms as the sum of its six kernel phases (lse twice)' %
                  (name, k, med['one iteration (smf.user_step + smf.item_step)'], parts), flush=True)
            del Xa, Ya, Xl, Yl, Hx, Hy, Du, Di, Tu, Ti, Lu, Li, ws, work


if __name__ == '__main__':
    main()
