"""K20 (one WMF iteration: tkr_als_gram + tkr_als_solve_rows for the users, then for the items) at the ML-10M shape (69,878 users x
10,380 items) and the Netflix shape (480,189 x 17,770), likes drawn as synth.train_csr_shape draws them, k = 50 and 128, beside the same
step in torch on the same device:
  legs   K20 iteration      als.half_step twice, as als.WMF.train runs them (the loss rows of the item step included)
         torch bmm+cholesky per block of rows (sorted by length, a block's padded gather held under 1 GiB, rows longer than 65,536 likes
                            in segments of that many): index_select of the likes' rows -> bmm for the per-row normal matrices ->
                            torch.linalg.cholesky -> torch.cholesky_solve
  split  of the K20 iteration, per half-step: the shared Gram; the solve with the heavy rows (tkr_hip.ALS_HEAVY_FROM likes or more)
         shared between workgroups, as it runs; the same solve with every row summing its own likes (heavy_from = ALS_NO_HEAVY) --
         the difference is what the heavy rows' launch buys
python scripts/time_als.py [ml10m|netflix|both] [repeats] [k ...]
Warm-up of every leg, then `repeats` rounds that alternate the legs in this one process; each pass is timed by a pair of device events.
The two legs' tables are compared first (max |difference| relative to the largest entry)."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'top-k-rec_amd')]
import numpy as np
import torch

import als
import synth
import tkr_hip

SHAPES = {'ml10m': (69878, 10380), 'netflix': (480189, 17770)}
A, B, LU, LV = 1.0, 0.01, 0.01, 0.01
PAD_BYTES = 1 << 30
SEGMENT = 1 << 16


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def transpose_csr(ptr, cols, n_cols):
    rows = np.repeat(np.arange(len(ptr) - 1, dtype=np.int64), np.diff(ptr))
    order = np.argsort(cols, kind='stable')
    tptr = np.zeros(n_cols + 1, dtype=np.int64)
    np.cumsum(np.bincount(cols, minlength=n_cols), out=tptr[1:])
    return tptr, rows[order].astype(np.int32)


def torch_blocks(ptr, k):
    """rows with likes, longest first, cut into blocks whose padded gather [rows, longest, k] stays under PAD_BYTES"""
    lens = np.diff(ptr)
    order = np.argsort(-lens, kind='stable')
    order = order[lens[order] > 0]
    blocks, at = [], 0
    while at < len(order):
        h = int(lens[order[at]])
        n = max(1, min(len(order) - at, PAD_BYTES // (min(h, SEGMENT) * k * 4), 65536))
        blocks.append((order[at:at + n].copy(), h))
        at += n
    return blocks


def torch_half_step(X, Y, ptr, cols, rated, blocks, ridge_in_G, ridge):
    k = Y.shape[1]
    Yr = Y.index_select(0, rated)
    eye = torch.eye(k, device=Y.device)
    G = B * (Yr.T @ Yr) + ridge_in_G * eye
    for rows, h in blocks:
        lo = ptr[rows]
        n = ptr[rows + 1] - lo
        M = (G + ridge * eye).repeat(len(rows), 1, 1)
        rhs = torch.zeros((len(rows), k), device=Y.device)
        for s0 in range(0, h, SEGMENT):                             # a very long row goes through the bmm in segments of its likes
            at = torch.arange(s0, min(h, s0 + SEGMENT), device=Y.device).unsqueeze(0)
            valid = at < n.unsqueeze(1)
            idx = cols[(lo.unsqueeze(1) + at).clamp(max=cols.numel() - 1)].long()
            P = Y.index_select(0, idx.reshape(-1)).view(len(rows), at.shape[1], k) * valid.unsqueeze(2)
            M += (A - B) * torch.bmm(P.transpose(1, 2), P)
            rhs += A * P.sum(dim=1)
            del P, idx
        X[rows] = torch.cholesky_solve(rhs.unsqueeze(2), torch.linalg.cholesky(M)).squeeze(2)
        del M


def main():
    args = sys.argv[1:]
    which = args[0] if args else 'both'
    repeats = int(args[1]) if len(args) > 1 else 3
    ks = [int(x) for x in args[2:]] or [50, 128]
    if not torch.cuda.is_available():
        raise SystemExit('time_als.py measures on the GPU; none is visible')
    dev = torch.device('cuda', 0)
    for name, (n_users, n_items) in SHAPES.items():
        if which not in ('both', name):
            continue
        row_ptr, pos, _, _ = synth.train_csr_shape(n_users, n_items)
        up, uc = row_ptr.astype(np.int64), np.ascontiguousarray(pos, dtype=np.int32)
        ip, ic = transpose_csr(up, uc, n_items)
        u_rated, i_rated = np.flatnonzero(np.diff(up) > 0).astype(np.int32), np.flatnonzero(np.diff(ip) > 0).astype(np.int32)
        heavy = [(int((np.diff(p) >= tkr_hip.ALS_HEAVY_FROM).sum()), tkr_hip.als_heavy_slabs(p, tkr_hip.ALS_HEAVY_FROM)) for p in (up, ip)]
        print('%s: %d users x %d items, %d likes; longest user row %d, longest item row %d; heavy rows (>= %d likes): users %d (%d slabs), '
              'items %d (%d slabs)' % (name, n_users, n_items, len(uc), int(np.diff(up).max()), int(np.diff(ip).max()), tkr_hip.ALS_HEAVY_FROM,
                                       heavy[0][0], heavy[0][1], heavy[1][0], heavy[1][1]), flush=True)
        d = lambda a: torch.from_numpy(a).to(dev)
        upd, ucd, ipd, icd, urd, ird = d(up), d(uc), d(ip), d(ic), d(u_rated), d(i_rated)
        for k in ks:
            g = torch.Generator(device=dev)
            g.manual_seed(20)
            U0 = torch.rand((n_users, k), device=dev, generator=g)
            V0 = torch.rand((n_items, k), device=dev, generator=g)
            ublocks = [(d(r), h) for r, h in torch_blocks(up, k)]
            iblocks = [(d(r), h) for r, h in torch_blocks(ip, k)]
            w = als.Work()
            state = {}

            def k20():
                U, V = U0.clone(), V0.clone()
                _, su = als.half_step(U, V, upd, ucd, ird, w=w, ridge_in_G=LU, ridge=0.0, a=A, b=B)
                loss, sv = als.half_step(V, U, ipd, icd, urd, w=w, ridge_in_G=0.0, ridge=LV, a=A, b=B, want_loss=True)
                state['k20'] = (U, V, su, sv)

            def torch_leg():
                U, V = U0.clone(), V0.clone()
                torch_half_step(U, V, upd, ucd, ird.long(), ublocks, LU, 0.0)
                torch_half_step(V, U, ipd, icd, urd.long(), iblocks, 0.0, LV)
                state['torch'] = (U, V)

            legs = [('K20 iteration', k20), ('torch bmm+cholesky', torch_leg)]
            k20()
            torch.cuda.synchronize()
            U, V, su, sv = state['k20']
            als.check_status(torch.cat([su, sv]).cpu().numpy(), ('the user step', 'the item step'))
            try:
                torch_leg()
                torch.cuda.synchronize()
                Ut, Vt = state['torch']
                print('%s k %d: K20 against torch: max |dU| / max |U| = %.3g, max |dV| / max |V| = %.3g' %
                      (name, k, float((U - Ut).abs().max() / Ut.abs().max()), float((V - Vt).abs().max() / Vt.abs().max())), flush=True)
            except RuntimeError as e:                                # (torch._C._LinAlgError is one)
                print('%s k %d: the torch leg did not finish and is left out: %s' % (name, k, str(e).split(chr(10))[0]), flush=True)
                legs = legs[:1]
            times = {label: [] for label, _ in legs}
            for _ in range(repeats):
                for label, fn in legs:
                    times[label].append(timed(fn))
            for label, _ in legs:
                ms = times[label]
                print('%s k %-4d %-20s min %9.2f  median %9.2f  max %9.2f ms' % (name, k, label, min(ms), float(np.median(ms)), max(ms)), flush=True)
            if len(legs) == 2:
                print('%s k %-4d torch / K20 = %.2f' % (name, k, float(np.median(times['torch bmm+cholesky'])) / float(np.median(times['K20 iteration']))),
                      flush=True)
            G = torch.empty((k, k), device=dev)
            for side, X, Y, ptr, cols, rated, rg, rs, hs in (('users', U, V0, upd, ucd, ird, LU, 0.0, heavy[0][1]), ('items', V, U, ipd, icd, urd, 0.0, LV, heavy[1][1])):
                X = X.clone()
                solve = lambda hf: tkr_hip.als_solve_rows(Y, G, ptr, cols, X, w_like=A - B, w_rhs=A, ridge=rs, heavy_from=hf, want_loss=side == 'items',
                                                          workspace=w.workspace, heavy_slabs=hs, check=False)
                parts = [('gram', lambda: tkr_hip.als_gram(Y, rated, scale=B, ridge=rg, workspace=w.workspace, out=G, check=False)),
                         ('solve, heavy rows shared', lambda: solve(tkr_hip.ALS_HEAVY_FROM)),
                         ('solve, every row alone', lambda: solve(tkr_hip.ALS_NO_HEAVY))]
                for label, fn in parts:
                    fn()
                    ms = [timed(fn) for _ in range(repeats)]
                    print('%s k %-4d split %-6s %-26s median %9.2f ms' % (name, k, side, label, float(np.median(ms))), flush=True)
            del ublocks, iblocks, U0, V0, state, w


if __name__ == '__main__':
    main()
