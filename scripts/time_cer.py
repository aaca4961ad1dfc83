"""K21 (one CER iteration, als.CER.train's loop body) at the ML-10M shape (69,878 users x 10,380 items), likes drawn as
synth.train_csr_shape draws them and then every fifth item's likes removed (those items are cold), dense standard-normal features of
d = 1,024 and 20,000, k = 50 and 128:
  phases  Fe = F E (fp64 product, rounded once)                                          library
          the user half-step (K20: tkr_als_gram + tkr_als_solve_rows)
          the item half-step (K21: tkr_als_gram + tkr_als_solve_rows_prior, the loss rows included), and its parts, each a call of
          its own on a CSR cut for it: the rows with likes alone (the factor launch rides along, no cold row), the factor with ONE
          cold row, all cold rows alone (the factor rides along)
          the E-step  E = FF^-1 (lv F^T V)  (fp64, cholesky_solve)                        library
          once per train(): FF = lv F^T F + le I and its Cholesky factor (fp64)           library
  legs    of the item half-step: K21, and torch on the same device built as scripts/time_als.py builds K20's: index_select -> bmm ->
          linalg.cholesky -> cholesky_solve per block of rows, the prior added to the right-hand side, the cold rows by ONE
          cholesky_solve with n_cold right-hand sides.  The two legs' tables are compared first.
python scripts/time_cer.py [repeats] [k ...]      (TIME_CER_D=1024,20000 picks the feature widths)
Warm-up of every leg, then `repeats` rounds that alternate the legs in this one process; each pass is timed by a pair of device events;
medians with min and max beside them."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'top-k-rec_amd')]
import numpy as np
import torch

import als
import synth
import tkr_hip
from time_als import SHAPES, timed, torch_blocks, transpose_csr

A, B, LU, LV, LE = 1.0, 0.01, 0.01, 10.0, 10e3
SEGMENT = 1 << 16


def csr_of(rows_of_entries, cols, n_rows):
    order = np.argsort(rows_of_entries, kind='stable')
    ptr = np.zeros(n_rows + 1, dtype=np.int64)
    np.cumsum(np.bincount(rows_of_entries, minlength=n_rows), out=ptr[1:])
    return ptr, np.ascontiguousarray(cols[order], dtype=np.int32)


def torch_item_step(X, Y, ptr, cols, rated, blocks, cold, prior):
    """time_als.torch_half_step for the items, with the prior: G + lv I per block, rhs += lv prior; the cold rows in one solve"""
    k = Y.shape[1]
    Yr = Y.index_select(0, rated)
    eye = torch.eye(k, device=Y.device)
    G = B * (Yr.T @ Yr)
    for rows, h in blocks:
        lo = ptr[rows]
        n = ptr[rows + 1] - lo
        M = (G + LV * eye).repeat(len(rows), 1, 1)
        rhs = LV * prior[rows]
        for s0 in range(0, h, SEGMENT):
            at = torch.arange(s0, min(h, s0 + SEGMENT), device=Y.device).unsqueeze(0)
            valid = at < n.unsqueeze(1)
            idx = cols[(lo.unsqueeze(1) + at).clamp(max=cols.numel() - 1)].long()
            P = Y.index_select(0, idx.reshape(-1)).view(len(rows), at.shape[1], k) * valid.unsqueeze(2)
            M += (A - B) * torch.bmm(P.transpose(1, 2), P)
            rhs += A * P.sum(dim=1)
            del P, idx
        X[rows] = torch.cholesky_solve(rhs.unsqueeze(2), torch.linalg.cholesky(M)).squeeze(2)
        del M
    X[cold] = torch.cholesky_solve(LV * prior[cold].T, torch.linalg.cholesky(G + LV * eye)).T


def report(label, ms):
    print('%-58s min %9.3f  median %9.3f  max %9.3f ms' % (label, min(ms), float(np.median(ms)), max(ms)), flush=True)
    return float(np.median(ms))


def main():
    args = sys.argv[1:]
    repeats = int(args[0]) if args else 3
    ks = [int(x) for x in args[1:]] or [50, 128]
    ds = [int(x) for x in os.environ.get('TIME_CER_D', '1024,20000').split(',')]
    if not torch.cuda.is_available():
        raise SystemExit('time_cer.py measures on the GPU; none is visible')
    dev = torch.device('cuda', 0)
    n_users, n_items = SHAPES['ml10m']
    row_ptr, pos, _, _ = synth.train_csr_shape(n_users, n_items)
    users = np.repeat(np.arange(n_users, dtype=np.int64), np.diff(row_ptr))
    items = np.asarray(pos, dtype=np.int64)
    keep = items % 5 != 0                                             # every fifth item loses its likes
    users, items = users[keep], items[keep]
    up, uc = csr_of(users, items, n_users)
    ip, ic = csr_of(items, users, n_items)
    u_rated, i_rated = np.flatnonzero(np.diff(up) > 0).astype(np.int32), np.flatnonzero(np.diff(ip) > 0).astype(np.int32)
    cold = np.flatnonzero(np.diff(ip) == 0)
    warm = np.flatnonzero(np.diff(ip) > 0)
    print('ml10m: %d users x %d items, %d likes; %d items with likes, %d cold; heavy item rows (>= %d likes): %d'
          % (n_users, n_items, len(uc), len(warm), len(cold), tkr_hip.ALS_HEAVY_FROM, int((np.diff(ip) >= tkr_hip.ALS_HEAVY_FROM).sum())), flush=True)
    d_ = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    upd, ucd, ipd, icd, urd, ird, coldd, warmd = d_(up), d_(uc), d_(ip), d_(ic), d_(u_rated), d_(i_rated), d_(cold), d_(warm)
    # the CSRs of the parts: the warm rows alone (in their order), n_cold rows without likes, one row without likes
    wp = np.zeros(len(warm) + 1, dtype=np.int64)
    np.cumsum(np.diff(ip)[warm], out=wp[1:])
    warm_slabs = tkr_hip.als_heavy_slabs(wp, tkr_hip.ALS_HEAVY_FROM)
    wpd, cpd, onepd = d_(wp), torch.zeros(len(cold) + 1, dtype=torch.int64, device=dev), torch.zeros(2, dtype=torch.int64, device=dev)
    for dd in ds:
        g = torch.Generator(device=dev)
        g.manual_seed(21)
        F = torch.randn((n_items, dd), device=dev, generator=g).double()
        once = []
        for _ in range(repeats + 1):
            def ff():
                FF = torch.addmm(torch.eye(dd, dtype=torch.float64, device=dev), F.t(), F, beta=LE, alpha=LV)
                ff.chol = torch.linalg.cholesky(FF)
            once.append(timed(ff))
        report('d %-5d once per train(): FF and its Cholesky factor' % dd, once[1:])
        chol = ff.chol
        for k in ks:
            U0 = torch.rand((n_users, k), device=dev, generator=g)
            V0 = torch.rand((n_items, k), device=dev, generator=g)
            E0 = torch.randn((dd, k), device=dev, generator=g) / dd ** 0.5
            w = als.Work()
            iblocks = [(d_(r), h) for r, h in torch_blocks(ip, k)]
            st = {}
            phases = {
                'Fe = F E': lambda: st.__setitem__('Fe', (F @ E0.double()).float()),
                'user half-step (K20)': lambda: st.__setitem__('su', als.half_step(st['U'], V0, upd, ucd, ird, w=w, ridge_in_G=LU, ridge=0.0, a=A, b=B)[1]),
                'item half-step (K21)': lambda: st.__setitem__('sv', als.half_step(st['V'], st['U'], ipd, icd, urd, w=w, ridge_in_G=0.0, ridge=LV, a=A, b=B,
                                                                                    want_loss=True, prior=st['Fe'], w_prior=LV)[1]),
                'E-step': lambda: st.__setitem__('E', torch.cholesky_solve(LV * (F.t() @ st['V'].double()), chol).float()),
            }
            st['U'], st['V'] = U0.clone(), V0.clone()
            for fn in phases.values():                                # warm-up, in the order of an iteration
                fn()
            torch.cuda.synchronize()
            als.check_status(torch.cat([st['su'], st['sv']]).cpu().numpy(), ('the user step', 'the item step'))
            Vk = st['V'].clone()
            Vt = V0.clone()
            torch_leg = lambda: torch_item_step(Vt, st['U'], ipd, icd, urd.long(), iblocks, coldd, st['Fe'])
            torch_leg()
            torch.cuda.synchronize()
            scale = float(Vt.abs().max())
            print('d %-5d k %-4d K21 against torch, item table: max |dV| / max |V| = %.3g (rows with likes %.3g, cold rows %.3g)'
                  % (dd, k, float((Vk - Vt).abs().max()) / scale, float((Vk[warmd] - Vt[warmd]).abs().max()) / scale,
                     float((Vk[coldd] - Vt[coldd]).abs().max()) / scale), flush=True)
            # the parts of the item half-step, each on a CSR of its own (the Gram is in w.G from the warm-up)
            Xw, Pw = st['V'][warmd].contiguous(), st['Fe'][warmd].contiguous()
            Xc, Pc = st['V'][coldd].contiguous(), st['Fe'][coldd].contiguous()
            solve = lambda X, P, ptr, cols: tkr_hip.als_solve_rows_prior(st['U'], w.G, ptr, cols, X, P, w_like=A - B, w_rhs=A, w_prior=LV, ridge=LV,
                                                                         want_loss=True, heavy_slabs=warm_slabs, check=False)
            none = torch.zeros(0, dtype=torch.int32, device=dev)
            parts = {
                'item: gram': lambda: tkr_hip.als_gram(st['U'], urd, scale=B, ridge=0.0, workspace=w.workspace, out=w.G, check=False),
                'item: rows with likes alone (+ the factor launch)': lambda: solve(Xw, Pw, wpd, icd),
                'item: the factor + ONE cold row': lambda: solve(Xc[:1], Pc[:1], onepd, none),
                'item: all %d cold rows alone (+ the factor launch)' % len(cold): lambda: solve(Xc, Pc, cpd, none),
                'item half-step, torch bmm+cholesky': torch_leg,
            }
            legs = dict(phases)
            legs.update(parts)
            for fn in parts.values():
                fn()
            times = {label: [] for label in legs}
            for _ in range(repeats):
                for label, fn in legs.items():
                    times[label].append(timed(fn))
            med = {label: report('d %-5d k %-4d %s' % (dd, k, label), ms) for label, ms in times.items()}
            total = sum(med[label] for label in phases)
            print('d %-5d k %-4d one iteration = %.3f ms: Fe %.1f %%, users %.1f %%, items %.1f %%, E-step %.1f %%; torch / K21 on the item half-step = %.2f'
                  % (dd, k, total, 100 * med['Fe = F E'] / total, 100 * med['user half-step (K20)'] / total, 100 * med['item half-step (K21)'] / total,
                     100 * med['E-step'] / total, med['item half-step, torch bmm+cholesky'] / med['item half-step (K21)']), flush=True)
            del iblocks, st, w
        del F, chol
        ff.chol = None
        torch.cuda.empty_cache()


if __name__ == '__main__':
    main()
