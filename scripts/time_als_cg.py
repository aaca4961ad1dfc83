"""K24 (one ALS iteration under solver='cg': tkr_als_gram_wide + tkr_als_cg_rows for the users, then for the items) beside the same
iteration under solver='cholesky' (K20) of the same tree, at the shapes of scripts/time_als.py: the ML-10M shape (69,878 users x 10,380
items) and the Netflix shape (480,189 x 17,770), likes drawn as synth.train_csr_shape draws them.
  legs   k = 50 and 128: 'cholesky' and 'cg' (3 steps) alternated in this one process; k = 256: 'cg' alone (K20 stops at 128)
  steps  the 'cg' iteration at 2, 3 and 5 steps
  split  of the 'cg' iteration (3 steps): the Gram of each side, the user solve, the item solve (with its loss rows); for each solve the
         bytes its like gathers move ((steps + 1) products, + 1 for the loss, each reading every liked row once: n_likes * 4 k bytes)
         over its time, beside the 8.6 TB/s gather roofline K12 uses; and the same call with every like list empty and a prior of zeros
         (every row is still solved: P G on the MFMA and the vector updates, no gather) as a share of the solve
  tol    (ml10m, k = 50 only) the iterations each solver takes until |loss' - loss| / loss < 1e-4, from the same start
python scripts/time_als_cg.py [ml10m|netflix|both] [repeats] [k ...]
Warm-up of every leg, then `repeats` rounds that alternate the legs; each pass is timed by a pair of device events: min / median / max."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'top-k-rec_amd'), os.path.join(ROOT, 'scripts')]
import numpy as np
import torch

import als
import synth
import tkr_hip
from time_als import A, B, LU, LV, SHAPES, timed, transpose_csr

GATHER_ROOF = 8.6e12


def show(tag, ms):
    print('%-58s min %9.2f  median %9.2f  max %9.2f ms' % (tag, min(ms), float(np.median(ms)), max(ms)), flush=True)
    return float(np.median(ms))


def main():
    args = sys.argv[1:]
    which = args[0] if args else 'both'
    repeats = int(args[1]) if len(args) > 1 else 3
    ks = [int(x) for x in args[2:]] or [50, 128, 256]
    if not torch.cuda.is_available():
        raise SystemExit('time_als_cg.py measures on the GPU; none is visible')
    dev = torch.device('cuda', 0)
    for name, (n_users, n_items) in SHAPES.items():
        if which not in ('both', name):
            continue
        row_ptr, pos, _, _ = synth.train_csr_shape(n_users, n_items)
        up, uc = row_ptr.astype(np.int64), np.ascontiguousarray(pos, dtype=np.int32)
        ip, ic = transpose_csr(up, uc, n_items)
        u_rated, i_rated = np.flatnonzero(np.diff(up) > 0).astype(np.int32), np.flatnonzero(np.diff(ip) > 0).astype(np.int32)
        n_likes = len(uc)
        print('%s: %d users x %d items, %d likes' % (name, n_users, n_items, n_likes), flush=True)
        d = lambda a: torch.from_numpy(a).to(dev)
        upd, ucd, ipd, icd, urd, ird = d(up), d(uc), d(ip), d(ic), d(u_rated), d(i_rated)
        for k in ks:
            g = torch.Generator(device=dev)
            g.manual_seed(20)
            U0 = torch.rand((n_users, k), device=dev, generator=g)
            V0 = torch.rand((n_items, k), device=dev, generator=g)
            w = als.Work()
            state = {}

            def iteration(solver, steps=3, U=None, V=None):
                U, V = (U0.clone(), V0.clone()) if U is None else (U, V)
                _, su = als.half_step(U, V, upd, ucd, ird, w=w, ridge_in_G=LU, ridge=0.0, a=A, b=B, solver=solver, cg_steps=steps)
                rows, sv = als.half_step(V, U, ipd, icd, urd, w=w, ridge_in_G=0.0, ridge=LV, a=A, b=B, want_loss=True, solver=solver, cg_steps=steps)
                state[solver] = (U, V, su, sv, rows)

            legs = [('cg', lambda: iteration('cg'))]
            if k <= tkr_hip.ALS_MAX_K:
                legs.insert(0, ('cholesky', lambda: iteration('cholesky')))
            for label, fn in legs:
                fn()
                torch.cuda.synchronize()
                als.check_status(torch.cat(state[label][2:4]).cpu().numpy(), ('the user step', 'the item step'))
            if len(legs) == 2:
                (Uc, Vc), (Ug, Vg) = state['cholesky'][:2], state['cg'][:2]
                print('%s k %d: one cg iteration (3 steps) against one cholesky iteration from the same start: max |dU| / max |U| = %.3g, '
                      'max |dV| / max |V| = %.3g' % (name, k, float((Ug - Uc).abs().max() / Uc.abs().max()), float((Vg - Vc).abs().max() / Vc.abs().max())),
                      flush=True)
            times = {label: [] for label, _ in legs}
            for _ in range(repeats):
                for label, fn in legs:
                    times[label].append(timed(fn))
            med = {label: show('%s k %-4d %s iteration' % (name, k, label), times[label]) for label, _ in legs}
            if len(legs) == 2:
                print('%s k %-4d cholesky / cg = %.2f' % (name, k, med['cholesky'] / med['cg']), flush=True)
            for steps in (2, 3, 5):
                fn = lambda: iteration('cg', steps)
                fn()
                show('%s k %-4d cg iteration, %d steps' % (name, k, steps), [timed(fn) for _ in range(repeats)])
            # the split of the cg iteration
            G = torch.empty((k, k), device=dev)
            U1 = state['cg'][0]
            zeros = lambda n: (torch.zeros(n + 1, dtype=torch.int64, device=dev), torch.zeros(0, dtype=torch.int32, device=dev),
                               torch.zeros((n, k), device=dev))
            for side, X0_, Y, ptr, cols, rated, rg, rs in (('users', U0, V0, upd, ucd, ird, LU, 0.0), ('items', V0, U1, ipd, icd, urd, 0.0, LV)):
                X = X0_.clone()
                want = side == 'items'
                gram = lambda: tkr_hip.als_gram_wide(Y, rated, scale=B, ridge=rg, workspace=w.workspace, out=G, check=False)
                solve = lambda: tkr_hip.als_cg_rows(Y, G, ptr, cols, X, w_like=A - B, w_rhs=A, ridge=rs, steps=3, want_loss=want, check=False)
                eptr, ecols, eprior = zeros(X.shape[0])
                bare = lambda: tkr_hip.als_cg_rows(Y, G, eptr, ecols, X, w_like=A - B, w_rhs=A, ridge=rs + 1.0, steps=3, prior=eprior, w_prior=1.0,
                                                   want_loss=want, check=False)
                gram()
                t_gram = show('%s k %-4d split %-6s gram' % (name, k, side), [timed(gram) for _ in range(repeats)])
                solve()
                t_solve = show('%s k %-4d split %-6s solve (3 steps%s)' % (name, k, side, ', loss' if want else ''), [timed(solve) for _ in range(repeats)])
                products = 3 + 1 + (1 if want else 0)
                moved = products * n_likes * 4.0 * k
                print('%s k %-4d split %-6s like gathers: %d products x %d likes x %d bytes = %.2f GB in %.2f ms: %.2f TB/s if the solve were '
                      'gathers alone, %.0f %% of the %.1f TB/s gather roofline' % (name, k, side, products, n_likes, 4 * k, moved / 1e9, t_solve,
                                                                                  moved / t_solve / 1e9, 100 * moved / (t_solve * 1e-3) / GATHER_ROOF,
                                                                                  GATHER_ROOF / 1e12), flush=True)
                X.copy_(X0_)
                bare()
                t_bare = show('%s k %-4d split %-6s the same call without likes (P G + updates)' % (name, k, side), [timed(bare) for _ in range(repeats)])
                print('%s k %-4d split %-6s P G on the MFMA and the updates: %.0f %% of the solve' % (name, k, side, 100 * t_bare / t_solve), flush=True)
            if name == 'ml10m' and k == 50:
                for solver in ('cholesky', 'cg'):
                    U, V = U0.clone(), V0.clone()
                    loss, n_iter = float(np.exp(50)), 0
                    for n_iter in range(1, 201):
                        iteration(solver, 3, U, V)
                        rows = state[solver][4]
                        new = float(rows.sum() + 0.5 * LU * U.double().square().sum() + 0.5 * LV * V.double().square().sum())
                        cond, loss = abs(loss - new) / loss, new
                        if cond < 1e-4:
                            break
                    print('%s k %-4d %s: %d iterations to tol = 1e-4, loss %.6g' % (name, k, solver, n_iter, loss), flush=True)
            del U0, V0, state, w


if __name__ == '__main__':
    main()
