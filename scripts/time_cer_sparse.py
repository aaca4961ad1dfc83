"""K26 (als.CER under estep='cg') at the shape of scripts/time_cer.py: ML-10M (69,878 users x 10,380 items), likes drawn as
synth.train_csr_shape draws them and then every fifth item's likes removed, k = 50 and 128 -- with SPARSE content features: d = 20,000
and 200,000, 100 nonzeros per item, the columns Zipf-distributed (column c with weight 1 / (c + 1)), values uniform (0, 1], every row
scaled to unit length.  By phase, medians of `repeats` rounds that alternate the legs in this one process:
  Fe = F E                   one tkr_csr_spmm                                  (d = 20,000: beside the dense fp64 product of K21)
  one product, each way      tkr_csr_spmm of F and of F^T beside torch.sparse.mm on the same device and the same CSR, with the bytes
                             the product moves (per nonzero a row of k floats gathered and 8 bytes of (col, val), per row k floats
                             written) and the share of the 8.6 TB/s gather figure K12 is held to
  the E-step                 tkr_estep_cg at 3 and at 8 steps, warm-started from the E of a converged call as train() starts it, beside
                             K21's cholesky_solve against the d x d factor (d = 20,000 only: at 200,000 the factor is 320 GB)
  the user and item half-steps (K20 / K21), and the iteration: Fe + users + items + E-step under each E-step
  heavy_from                 the F^T product and the 8-step E-step again at heavy_from = 256, 512 and 1,024 (TIME_CER_HEAVY), beside
                             the default 2,048 and beside no workgroup form at all
python scripts/time_cer_sparse.py [repeats] [k ...]      (TIME_CER_D=20000,200000 picks the feature widths)
Each pass is timed by a pair of device events; medians with min and max beside them."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'top-k-rec_amd'), os.path.join(ROOT, 'scripts')]
import numpy as np
import scipy.sparse as ss
import torch

import als
import synth
import tkr_hip
from time_als import SHAPES, timed
from time_cer import A, B, LE, LU, LV, csr_of, report

PER_ROW = 100
GATHER_TBS = 8.6


def zipf_features(n_items, d, seed=26):
    rng = np.random.Generator(np.random.PCG64([seed, d]))
    w = 1.0 / np.arange(1, d + 1)
    cols = rng.choice(d, size=(n_items, PER_ROW), p=w / w.sum())             # (with repeats: canonical_csr adds them up)
    rows = np.repeat(np.arange(n_items), PER_ROW)
    F = als.canonical_csr(ss.csr_matrix((1.0 - rng.random(n_items * PER_ROW), (rows, cols.ravel())), shape=(n_items, d)))
    F = als.canonical_csr(ss.diags(1.0 / np.sqrt(np.asarray(F.multiply(F).sum(axis=1)).ravel())) @ F)
    return F


def moved(Am, k):
    return Am.nnz * (4 * k + 8) + Am.shape[0] * 4 * k


def main():
    args = sys.argv[1:]
    repeats = int(args[0]) if args else 3
    ks = [int(x) for x in args[1:]] or [50, 128]
    ds = [int(x) for x in os.environ.get('TIME_CER_D', '20000,200000').split(',')]
    sweep = [int(x) for x in os.environ.get('TIME_CER_HEAVY', '256,512,1024').split(',') if x]
    if not torch.cuda.is_available():
        raise SystemExit('time_cer_sparse.py measures on the GPU; none is visible')
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
    d_ = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    upd, ucd, ipd, icd, urd, ird = d_(up), d_(uc), d_(ip), d_(ic), d_(u_rated), d_(i_rated)
    for dd in ds:
        Fm = zipf_features(n_items, dd)
        Ftm = als.canonical_csr(Fm.T)
        lens = np.diff(Ftm.indptr)
        print('d %-6d features: %d nonzeros (%.1f per item); rows of F^T: longest %d, %d heavier than %d, %d empty'
              % (dd, Fm.nnz, Fm.nnz / n_items, lens.max(), int((lens > tkr_hip.SPMM_HEAVY_FROM).sum()), tkr_hip.SPMM_HEAVY_FROM, int((lens == 0).sum())), flush=True)
        Fc, Ftc = tkr_hip.csr_upload(Fm, dev), tkr_hip.csr_upload(Ftm, dev)
        Ft_torch = torch.sparse_csr_tensor(Ftc.ptr, Ftc.col.long(), Ftc.val, size=Ftm.shape)
        F_torch = torch.sparse_csr_tensor(Fc.ptr, Fc.col.long(), Fc.val, size=Fm.shape)
        dense = dd <= 20000
        if dense:
            Fd = torch.from_numpy(Fm.toarray()).to(dev).double()
            chol = torch.linalg.cholesky(torch.addmm(torch.eye(dd, dtype=torch.float64, device=dev), Fd.t(), Fd, beta=LE, alpha=LV))
        g = torch.Generator(device=dev)
        g.manual_seed(21)
        for k in ks:
            U0 = torch.rand((n_users, k), device=dev, generator=g)
            V0 = torch.rand((n_items, k), device=dev, generator=g)
            ws = tkr_hip.workspace_room(None, tkr_hip.estep_cg_workspace_bytes(n_items, dd, k), dev)
            w = als.Work()
            st = {'U': U0.clone(), 'V': V0.clone()}
            # the E of a converged call: what an iteration of train() starts from
            Ewarm = torch.randn((dd, k), device=dev, generator=g)
            tkr_hip.estep_cg(Fc, Ftc, V0, Ewarm, lv=LV, le=LE, steps=24, workspace=ws)
            if dense:
                Edirect = torch.cholesky_solve(LV * (Fd.t() @ V0.double()), chol).float()
                print('d %-6d k %-4d 24 steps of CG against the Cholesky E-step: max |dE| / max |E| = %.3g'
                      % (dd, k, float((Ewarm - Edirect).abs().max() / Edirect.abs().max())), flush=True)

            def estep(steps, heavy_from=None):
                def run():
                    E = Ewarm.clone()                                 # (the copy is inside the timed span: 4 d k bytes)
                    st['se'] = tkr_hip.estep_cg(Fc, Ftc, st['V'], E, lv=LV, le=LE, steps=steps, heavy_from=heavy_from, workspace=ws, check=False)[1]
                return run

            X50 = torch.randn((dd, k), device=dev, generator=g)
            T50 = torch.randn((n_items, k), device=dev, generator=g)
            legs = {
                'Fe = F E (tkr_csr_spmm)': lambda: st.__setitem__('Fe', tkr_hip.csr_spmm(Fc, Ewarm, workspace=ws, check=False)[0]),
                'user half-step (K20)': lambda: st.__setitem__('su', als.half_step(st['U'], V0, upd, ucd, ird, w=w, ridge_in_G=LU, ridge=0.0, a=A, b=B)[1]),
                'item half-step (K21)': lambda: st.__setitem__('sv', als.half_step(st['V'], st['U'], ipd, icd, urd, w=w, ridge_in_G=0.0, ridge=LV, a=A, b=B,
                                                                                    want_loss=True, prior=st['Fe'], w_prior=LV)[1]),
                'E-step, cg 3 steps': estep(3),
                'E-step, cg 8 steps': estep(8),
                'F X: tkr_csr_spmm': lambda: tkr_hip.csr_spmm(Fc, X50, workspace=ws, check=False),
                'F X: torch.sparse.mm': lambda: torch.sparse.mm(F_torch, X50),
                'F^T T: tkr_csr_spmm': lambda: tkr_hip.csr_spmm(Ftc, T50, workspace=ws, check=False),
                'F^T T: tkr_csr_spmm, no heavy rows': lambda: tkr_hip.csr_spmm(Ftc, T50, heavy_from=tkr_hip.SPMM_NO_HEAVY, check=False),
                'F^T T: torch.sparse.mm': lambda: torch.sparse.mm(Ft_torch, T50),
            }
            for hf in sweep:                                          # a lower bar for the workgroup form (the default is SPMM_HEAVY_FROM)
                legs['F^T T: tkr_csr_spmm, heavy_from %d' % hf] = lambda hf=hf: tkr_hip.csr_spmm(Ftc, T50, heavy_from=hf, workspace=ws, check=False)
                legs['E-step, cg 8 steps, heavy_from %d' % hf] = estep(8, hf)
            if dense:
                legs['Fe = F E (K21: dense fp64)'] = lambda: (Fd @ Ewarm.double()).float()
                legs['E-step, cholesky (K21)'] = lambda: torch.cholesky_solve(LV * (Fd.t() @ st['V'].double()), chol).float()
            try:
                b = torch.sparse.mm(Ft_torch, T50)
                a = tkr_hip.csr_spmm(Ftc, T50, workspace=ws)
                print('d %-6d k %-4d F^T T against torch.sparse.mm: max |d| / max = %.3g' % (dd, k, float((a - b).abs().max() / b.abs().max())), flush=True)
            except RuntimeError as e:                                 # (a torch build without a sparse CSR product: the legs are left out)
                print('torch.sparse.mm is not available here (%s): its legs are left out' % str(e).split('\n')[0], flush=True)
                legs = {label: fn for label, fn in legs.items() if 'torch.sparse' not in label}
            for fn in legs.values():                                  # warm-up, in the order of an iteration
                fn()
            torch.cuda.synchronize()
            tkr_hip.status_check('the E-step', tkr_hip._ESTEP_REFUSED, tkr_hip.EstepRefused, int(st['se'].item()))
            times = {label: [] for label in legs}
            for _ in range(repeats):
                for label, fn in legs.items():
                    times[label].append(timed(fn))
            med = {label: report('d %-6d k %-4d %s' % (dd, k, label), ms) for label, ms in times.items()}
            for label, Am in (('F X: tkr_csr_spmm', Fm), ('F^T T: tkr_csr_spmm', Ftm)):
                nbytes = moved(Am, k)
                print('d %-6d k %-4d %s moves %.1f MB: %.2f TB/s, %.1f %% of the %.1f TB/s gather figure'
                      % (dd, k, label, nbytes / 1e6, nbytes / med[label] / 1e9, 100 * nbytes / med[label] / 1e9 / GATHER_TBS, GATHER_TBS), flush=True)
            rest = med['user half-step (K20)'] + med['item half-step (K21)']
            line = 'd %-6d k %-4d one iteration: cg 3 steps %.3f ms, cg 8 steps %.3f ms' % (
                dd, k, rest + med['Fe = F E (tkr_csr_spmm)'] + med['E-step, cg 3 steps'], rest + med['Fe = F E (tkr_csr_spmm)'] + med['E-step, cg 8 steps'])
            if dense:
                line += ', cholesky %.3f ms (E-step: cholesky / cg 8 = %.1f)' % (
                    rest + med['Fe = F E (K21: dense fp64)'] + med['E-step, cholesky (K21)'], med['E-step, cholesky (K21)'] / med['E-step, cg 8 steps'])
            print(line, flush=True)
            del st, w, ws
        if dense:
            del Fd, chol
        torch.cuda.empty_cache()


if __name__ == '__main__':
    main()
