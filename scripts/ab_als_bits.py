"""The bits of the ALS family (K20, K21, K22's loop, K24) on a fixed, seeded set of cases, one SHA-256 per output: to be run on two
builds of the tree (TKR_HIP_LIB picks the library; the Python side is the tree the script lies in) whose printouts must be identical.
  gram    als_gram and als_gram_wide: k in 1, 31, 33, 64, 96, 128 (wide: also 129, 256, 512) x 1, 32, 33, 1024, 1025, 2100 listed rows,
          as a row list and as rows=None; one list with an index outside the table
  solve   als_solve_rows and als_solve_rows_prior: the same k, 40 rows: one of 2,100 likes (heavy_from = 1024: planned slabs; and no
          heavy rows), one without likes, one with a like outside the table; the loss rows
  cg      als_cg_rows: k in 50, 128, 129, 256, 512 x 31, 32, 33 rows x 0 and 3 steps, with and without a prior, one row of 2,100 likes
  train   WMF, CER and DPM on tests/golden/g2, 3 iterations, under both solvers: fue, fie, E, the encoder, losses, the log lines
python scripts/ab_als_bits.py [gram] [solve] [cg] [train]        (none: all four)"""
import contextlib
import hashlib
import io
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'top-k-rec_amd')]
import numpy as np
import torch

import als
import tkr_hip

N_Y = 2300
ALL = hashlib.sha256()


def sha(x):
    if isinstance(x, torch.Tensor):
        x = x.cpu().numpy()
    return hashlib.sha256(np.ascontiguousarray(x).tobytes()).hexdigest()


def show(tag, **outputs):
    line = '%-58s %s' % (tag, ' '.join('%s %s' % (name, 'none' if x is None else sha(x)) for name, x in outputs.items()))
    ALL.update(line.encode())
    print(line, flush=True)


def table(rng, n, k, dev):
    return torch.from_numpy(rng.random((n, k), dtype=np.float32)).to(dev)


def gram(dev):
    for k in (1, 31, 33, 64, 96, 128, 129, 256, 512):
        rng = np.random.Generator(np.random.PCG64(k))
        Y = table(rng, N_Y, k, dev)
        for name, fn in (('als_gram', tkr_hip.als_gram), ('als_gram_wide', tkr_hip.als_gram_wide)):
            if name == 'als_gram' and k > tkr_hip.ALS_MAX_K:
                continue
            for n_listed in (1, 32, 33, 1024, 1025, 2100):
                rows = torch.from_numpy(rng.integers(0, N_Y, n_listed).astype(np.int32)).to(dev)
                G, st = fn(Y, rows, scale=0.01, ridge=0.3, check=False)
                show('%s k %d listed %d' % (name, k, n_listed), G=G, status=st)
                G, st = fn(Y[:n_listed].contiguous(), None, scale=0.01, ridge=0.3, check=False)
                show('%s k %d rows=None n %d' % (name, k, n_listed), G=G, status=st)
            rows = torch.from_numpy(rng.integers(0, N_Y, 1100).astype(np.int32))
            rows[1030] = N_Y + 7
            G, st = fn(Y, rows.to(dev), scale=0.01, ridge=0.3, check=False)
            show('%s k %d a listed row outside the table' % (name, k), G=G, status=st)


def likes(rng, n_x, dev):
    """row 3: 2,100 likes; row 5: none; row 7: one like outside the table among its own"""
    lists = [rng.integers(0, N_Y, int(rng.integers(1, 41))) for _ in range(n_x)]
    lists[3] = rng.integers(0, N_Y, 2100)
    lists[5] = lists[5][:0]
    lists[7][len(lists[7]) // 2] = N_Y + 5
    ptr = np.zeros(n_x + 1, np.int64)
    np.cumsum([len(x) for x in lists], out=ptr[1:])
    return torch.from_numpy(ptr).to(dev), torch.from_numpy(np.concatenate(lists).astype(np.int32)).to(dev)


def solve(dev):
    for k in (1, 31, 33, 64, 96, 128):
        rng = np.random.Generator(np.random.PCG64(1000 + k))
        Y, X0, prior = table(rng, N_Y, k, dev), table(rng, 40, k, dev), table(rng, 40, k, dev)
        ptr, cols = likes(rng, 40, dev)
        G = tkr_hip.als_gram(Y, None, scale=0.01, ridge=0.0)
        for heavy_from in (1024, tkr_hip.ALS_NO_HEAVY):
            X = X0.clone()
            loss, st = tkr_hip.als_solve_rows(Y, G, ptr, cols, X, w_like=0.99, w_rhs=1.0, ridge=0.01, heavy_from=heavy_from, want_loss=True, check=False)
            show('als_solve_rows k %d heavy_from %d' % (k, heavy_from), X=X, row_loss=loss, status=st)
            X = X0.clone()
            loss, st = tkr_hip.als_solve_rows_prior(Y, G, ptr, cols, X, prior, w_like=0.99, w_rhs=1.0, w_prior=0.7, ridge=0.7, heavy_from=heavy_from,
                                                    want_loss=True, check=False)
            show('als_solve_rows_prior k %d heavy_from %d' % (k, heavy_from), X=X, row_loss=loss, status=st)


def cg(dev):
    for k in (50, 128, 129, 256, 512):
        for n_x in (31, 32, 33):
            rng = np.random.Generator(np.random.PCG64(2000 + 10 * k + n_x))
            Y, X0, prior = table(rng, N_Y, k, dev), table(rng, n_x, k, dev), table(rng, n_x, k, dev)
            ptr, cols = likes(rng, n_x, dev)
            G = tkr_hip.als_gram_wide(Y, None, scale=0.01, ridge=0.0)
            for steps in (0, 3):
                for p in (None, prior):
                    X = X0.clone()
                    loss, st = tkr_hip.als_cg_rows(Y, G, ptr, cols, X, w_like=0.99, w_rhs=1.0, ridge=0.7, steps=steps, prior=p,
                                                   w_prior=0.0 if p is None else 0.7, want_loss=True, check=False)
                    show('als_cg_rows k %d n_x %d steps %d prior %s' % (k, n_x, steps, p is not None), X=X, row_loss=loss, status=st)


def train(dev):
    d = os.path.join(ROOT, 'tests', 'golden', 'g2')
    files = [os.path.join(d, name) for name in ('uid', 'vid', 'f0tr.txt')]
    k, width = 8, 24
    for solver in als.SOLVERS:
        for name in ('WMF', 'CER', 'DPM'):
            hyper = dict(k=k, lu=0.1, a=1.0, b=0.01, solver=solver, cg_steps=2)
            model = als.WMF(lv=0.1, **hyper) if name == 'WMF' else getattr(als, name)(d=width, lv=0.7, **hyper)
            log = io.StringIO()
            with contextlib.redirect_stdout(log):
                model.load_training_data(*files, seed=11)
                if name != 'WMF':
                    model.feat = np.random.Generator(np.random.PCG64(12)).standard_normal((model.n_items, width)).astype(np.float32)
                if name == 'DPM':
                    model.train(als.MLP(k, width, lr=1e-3, hidden_layers=(16, 12), seed=13), max_iter=3, device=dev, batch_size=8)
                else:
                    model.train(max_iter=3, tol=0.0, device=dev)
            lines = [re.sub(r', time [0-9.]+s$', '', line.split(': ', 1)[1]) for line in log.getvalue().splitlines() if ': Iter' in line]
            out = dict(fue=model.fue, fie=model.fie, losses=np.asarray(model.losses, dtype=np.float64), log='\n'.join(lines).encode())
            if name == 'CER':
                out['E'] = model.E
            if name == 'DPM':
                state = model.encoder.state()
                out['encoder'] = b''.join(np.ascontiguousarray(state[key]).tobytes() for key in sorted(state))
            show('%s on g2, solver %s, 3 iterations' % (name, solver), **{key: np.frombuffer(x, dtype=np.uint8) if isinstance(x, bytes) else x
                                                                           for key, x in out.items()})
            for line in lines:
                print('    ' + line, flush=True)


def main():
    if not torch.cuda.is_available():
        raise SystemExit('ab_als_bits.py runs the kernels; no GPU is visible')
    dev = torch.device('cuda', 0)
    parts = sys.argv[1:] or ['gram', 'solve', 'cg', 'train']
    for part in parts:
        {'gram': gram, 'solve': solve, 'cg': cg, 'train': train}[part](dev)
    torch.cuda.synchronize()
    print('all of the above: %s' % ALL.hexdigest(), flush=True)


if __name__ == '__main__':
    main()
