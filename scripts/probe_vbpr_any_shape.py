"""Microseconds per VBPR batch at the shapes only the generic sparse view (k // 2 > 128 beyond the column plan) and the occt-indexed
records (batch > 65,536) take: VbprEngine.run_batches (K1 + the step) between two device events after one warm-up batch.

    python scripts/probe_vbpr_any_shape.py            # one JSON line per shape"""
import json
import os
import sys
import warnings

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'top-k-rec_amd')]
import numpy as np
import torch

from oracle import plan_np as P
from single import _engine

# name: (users, items, k, d, nonzeros per feature row (d: dense), batch, timed batches)
SHAPES = {'k300_dense_d4096_B256': (20000, 10000, 300, 4096, 4096, 256, 10),
          'k300_sparse_d20000_B2048': (20000, 10000, 300, 20000, 100, 2048, 10),
          'k128_sparse_d2000_B131072': (20000, 10000, 128, 2000, 100, 131072, 3)}


def main():
    warnings.simplefilter('ignore')
    dev = torch.device('cuda')
    for name, (nu, ni, k, d, nnz, B, nb) in SHAPES.items():
        rng = np.random.Generator(np.random.PCG64(1))
        tr = {u: [int(x) for x in rng.integers(0, ni, int(rng.integers(1, 20)))] for u in range(nu)}
        row_ptr, pos, _ = P.build_csr(tr, nu)
        csr = _engine.TrainingCSR.from_arrays(row_ptr, pos, np.arange(nu, dtype=np.int32), dev)
        if nnz >= d:
            f = rng.random((ni, d), dtype=np.float32) + 0.1
        else:
            f = np.zeros((ni, d), np.float32)
            f[np.repeat(np.arange(ni), nnz), rng.integers(0, d, ni * nnz)] = rng.random(ni * nnz, dtype=np.float32) + 0.1
        f /= np.linalg.norm(f, axis=1, keepdims=True)
        hp = dict(lu=2.5e-3, li=2.5e-3, lj=2.5e-4, lb=1e-3, le=1e-3, lr=1e-3, mode='l2')
        eng = _engine.VbprEngine(nu, ni, k, d, torch.from_numpy(f).to(dev), hp, dev, seed=5)
        eng.run_batches(csr, 1, B)                                   # code objects, workspace, plan buffers
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        loss = eng.run_batches(csr, nb, B)
        e1.record()
        torch.cuda.synchronize()
        print(json.dumps(dict(shape=name, us_per_batch=round(1e3 * e0.elapsed_time(e1) / nb, 1), batches=nb, column_plan=eng.wants_cols(B),
                              finite=bool(torch.isfinite(loss).all()))), flush=True)


if __name__ == '__main__':
    main()
