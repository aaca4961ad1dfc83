"""The bits of the VBPR step (K3) on a fixed, seeded set of cases, one SHA-256 per table: to be run on two trees whose printouts must be
identical, line for line ('#' lines excepted).  The tree is an argument, because binding and engine are part of what is compared: its
top-k-rec_amd is imported, and with it the libtkr_hip.so built there.

Every case is 300 users x 120 items, content features with exactly r nonzeros per row (so the row cap of the column plan is r), three
batches (one at batch 70,000) through VbprEngine.run_batches; printed: U, msU, I, msI, irb, msirb, cem, mscem, icb, msicb, and for the
column-plan cases the loss vector, which is reproducible bit for bit there.  The loss of the views that add it up in spread atomic
slots is printed on a '#' line and not compared.  What a case launches follows from tkr_vbpr_run_cols / tkr_vbpr_run:

  column plan      k 16   d 40    r 40   B 64    tproject<1,4>,  update<1,4,16>  (a column's run: 2 B r / d = 128 > 32)
                   k 16   d 2000  r 8    B 128   update<1,4,4>
                   k 64   d 4000  r 100  B 256   tproject<1,8>,  update<1,8,4>
                   k 64   d 400   r 100  B 256   update<1,8,16>
                   k 128  d 8000  r 200  B 256   tproject<1,16>, update<2,16,4>
                   k 128  d 800   r 200  B 256   update<2,16,16>
                   k 192  d 2000  r 40   B 128   tproject<2,4>,  update<3,32,4>
                   k 192  d 100   r 40   B 128   update<3,32,16>
                   k 256  d 4000  r 100  B 512   tproject<2,8>,  update<4,32,4>
                   k 256  d 400   r 100  B 512   update<4,32,16>
  ... generic      k 272, 274     d 300  r 20  B 64      vbpr_wide_* (k // 2 = 136 > 128; 137 is no multiple of 4 either.  The engine keeps
                                                         k // 2 <= 128 that is no multiple of 4 off the column plan, so k = 20 is below)
  sparse           k 16, 20, 128, 192, 256  d 300  r 30  B 256   (TKR_VBPR_COLS=0) NH 1 / 2, NE 1 to 4, team 4
                   k 64   d 300   r 30   B 8192  team 8
  ... generic      k 272  d 700   r 70   B 1500  vbpr_gen_*
  ... no parities  k 64, 272  d 300  r 30  B 256  vbpr_occur_kernel and G2: the plan wrapped as tests/test_gpu_vbpr_any_shape.py wraps it
  dense            k 16, 128, 192, 256  d 128  every entry nonzero  B 64   (sparse=False) NT 1 to 4
  one batch        k 16   d 200   r 20   B 70,000  sparse and dense: team 16, records read with kBig
python scripts/ab_vbpr_bits.py TREE"""
import hashlib
import os
import sys
import warnings

if len(sys.argv) != 2 or not os.path.isdir(os.path.join(sys.argv[1], 'top-k-rec_amd')):
    raise SystemExit(__doc__)
ROOT = os.path.abspath(sys.argv[1])
sys.path[:0] = [ROOT, os.path.join(ROOT, 'top-k-rec_amd')]
import numpy as np
import torch

import tkr_hip
from single import _engine
from single._config import Tuning

N_USERS, N_ITEMS = 300, 120
ALL = hashlib.sha256()
N_HASHES = 0


def sha(t):
    return hashlib.sha256(np.ascontiguousarray(t.cpu().numpy()).tobytes()).hexdigest()


def features(d, r, seed):
    rng = np.random.Generator(np.random.PCG64(seed))
    feat = np.zeros((N_ITEMS, d), np.float32)
    for row in range(N_ITEMS):
        feat[row, rng.choice(d, r, replace=False)] = rng.random(r) + 0.1
    return (feat / np.linalg.norm(feat, axis=1, keepdims=True)).astype(np.float32)


class NoParities:
    """a plan buffer seen without K1's per-triplet parities (tests/test_gpu_vbpr_any_shape.py)"""

    def __init__(self, plan):
        self._plan = plan

    def __getattr__(self, name):
        if name == 'tpar':
            raise AttributeError(name)
        return getattr(self._plan, name)


def case(csr, view, k, d, r, B, nb=3, parities=True, lr=0.02):
    """view: 'cols' (the column plan, asserted), 'sparse' (the five launches on the CSR view) or 'dense'"""
    global N_HASHES
    dev = csr.row_ptr.device
    kh = k // 2
    hp = dict(lu=2.5e-3, li=2.5e-3, lj=2.5e-4, lb=1e-3, le=1e-3, lr=lr, mode='l2')
    eng = _engine.VbprEngine(N_USERS, N_ITEMS, k, d, features(d, r, [3, d, r]), hp, dev, seed=5, sparse=view != 'dense',
                             tuning=Tuning(vbpr_cols=view == 'cols'))
    rng = np.random.Generator(np.random.PCG64([7, k, d]))
    eng.set_dense(cem=(rng.standard_normal((d, kh)) * 0.05).astype(np.float32), icb=(rng.standard_normal(d) * 0.05).astype(np.float32))
    eng.set_items(irb=(rng.standard_normal(N_ITEMS) * 0.01).astype(np.float32))
    assert eng.wants_cols(B) == (view == 'cols'), (view, k, d, r, B)
    assert (eng.sparse is None) == (view == 'dense') and (view == 'dense' or eng.max_row_nnz == r)
    real = tkr_hip.vbpr_run
    if not parities:
        tkr_hip.vbpr_run = lambda state, plan, *a, **kw: real(state, NoParities(plan), *a, **kw)
    try:
        with warnings.catch_warnings():
            warnings.simplefilter('ignore')
            loss = eng.run_batches(csr, nb, B)
        torch.cuda.synchronize()
    finally:
        tkr_hip.vbpr_run = real
    tables = dict(zip(('U', 'msU'), eng.get('U')))
    tables.update(zip(('I', 'msI'), eng.get('I')))
    tables.update(zip(('irb', 'msirb'), eng.get('irb')))
    tables.update(cem=eng.cem, mscem=eng.mscem, icb=eng.icb, msicb=eng.msicb)
    if view == 'cols':
        tables['loss'] = loss
    tag = '%s%s k %d d %d r %d B %d' % (view, '' if parities else ', no parities', k, d, r, B)
    line = '%-44s %s' % (tag, ' '.join('%s %s' % (name, sha(t)) for name, t in tables.items()))
    ALL.update(line.encode())
    N_HASHES += len(tables)
    print(line, flush=True)
    if view != 'cols':
        print('# %s loss %s' % (tag, ' '.join('%.9g' % x for x in loss.cpu().numpy())), flush=True)


def main():
    if not torch.cuda.is_available():
        raise SystemExit('ab_vbpr_bits.py runs the kernels; no GPU is visible')
    rng = np.random.Generator(np.random.PCG64(1))
    tr = {int(u): [int(x) for x in rng.integers(0, N_ITEMS, int(rng.integers(1, 10)))] for u in rng.permutation(N_USERS)[: N_USERS - 5]}
    csr = _engine.TrainingCSR(tr, list(tr.keys()), N_USERS, torch.device('cuda', 0))
    for k, d, r, B in ((16, 40, 40, 64), (16, 2000, 8, 128), (64, 4000, 100, 256), (64, 400, 100, 256), (128, 8000, 200, 256),
                       (128, 800, 200, 256), (192, 2000, 40, 128), (192, 100, 40, 128), (256, 4000, 100, 512), (256, 400, 100, 512),
                       (272, 300, 20, 64), (274, 300, 20, 64)):
        case(csr, 'cols', k, d, r, B)
    for k in (16, 20, 128, 192, 256):
        case(csr, 'sparse', k, 300, 30, 256)
    case(csr, 'sparse', 64, 300, 30, 8192)
    case(csr, 'sparse', 272, 700, 70, 1500)
    for k in (64, 272):
        case(csr, 'sparse', k, 300, 30, 256, parities=False)
    for k in (16, 128, 192, 256):
        case(csr, 'dense', k, 128, 128, 64)
    for view in ('sparse', 'dense'):
        case(csr, view, 16, 200, 20, 70000, nb=1, lr=1e-4)
    print('all of the above, %d hashes: %s' % (N_HASHES, ALL.hexdigest()), flush=True)


if __name__ == '__main__':
    main()
