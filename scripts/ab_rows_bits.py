"""The bits of the gradient-trained family (K25 LMF, K27 SMF) on a fixed, seeded set of cases, one SHA-256 per output: to be run on two
trees whose printouts must be identical, line for line.  The tree is an argument, because binding and models are part of what is
compared: its top-k-rec_amd is imported, and with it the libtkr_hip.so built there.
  dense   lmf_dense_rows (with and without want_loss), smf_lse_rows and smf_dense_rows (no offsets, row, column, both; one +inf in
          seven column offsets): every KT of both models (LMF K in 3, 32, 33, 64, 65, 96, 97, 128, 130; SMF K in 2, 31, 32, 33, 64, 65,
          96, 97, 128, 129) x n_x in 1, 33, 129, 130 (one lane, a partial wave, a second workgroup) x n_y in 1, 31, 33, 4096, 4097,
          8200 (a partial tile, one slab, two, three)
  step    lmf_step_rows and smf_step_rows: k in 1, 30, 63, 64, 127, 128 (NR 1, 2, 3 at k + 1 and at k + 2 columns), rows with the like
          counts of the oracles' STEP_M, one with a like outside the table, one with a descending like_ptr; heavy_from in 8, 300, none;
          both `fixed` conventions, both SMF scalings, with and without the row loss: X, H, the row loss, the status word
  models  LMF and SMF on tests/golden/g2, 5 iterations: fue, fie, fib, fub, hu, hi, losses, the log lines without their times;
          fold_in(steps=5) of five users; the arrays of the exported .npz; a second train(max_iter=1, model_path=...)
python scripts/ab_rows_bits.py TREE [dense] [step] [models]        (none: all three)"""
import contextlib
import hashlib
import io
import os
import re
import sys
import tempfile

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if len(sys.argv) < 2 or not os.path.isdir(os.path.join(sys.argv[1], 'top-k-rec_amd')):
    raise SystemExit(__doc__)
ROOT = os.path.abspath(sys.argv[1])
sys.path[:0] = [ROOT, os.path.join(ROOT, 'top-k-rec_amd')]
import numpy as np
import torch

import lmf
import smf
import tkr_hip

LIKES = (0, 1, 2, 7, 8, 9, 31, 64, 65, 300, 700, 5)       # tests/_lmf_oracle.py and tests/_smf_oracle.py: STEP_M
N_Y = 41
ALL = hashlib.sha256()


def sha(x):
    if isinstance(x, torch.Tensor):
        x = x.cpu().numpy()
    return hashlib.sha256(np.ascontiguousarray(x).tobytes()).hexdigest()


def show(tag, **outputs):
    line = '%-64s %s' % (tag, ' '.join('%s %s' % (name, 'none' if x is None else sha(x)) for name, x in outputs.items()))
    ALL.update(line.encode())
    print(line, flush=True)


def table(rng, n, K, dev, scale=0.5):
    return torch.from_numpy((rng.standard_normal((n, K)) * scale).astype(np.float32)).to(dev)


def dense(dev):
    for model, widths in (('lmf', (3, 32, 33, 64, 65, 96, 97, 128, 130)), ('smf', (2, 31, 32, 33, 64, 65, 96, 97, 128, 129))):
        for K in widths:
            for n_y in (1, 31, 33, 4096, 4097, 8200):
                rng = np.random.Generator(np.random.PCG64([25, K, n_y]))
                Y = table(rng, n_y, K, dev, 0.3)
                X_all = table(rng, 130, K, dev, 0.3)
                col = table(rng, n_y, 1, dev).reshape(-1).contiguous()
                col[::7] = float('inf')
                for n_x in (1, 33, 129, 130):
                    X = X_all[:n_x].contiguous()
                    tag = '%s K %d n_x %d n_y %d' % (model, K, n_x, n_y)
                    if model == 'lmf':
                        show('lmf_dense_rows ' + tag, D=tkr_hip.lmf_dense_rows(X, Y))
                        D, sp = tkr_hip.lmf_dense_rows(X, Y, want_loss=True)
                        show('lmf_dense_rows want_loss ' + tag, D=D, sp=sp)
                        continue
                    lse = tkr_hip.smf_lse_rows(X, Y)
                    show('smf_lse_rows ' + tag, lse=lse)
                    for name, offsets in (('none', {}), ('row', dict(row_off=lse)), ('col', dict(col_off=col)), ('both', dict(row_off=lse, col_off=col))):
                        show('smf_dense_rows %s %s' % (name, tag), D=tkr_hip.smf_dense_rows(X, Y, **offsets))


def likes(rng, dev):
    """rows with LIKES[r mod 12] likes, twice over and one more; row 3: one like outside the table among its own; row 17's like_ptr
    lies above row 18's"""
    lists = [rng.integers(0, N_Y, LIKES[r % len(LIKES)]) for r in range(2 * len(LIKES) + 1)]
    lists[3][len(lists[3]) // 2] = N_Y + 5
    ptr = np.zeros(len(lists) + 1, np.int64)
    np.cumsum([len(x) for x in lists], out=ptr[1:])
    ptr[17] = ptr[18] + 3
    return torch.from_numpy(ptr).to(dev), torch.from_numpy(np.concatenate(lists).astype(np.int32)).to(dev)


def step(dev):
    for k in (1, 30, 63, 64, 127, 128):
        rng = np.random.Generator(np.random.PCG64([27, k]))
        ptr, cols = likes(rng, dev)
        n_x = ptr.numel() - 1
        for model, K in (('lmf', k + 2), ('smf', k + 1)):
            Y, X0, D = table(rng, N_Y, K, dev), table(rng, n_x, K, dev), table(rng, n_x, K, dev)
            H0 = torch.from_numpy((1 + rng.random((n_x, K))).astype(np.float32)).to(dev)
            if model == 'lmf':
                calls = [('fixed %d' % fixed, tkr_hip.lmf_step_rows, dict(fixed=fixed, alpha=1.7, lam=0.3, lr=0.5)) for fixed in (k + 1, k)]
            else:
                calls = [('fixed %d by likes %s' % (fixed, by), tkr_hip.smf_step_rows, dict(fixed=fixed, scale_by_likes=by, lam=0.3, lr=0.5))
                         for fixed, by in ((k, True), (-1, False))]
            for name, fn, hyper in calls:
                for heavy_from in (8, 300, 1 << 62):
                    for want_loss in (False, True):
                        X, H = X0.clone(), H0.clone()
                        loss, st = fn(Y, D, ptr, cols, X, H, heavy_from=heavy_from, want_loss=want_loss, check=False, **hyper)
                        show('%s_step_rows k %d %s heavy_from %d' % (model, k, name, heavy_from), X=X, H=H, row_loss=loss, status=st)


def models(dev):
    d = os.path.join(HERE, 'tests', 'golden', 'g2')
    files = [os.path.join(d, name) for name in ('uid', 'vid', 'f0tr.txt')]
    histories = [[0, 3, 5], [], [1], [2, 2, 4, 7], [6]]
    for name, make in (('LMF', lambda: lmf.LMF(k=8)), ('SMF', lambda: smf.SMF(k=8, lam=0.01, lr=0.1))):
        with tempfile.TemporaryDirectory() as tmp:
            path = os.path.join(tmp, 'model')
            log = io.StringIO()
            with contextlib.redirect_stdout(log):
                model = make()
                model.load_training_data(*files, seed=11)
                model.train(max_iter=5, device=dev)
                folded = model.fold_in(histories, steps=5, device=dev)
                model.export_embeddings(path)
                again = make()
                again.load_training_data(*files, seed=12)
                again.train(max_iter=1, model_path=path, device=dev)
            lines = [re.sub(r', time [0-9.]+s$', '', line.split(': ', 1)[1]) for line in log.getvalue().splitlines() if ': Iter' in line]
            state = lambda m: {key: getattr(m, key) for key in ('fue', 'fie', 'fib', 'fub', 'hu', 'hi') if hasattr(m, key)}
            show('%s on g2, 5 iterations' % name, losses=np.asarray(model.losses, dtype=np.float64), log=np.frombuffer('\n'.join(lines).encode(), dtype=np.uint8),
                 **state(model))
            show('%s fold_in of five users, 5 steps' % name, **{'out%d' % i: x for i, x in enumerate(folded if isinstance(folded, tuple) else (folded,))})
            with np.load(os.path.join(path, '%s.npz' % name.lower())) as z:
                show('%s.npz' % name.lower(), **{key: z[key] for key in z.files})
            show('%s a second train from the directory, 1 iteration' % name, losses=np.asarray(again.losses, dtype=np.float64),
                 iters=np.int64(again.iters_done), **state(again))
            for line in lines:
                print('    ' + line, flush=True)


def main():
    if not torch.cuda.is_available():
        raise SystemExit('ab_rows_bits.py runs the kernels; no GPU is visible')
    dev = torch.device('cuda', 0)
    for part in sys.argv[2:] or ['dense', 'step', 'models']:
        {'dense': dense, 'step': step, 'models': models}[part](dev)
    torch.cuda.synchronize()
    print('all of the above: %s' % ALL.hexdigest(), flush=True)


if __name__ == '__main__':
    main()
