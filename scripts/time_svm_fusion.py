"""K23 (tkr_fusion_svm_sums: the sums of a Newton pass of the SVM fusion) at the ML-10M shape (69,878 x 10,380; synth.train_csr_shape's
training likes), the reference's 1,000,000 sampled triplets, M = 3, 8 and 16 models at k = 50, beside the same computation in torch on
the same device, in fp64:
  sums pass    tkr_fusion_svm_sums over the 1,000,000 rows of D (two launches)   | torch: X = (D, y) in fp64, z = X W, the mask 1 - z > 0,
                                                                                   X_active^T X_active, (1 - z)_active X_active, their squares
  learn_svm    svmfusion.learn_svm end to end: features, Newton passes, host solve | torch: the same features kernel and the same
                                                                                   svmfusion.newton on the torch sums
Model 0 fits the likes (its user rows are three times the mean of the liked items' rows), so the iteration takes several passes over a
changing active set; the other models are noise.
python scripts/time_svm_fusion.py [repeats]
Warm-up of every leg, then `repeats` rounds that alternate the legs in this one process; each pass is timed by a pair of device
events.  Prints min / median / max per leg in ms."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'top-k-rec_amd')]
import numpy as np
import torch

import svmfusion
import synth
import tkr_hip
from single import _engine

N_USERS, N_ITEMS, K = 69878, 10380, 50
SAMPLES, C_SVM = 1_000_000, 0.01


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def make_models(M, like_ptr, like_cols, dev, seed=3):
    g = torch.Generator(device=dev)
    g.manual_seed(seed)
    rnd = lambda *shape: ((torch.randn(shape, device=dev, generator=g) * 0.1 * 1e6).round() / 1e6).contiguous()
    models = [(rnd(N_USERS, K), rnd(N_ITEMS, K), rnd(N_ITEMS) if m % 2 else None) for m in range(M)]
    n_like = like_ptr[1:] - like_ptr[:-1]
    rows = torch.repeat_interleave(torch.arange(N_USERS, device=dev), n_like)
    V = models[0][1] * 4
    U = torch.zeros((N_USERS, K), device=dev).index_add_(0, rows, V.index_select(0, like_cols.long())) / n_like.clamp(min=1).unsqueeze(1) * 3
    models[0] = (U.contiguous(), V.contiguous(), None)
    return models


def torch_sums(D, y, W):
    X = torch.cat([D.double(), y], dim=1)
    a = 1.0 - X @ W
    act = a > 0
    Xa, aa = X[act], a[act]
    return Xa.t() @ Xa, aa @ Xa, aa @ aa, act.sum()


def torch_learn(models, csr, M):
    D = tkr_hip.fusion_features(models, csr, N_ITEMS, 0, 0, SAMPLES)
    y = (1.0 - 2.0 * (torch.arange(SAMPLES, device=D.device) % 2).double()).unsqueeze(1)

    def sums(w):
        S, r, q, count = torch_sums(D, y, torch.from_numpy(w).to(D.device))
        return S.cpu().numpy(), r.cpu().numpy(), float(q), int(count)

    return svmfusion.newton(sums, M, SAMPLES, C_SVM, 50)


def report(name, legs, repeats):
    for _, fn in legs:                                               # warm-up: code objects, the allocator's blocks
        fn()
        fn()
    torch.cuda.synchronize()
    times = {label: [] for label, _ in legs}
    for _ in range(repeats):
        for label, fn in legs:
            times[label].append(timed(fn))
    for label, _ in legs:
        t = times[label]
        print('%-10s %-26s min %9.3f  median %9.3f  max %9.3f ms' % (name, label, min(t), float(np.median(t)), max(t)), flush=True)


def main():
    repeats = int(sys.argv[1]) if len(sys.argv) > 1 else 5
    if not torch.cuda.is_available():
        raise SystemExit('time_svm_fusion.py measures on the GPU; none is visible')
    dev = torch.device('cuda', 0)
    row_ptr, pos, srt, tr_users = synth.train_csr_shape(N_USERS, N_ITEMS)
    csr = _engine.TrainingCSR.from_arrays(row_ptr, pos, tr_users, dev)
    like_ptr = torch.from_numpy(row_ptr.astype(np.int64)).to(dev)
    like_cols = torch.from_numpy(srt).to(dev)
    print('shape %d x %d, %d training likes; %d samples, C = %g, slab %d' % (N_USERS, N_ITEMS, csr.nnz, SAMPLES, C_SVM, tkr_hip.FUSION_SVM_SLAB),
          flush=True)
    for M in (3, 8, 16):
        models = make_models(M, like_ptr, like_cols, dev)
        name = 'M = %d' % M
        W, info = svmfusion.learn_svm(models, csr, N_ITEMS, n_samples=SAMPLES, C=C_SVM, want_info=True)
        ref = torch_learn(models, csr, M)
        print('%-10s learn_svm: %d Newton steps, %d of %d rows active, max|g| = %.3g; torch: %d steps, max |w~ - torch w~| = %.3g, max|w~| = %.3g'
              % (name, info['iterations'], info['active'], SAMPLES, info['grad'], ref['iterations'],
                 float(np.abs(np.concatenate([info['weights'], [info['intercept']]]) - ref['w']).max()), float(np.abs(ref['w']).max())), flush=True)
        D = tkr_hip.fusion_features(models, csr, N_ITEMS, 0, 0, SAMPLES)
        y = (1.0 - 2.0 * (torch.arange(SAMPLES, device=dev) % 2).double()).unsqueeze(1)
        Wd = torch.from_numpy(ref['w']).to(dev)
        partial = torch.empty(tkr_hip.fusion_svm_partial_bytes(SAMPLES, M) // 8, dtype=torch.float64, device=dev)
        out = torch.empty(tkr_hip.fusion_svm_words(M), dtype=torch.float64, device=dev)
        status = torch.empty(1, dtype=torch.int64, device=dev)
        report(name, [('sums pass', lambda: tkr_hip.fusion_svm_sums(D, Wd, partial=partial, out=out, status=status, check=False)),
                      ('torch sums pass', lambda: torch_sums(D, y, Wd))], repeats)
        del D, y
        report(name, [('learn_svm', lambda: svmfusion.learn_svm(models, csr, N_ITEMS, n_samples=SAMPLES, C=C_SVM)),
                      ('torch learn', lambda: torch_learn(models, csr, M))], max(2, repeats // 2))
        del models


if __name__ == '__main__':
    main()
