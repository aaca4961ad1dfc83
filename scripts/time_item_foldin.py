"""K10 (tkr_bpr_foldin_items: rows of new items folded in against the frozen model) at the ML-10M shape, beside K9 (tkr_bpr_foldin) on
as many rows in the same process.
python scripts/time_item_foldin.py [new_items] [likers_per_item] [repeats]
k = 128, 69,878 users x 10,380 items with ~36 positives per user; `new_items` (1,000) new items with `likers_per_item` (50) likers each,
drawn uniformly among the users with a row; the default depth (foldin.ITEM_STEPS steps of ITEM_TRIPLETS triplets) and the thresholds
of foldin.role_thresholds.  Warm-up, then `repeats` passes, each timed by a pair of device events.  Prints rows/s and triplets/s of
K10, of K10 with roles='positive', and of K9 on the first `new_items` users of the shape at the same steps x triplets, and the ratio
per row.  K10's draw is one dependent load longer than K9's (user -> row bounds -> candidate -> membership; K9 has its row bounds
per wave), and a role-0 triplet searches the liker list once per candidate user."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'top-k-rec_amd')]
import numpy as np
import torch

import foldin
import synth
import tkr_hip

m = int(sys.argv[1]) if len(sys.argv) > 1 else 1000
per_item = int(sys.argv[2]) if len(sys.argv) > 2 else 50
repeats = int(sys.argv[3]) if len(sys.argv) > 3 else 5
if not torch.cuda.is_available():
    raise SystemExit('time_item_foldin.py measures on the GPU; none is visible')
dev = torch.device('cuda', 0)
n_users, n_items, k, mean_pos = 69878, 10380, 128, 36.0
T, P = foldin.ITEM_STEPS, foldin.ITEM_TRIPLETS


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def report(name, run, rows):
    for _ in range(2):
        run()
    torch.cuda.synchronize()
    t = [timed(run) for _ in range(repeats)]
    med = float(np.median(t)) * 1e-3
    print('%-22s min %8.3f  median %8.3f  max %8.3f ms   %.2f M rows/s  %.1f M triplets/s'
          % (name, min(t), med * 1e3, max(t), rows / med / 1e6, rows * T * P / med / 1e6), flush=True)
    return med / rows


row_ptr, pos, srt, tr_users = synth.train_csr_shape(n_users, n_items, mean_pos=mean_pos, seed=42)
rng = np.random.Generator(np.random.PCG64(7))
with_row = np.flatnonzero(np.diff(row_ptr) > 0)
likers = [np.sort(rng.choice(with_row, per_item, replace=False)) for _ in range(m)]
uptr = row_ptr.astype(np.int64)
lptr, lrows = foldin.history_csr(likers, n_users)
g = torch.Generator(device=dev)
g.manual_seed(11)
U = torch.randn((n_users, k), device=dev, generator=g) * 0.1
V = torch.randn((n_items, k), device=dev, generator=g) * 0.1
b = torch.randn(n_items, device=dev, generator=g) * 0.1
d = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
uptr_d, ucols_d, lptr_d, lrows_d = d(uptr), d(srt), d(lptr), d(lrows)
print('%d users x %d items, k = %d, %.1f positives per user; %d new items x %d likers, T = %d, P = %d'
      % (n_users, n_items, k, len(srt) / n_users, m, per_item, T, P), flush=True)
per_row = {}
for roles in ('both', 'positive'):
    thresh = foldin.role_thresholds(uptr, lptr, lrows, n_items, roles)
    if roles == 'both':
        print('share of role-1 triplets: mean %.4f' % float(np.mean(thresh / 2.0 ** 32)), flush=True)
    run = lambda: tkr_hip.fold_in_items(U, V, b, uptr_d, ucols_d, lptr_d, lrows_d, thresh, li=2.5e-3, lj=2.5e-4, lb=0.0, lr=0.05, steps=T,
                                        triplets=P, seed=1)
    per_row[roles] = report('K10 roles=%s' % roles, run, m)
first = with_row[:m]
hptr = np.zeros(m + 1, np.int64)
np.cumsum(np.diff(row_ptr)[first], out=hptr[1:])
hcols = np.concatenate([srt[row_ptr[u]:row_ptr[u + 1]] for u in first])
hptr_d, hcols_d = d(hptr), d(hcols)
per_row['K9'] = report('K9 on %d users' % m, lambda: tkr_hip.fold_in(V, b, hptr_d, hcols_d, lu=2.5e-3, lr=0.05, steps=T, triplets=P, seed=1), m)
print('K10 / K9 per row at equal steps x triplets: %.2f (roles=both), %.2f (roles=positive)'
      % (per_row['both'] / per_row['K9'], per_row['positive'] / per_row['K9']), flush=True)
