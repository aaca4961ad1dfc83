"""Fold-in: user vectors for users the model was not trained on, on MI355X (K9, csrc/foldin.hip).

    U = fold_in(fie, fib, histories, lu=2.5e-3, lr=0.05, steps=50, triplets=16, seed=0)

The model's own BPR step (single/bpr.py:81-100) with the item side frozen, ``steps`` times on ``triplets`` triplets per user and
step, every user independent of the others (include/tkr.h tkr_bpr_foldin).  ``fie`` [n_items, k] / ``fib`` [n_items, 1] or None
are the exported item factors of BPR or VBPR (VBPR's already hold the content half: fie = [ire | feat.cem]).  Array in, array out;
ratings files are the business of ``BPR.fold_in`` and ``recommend.py``.
"""
from __future__ import annotations

import numpy as np
import torch

import tkr_hip


def group_history(rows, cols, m, n_items):
    """(user row, item index) pairs in any order, duplicates allowed -> (ptr int64 [m+1], cols int32 ascending and unique per row)"""
    rows, cols = np.asarray(rows, dtype=np.int64), np.asarray(cols, dtype=np.int64)
    if len(cols) and (cols.min() < 0 or cols.max() >= n_items):
        raise ValueError('history holds an item index outside [0, %d)' % n_items)
    key = np.unique(rows * n_items + cols)
    ptr = np.zeros(m + 1, dtype=np.int64)
    np.cumsum(np.bincount(key // n_items, minlength=m), out=ptr[1:])
    return ptr, (key % n_items).astype(np.int32)


def history_csr(histories, n_items):
    """a list of item-index sequences, one per user -> the CSR of group_history"""
    lens = [len(h) for h in histories]
    cols = np.concatenate([np.asarray(h, dtype=np.int64).reshape(-1) for h in histories] + [np.zeros(0, np.int64)])
    return group_history(np.repeat(np.arange(len(lens), dtype=np.int64), lens), cols, len(lens), n_items)


def fold_in(fie, fib, histories, *, lu, lr, mode='l2', steps=50, triplets=16, seed=0, first_row=0, U0=None, device=None,
            want_loss=False):
    """-> U fp32 [m, k] (numpy; with want_loss also the per-user objective of the last step).  Users with an empty history, or one
    that covers the catalogue, keep U0 (zeros by default: such a user is ranked by the item biases).  ``histories``: a list of
    item-index sequences, one per user, or the (ptr, cols) pair group_history returns."""
    if device is None:
        if not torch.cuda.is_available():
            raise tkr_hip.TkrError('fold_in runs on the GPU through libtkr_hip.so; no MI355X is visible')
        device = torch.device('cuda', torch.cuda.current_device())
    fie = np.ascontiguousarray(fie, dtype=np.float32)
    n_items = fie.shape[0]
    ptr, cols = histories if isinstance(histories, tuple) else history_csr(histories, n_items)
    V = torch.from_numpy(fie).to(device)
    b = None if fib is None else torch.from_numpy(np.ascontiguousarray(np.asarray(fib, dtype=np.float32).reshape(-1))).to(device)
    start = None if U0 is None else torch.from_numpy(np.ascontiguousarray(U0, dtype=np.float32)).to(device)
    out = tkr_hip.fold_in(V, b, torch.from_numpy(ptr).to(device), torch.from_numpy(cols).to(device), lu=lu, lr=lr, mode=mode, steps=steps,
                          triplets=triplets, seed=seed, first_row=first_row, U0=start, want_loss=want_loss)
    if want_loss:
        return out[0].cpu().numpy(), out[1].cpu().numpy()
    return out.cpu().numpy()
