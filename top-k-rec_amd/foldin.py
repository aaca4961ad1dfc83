"""Fold-in: user vectors for users, and item rows for items, the model was not trained on, on MI355X (K9 csrc/foldin.hip, K10
csrc/foldin_items.hip).

    U = fold_in(fie, fib, histories, lu=2.5e-3, lr=0.05, steps=50, triplets=16, seed=0)

The model's own BPR step (single/bpr.py:81-100) with the item side frozen, ``steps`` times on ``triplets`` triplets per user and
step, every user independent of the others (include/tkr.h tkr_bpr_foldin).  ``fie`` [n_items, k] / ``fib`` [n_items, 1] or None
are the exported item factors of BPR or VBPR (VBPR's already hold the content half: fie = [ire | feat.cem]).  Array in, array out;
ratings files are the business of ``BPR.fold_in`` and ``recommend.py``.

    V_new, b_new = fold_in_items(fue, fie, fib, user_pos, likers, li=2.5e-3, lj=2.5e-4, lb=0.0, lr=0.05)

The twin for new items: everything but the new item's row and bias frozen (include/tkr.h tkr_bpr_foldin_items).
"""
from __future__ import annotations

import math

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


def liked_csr(R, m, n, by='user'):
    """a parsed ratings file (textio.parse_ratings) -> the group_history CSR of its like == 1 entries of known users and items:
    by='user' the m users' liked items among n, by='item' the m items' likers among n users"""
    rows, cols = {'user': (R.entry_user, R.item), 'item': (R.item, R.entry_user)}[by]
    keep = (rows >= 0) & (cols >= 0) & (R.like == 1)
    return group_history(rows[keep], cols[keep], m, n)


def _device(device, who):
    if device is None and not torch.cuda.is_available():
        raise tkr_hip.TkrError('%s runs on the GPU through libtkr_hip.so; no MI355X is visible' % who)
    return torch.device('cuda', torch.cuda.current_device()) if device is None else device


def _upload(a, device, dtype=None, flat=False):
    """an optional array -> a contiguous tensor on the device (None stays None); flat: as one dimension"""
    return None if a is None else torch.from_numpy(np.ascontiguousarray(np.asarray(a, dtype=dtype).reshape(-1 if flat else np.shape(a)))).to(device)


def fold_in(fie, fib, histories, *, lu, lr, mode='l2', steps=50, triplets=16, seed=0, first_row=0, U0=None, device=None,
            want_loss=False):
    """-> U fp32 [m, k] (numpy; with want_loss also the per-user objective of the last step).  Users with an empty history, or one
    that covers the catalogue, keep U0 (zeros by default: such a user is ranked by the item biases).  ``histories``: a list of
    item-index sequences, one per user, or the (ptr, cols) pair group_history returns."""
    device = _device(device, 'fold_in')
    ptr, cols = histories if isinstance(histories, tuple) else history_csr(histories, len(fie))
    out = tkr_hip.fold_in(_upload(fie, device, np.float32), _upload(fib, device, np.float32, flat=True), _upload(ptr, device), _upload(cols, device), lu=lu, lr=lr,
                          mode=mode, steps=steps, triplets=triplets, seed=seed, first_row=first_row, U0=_upload(U0, device, np.float32),
                          want_loss=want_loss)
    return (out[0].cpu().numpy(), out[1].cpu().numpy()) if want_loss else out.cpu().numpy()


ITEM_STEPS, ITEM_TRIPLETS, ITEM_LR = 50, 16, 0.05      # chosen by tests/test_item_foldin_cpu.py (the numbers: DESIGN.md section 4, K10)


def role_thresholds(user_ptr, liker_ptr, liker_rows, n_items, roles='both'):
    """-> uint32-valued int64 [m]: the share of a new item's triplets that carry it as the positive, as the kernel compares it with
    the first Philox word of a triplet.  The model's own sampler on the training set grown by x -- u uniform over the users with a
    row, i uniform over u's row, j uniform over the columns not in it -- draws x as the positive at the rate
    w+ = sum over its likers of 1 / (deg_u + 1) and as the negative at w- = sum over the non-likers with a row of
    1 / (n_items + 1 - deg_u), both up to the common factor 1 / n_tr: thresh = floor(2^32 w+ / (w+ + w-)), and 0xffffffff (always
    the positive) when no non-liker has a row or with roles='positive'.  Evaluated in float64 (math.fsum)."""
    if roles not in ('both', 'positive'):
        raise ValueError("roles must be 'both' or 'positive'")
    m = len(liker_ptr) - 1
    if roles == 'positive':
        return np.full(m, tkr_hip.ROLE_ALWAYS_POSITIVE, dtype=np.int64)
    deg = np.diff(np.asarray(user_ptr, dtype=np.int64))
    as_pos, as_neg = 1.0 / (deg + 1.0), np.where(deg > 0, 1.0 / (n_items + 1.0 - deg), 0.0)
    rows_total, neg_total = int((deg > 0).sum()), math.fsum(as_neg)
    out = np.empty(m, dtype=np.int64)
    for x in range(m):
        L = np.asarray(liker_rows[liker_ptr[x]:liker_ptr[x + 1]], dtype=np.int64)
        if rows_total - int((deg[L] > 0).sum()) == 0:
            out[x] = tkr_hip.ROLE_ALWAYS_POSITIVE
            continue
        wp, wm = math.fsum(as_pos[L]), max(neg_total - math.fsum(as_neg[L]), 0.0)
        out[x] = min(int(math.floor(2.0 ** 32 * (wp / (wp + wm)))), tkr_hip.ROLE_ALWAYS_POSITIVE)
    return out


def fold_in_items(fue, fie, fib, user_pos, likers, *, li, lj, lb, lr, mode='l2', steps=ITEM_STEPS, triplets=ITEM_TRIPLETS, seed=0,
                  roles='both', first_row=0, V0=None, b0=None, device=None, want_loss=False):
    """-> (V_new fp32 [m, k], b_new fp32 [m, 1]) (numpy; with want_loss also the per-item objective of the last step): rows and
    biases for m new items against the frozen model ``fue`` [n_users, k], ``fie`` [n_items, k], ``fib`` [n_items, 1] or None (then
    no bias is learnt and b_new = b0).  ``user_pos``: the users' training positives, a list of item-index sequences or the
    (ptr, cols) pair of group_history; ``likers``: per new item the user rows that like it, a list or such a pair over n_users.

    A triplet of a step carries the new item x either as the positive of one of its likers against a negative that user has not
    rated, or -- roles='both' -- as the negative of a user who does not like it against one of that user's positives, in the
    proportion role_thresholds derives from the model's own sampler.  THE ONE APPROXIMATION: inside a role the user is drawn
    uniformly (over the likers, or over the non-likers with a row), not in proportion to the weights 1 / (deg_u + 1) and
    1 / (n_items + 1 - deg_u) with which the sampler would reach x through that user.  roles='positive' never pushes x down: its
    scores are then too high for the users who do not like it.  An item nobody likes, with roles='positive', keeps V0 / b0."""
    device = _device(device, 'fold_in_items')
    n_users, n_items = len(fue), len(fie)
    uptr, ucols = user_pos if isinstance(user_pos, tuple) else history_csr(user_pos, n_items)
    lptr, lrows = likers if isinstance(likers, tuple) else history_csr(likers, n_users)
    if len(uptr) != n_users + 1:
        raise ValueError('user_pos describes %d users, fue has %d rows' % (len(uptr) - 1, n_users))
    dev = lambda a, **kw: _upload(a, device, **kw)
    out = tkr_hip.fold_in_items(dev(fue, dtype=np.float32), dev(fie, dtype=np.float32), dev(fib, dtype=np.float32, flat=True), dev(uptr), dev(ucols), dev(lptr), dev(lrows),
                                role_thresholds(uptr, lptr, lrows, n_items, roles), li=li, lj=lj, lb=lb, lr=lr, mode=mode, steps=steps,
                                triplets=triplets, seed=seed, first_row=first_row, V0=dev(V0, dtype=np.float32),
                                b0=dev(b0, dtype=np.float32, flat=True), want_loss=want_loss)
    res = (out[0].cpu().numpy(), out[1].cpu().numpy().reshape(-1, 1))
    return res + (out[2].cpu().numpy(),) if want_loss else res
