"""WMF -- weighted matrix factorisation for implicit feedback by alternating least squares, trained on MI355X (K20, csrc/als.hip).

    from als import WMF
    model = WMF(k=50)
    model.load_training_data('data/uid', 'data/vid', 'data/f0tr.txt')
    model.train(max_iter=200, tol=1e-4)
    model.export_embeddings('embed/wmf')

The class API of the reference's single/wmf.py:10-107 (train.py:18-22).  Its train() cannot run -- wmf.py:75,86 call .keys() on lists --
so the semantics are those of dpm.py:36-58, the same algebra on the same lists with every stored like r = 1:

    G_V = b sum_{i rated} v v^T + lu I;   every user u with likes:  (G_V + (a - b) sum_{i in L_u} v v^T) u = a sum_{i in L_u} v
    G_U = b sum_{u rated} u u^T;          every item i with likes:  (G_U + (a - b) sum_{u in L_i} u u^T + lv I) v = a sum_{u in L_i} u

The two shared Grams and the per-row Gram + Cholesky solve are HIP kernels; the tables and both like CSRs stay on the device for the
whole loop, and one scalar (the loss, with the kernels' status words behind it) comes down per iteration.  ``single.WMF`` still raises:
the reference's package surface is pinned as it is, this class lives here.  What it writes (final-U.dat, final-V.dat, no final-B.dat)
is a model directory like any other to evaluate.py, recommend.py and fuse.py.
"""
from __future__ import annotations

import os
import time

import numpy as np
import torch

import foldin
import textio
import tkr_hip
from single.rec import REC
from utils import get_id_dict_from_file, tprint

MAX_K = tkr_hip.ALS_MAX_K


class Work:
    """what a half-step keeps between calls on one device: the workspace of both launches, the Gram, and the slabs the heavy rows of
    each CSR have (counted once on the host, from the CSR the caller built there)"""

    def __init__(self, heavy_from=None):
        self.heavy_from = tkr_hip.ALS_HEAVY_FROM if heavy_from is None else int(heavy_from)
        self.workspace = None
        self.G = None
        self._slabs = {}

    def heavy_slabs(self, like_ptr):
        key = (like_ptr.data_ptr(), like_ptr.numel())
        if key not in self._slabs:
            self._slabs[key] = tkr_hip.als_heavy_slabs(like_ptr, self.heavy_from)
        return self._slabs[key]

    def room(self, need, device):
        if self.workspace is None or self.workspace.device != device or self.workspace.numel() * 8 < need:
            self.workspace = torch.empty(max(need, 16) // 8 + 1, dtype=torch.int64, device=device)
        return self.workspace


def half_step(X, Y, like_ptr, like_cols, rated_y, *, w=None, ridge_in_G, ridge, a, b, want_loss=False):
    """one gram plus one solve, in place on X: G = b sum over the rows rated_y of Y of y y^T + ridge_in_G I, then for every row r of X
    with likes (G + (a - b) sum y y^T + ridge I) x = a sum y.  All arguments device tensors (rated_y int32, or None: every row of Y);
    w: a Work to reuse between calls.  -> (row_loss float64 [n_x] or None, status int64 [2]: the words of the two launches, -1 = nothing
    refused).  Nothing is read back here: the caller looks at the status when it next synchronises (check_status)."""
    w = Work() if w is None else w
    n_x, k = int(X.shape[0]), int(Y.shape[1])
    n_listed = int(Y.shape[0]) if rated_y is None else int(rated_y.numel())
    n_likes = int(like_cols.numel())
    need = tkr_hip.als_workspace_bytes(0, k, (n_listed + tkr_hip.ALS_GRAM_SLAB - 1) // tkr_hip.ALS_GRAM_SLAB)
    slabs = None
    if w.heavy_from <= n_likes:
        slabs = w.heavy_slabs(like_ptr)
        need = max(need, tkr_hip.als_workspace_bytes(n_x, k, slabs))
    ws = w.room(need, Y.device)
    if w.G is None or w.G.shape != (k, k) or w.G.device != Y.device:
        w.G = torch.empty((k, k), dtype=torch.float32, device=Y.device)
    _, s0 = tkr_hip.als_gram(Y, rated_y, scale=b, ridge=ridge_in_G, workspace=ws, out=w.G, check=False)
    loss, s1 = tkr_hip.als_solve_rows(Y, w.G, like_ptr, like_cols, X, w_like=a - b, w_rhs=a, ridge=ridge, heavy_from=w.heavy_from,
                                      want_loss=want_loss, workspace=ws, heavy_slabs=slabs, check=False)
    return loss, torch.cat([s0, s1])


def check_status(words, what):
    """words: the status words of half-steps, as integers, (gram, solve) pairs in call order; raises for the first that is not -1"""
    for i, word in enumerate(words):
        word = int(word)
        if word != -1:
            raise tkr_hip.AlsRefused('%s, %s' % (what[i // 2], 'als_solve_rows' if i & 1 else 'als_gram (row = position in the rated list)'), word)


def _check_hyper(k, lu, lv, a, b):
    if not isinstance(k, (int, np.integer)) or not 1 <= k <= MAX_K:
        raise ValueError('WMF: k = %r, 1 <= k <= %d is supported (TKR_ALS_MAX_K: the k x k system of a row lives in the LDS of one '
                         'workgroup)' % (k, MAX_K))
    if not b > 0:
        raise ValueError('WMF: b = %r must be positive (the weight of an unobserved pair)' % (b,))
    if not a > b:
        raise ValueError('WMF: a = %r must exceed b = %r (a like weighs more than an unobserved pair)' % (a, b))
    if not (lu >= 0 and lv >= 0):
        raise ValueError('WMF: lu = %r and lv = %r must not be negative' % (lu, lv))


class WMF(REC):
    def __init__(self, k: int, lu: float = 0.01, lv: float = 0.01, a: float = 1, b: float = 0.01) -> None:
        _check_hyper(k, lu, lv, a, b)
        self.__sn = 'wmf'
        self.k = int(k)
        self.lu, self.lv, self.a, self.b = float(lu), float(lv), float(a), float(b)
        self.uids = self.iids = None
        self.n_users = self.n_items = self.n_ratings = None
        self.u_rated = self.i_rated = None
        self.fue = self.fie = None
        self.losses = []
        self._csr = None            # host CSRs: (user ptr, user cols, item ptr, item cols)

    # ------------------------------------------------------------------ data (wmf.py:32-56)
    def load_training_data(self, uid_file: str, iid_file: str, tr_file: str, seed=None) -> None:
        tprint('Load training data from %s' % (tr_file))
        self.uids = get_id_dict_from_file(uid_file)
        self.iids = get_id_dict_from_file(iid_file)
        self.n_users, self.n_items = len(self.uids), len(self.iids)
        if self.n_users < 1 or self.n_items < 1:
            raise ValueError('WMF: %s / %s list no users or no items' % (uid_file, iid_file))
        self.n_ratings = self.n_users * self.n_items
        R = textio.parse_ratings(tr_file, self.uids, self.iids)
        up, uc = foldin.liked_csr(R, self.n_users, self.n_items, by='user')
        ip, ic = foldin.liked_csr(R, self.n_items, self.n_users, by='item')
        self._csr = (up, uc, ip, ic)
        self.u_rated = np.flatnonzero(np.diff(up) > 0).tolist()
        self.i_rated = np.flatnonzero(np.diff(ip) > 0).tolist()
        rng = np.random.Generator(np.random.PCG64(seed))
        self.fue = rng.random((self.n_users, self.k), dtype=np.float32)
        self.fie = rng.random((self.n_items, self.k), dtype=np.float32)
        tprint('Loading finished!')

    def build_graph(self) -> None:
        tprint('%s does not require build_graph method!' % self.__sn)

    # ------------------------------------------------------------------ train (wmf.py:61-101)
    def train(self, max_iter: int = 200, tol: float = 1e-4, model_path: str = None, verbose: bool = True, device=None, heavy_from=None) -> None:
        if self._csr is None:
            raise ValueError('WMF.train: load_training_data() first')
        if model_path is not None and os.path.isdir(model_path):
            self.import_embeddings(model_path)
        for name, table, rows in (('fue', self.fue, self.n_users), ('fie', self.fie, self.n_items)):
            if np.shape(table) != (rows, self.k):
                raise ValueError('WMF.train: %s has shape %s, the model needs (%d, %d)' % (name, np.shape(table), rows, self.k))
        device = foldin._device(device, 'WMF.train')
        up, uc, ip, ic = (foldin._upload(x, device) for x in self._csr)
        u_rated = foldin._upload(np.asarray(self.u_rated, dtype=np.int32), device)
        i_rated = foldin._upload(np.asarray(self.i_rated, dtype=np.int32), device)
        U, V = foldin._upload(self.fue, device, np.float32), foldin._upload(self.fie, device, np.float32)
        w = Work(heavy_from)
        hyper = dict(a=self.a, b=self.b, w=w)
        loss, self.losses = np.exp(50), []
        for it in range(max_iter):
            t1 = time.time()
            loss_old = loss
            _, su = half_step(U, V, up, uc, i_rated, ridge_in_G=self.lu, ridge=0.0, **hyper)
            rows, sv = half_step(V, U, ip, ic, u_rated, ridge_in_G=0.0, ridge=self.lv, want_loss=True, **hyper)
            total = rows.sum() + 0.5 * self.lu * U.double().square().sum() + 0.5 * self.lv * V.double().square().sum()
            down = torch.cat([total.reshape(1), su.double(), sv.double()]).cpu().numpy()      # one copy: the loss, the four status words behind it
            check_status(down[1:], ('the user step of iteration %d' % it, 'the item step of iteration %d' % it))
            loss = float(down[0])
            self.losses.append(loss)
            cond = abs(loss_old - loss) / loss_old
            if verbose:
                tprint('Iter %3d, loss %.6f, converge %.6f, time %.2fs' % (it, loss, cond, time.time() - t1))
            if cond < tol:
                break
        self.fue, self.fie = U.cpu().numpy(), V.cpu().numpy()

    # ------------------------------------------------------------------ fold-in (new: the reference can only retrain)
    def fold_in(self, histories, device=None, heavy_from=None):
        """rows for users who were not in the training file, from the items they like: one user half-step against the trained item
        table (the kernel of train()).  histories: a list of item-index sequences, one per user, or the (ptr, cols) pair of
        foldin.group_history.  -> fp32 [n_new, k]; a user without likes gets a row of zeros"""
        if self.fie is None or self._csr is None:
            raise ValueError('WMF.fold_in: load_training_data() and train() first')
        device = foldin._device(device, 'WMF.fold_in')
        ptr, cols = histories if isinstance(histories, tuple) else foldin.history_csr(histories, self.n_items)
        X = torch.zeros((len(ptr) - 1, self.k), dtype=torch.float32, device=device)
        if len(ptr) == 1:
            return X.cpu().numpy()
        _, status = half_step(X, foldin._upload(self.fie, device, np.float32), foldin._upload(ptr, device), foldin._upload(cols, device),
                              foldin._upload(np.asarray(self.i_rated, dtype=np.int32), device), w=Work(heavy_from), ridge_in_G=self.lu, ridge=0.0,
                              a=self.a, b=self.b)
        check_status(status.cpu().numpy(), ('fold_in',))
        return X.cpu().numpy()

    def export_model(self, model_path: str) -> None:
        return

    def import_model(self, model_path: str) -> None:
        return
