"""WMF and CER -- weighted matrix factorisation for implicit feedback by alternating least squares, and its content-aware form
(collaborative embedding regression), trained on MI355X (K20 and K21, csrc/als.hip).

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

``CER`` (single/cer.py:16-85) is WMF with a prior on every item row, v_j ~ E^T f_j from the item's content features f_j, and a ridge
regression for E behind it:

    model = CER(k=50, d=1024)
    model.load_training_data('data/uid', 'data/vid', 'data/f0tr.txt')
    model.load_content_data('data/meta.pkl', 'data/vid')
    model.train(max_iter=200, tol=1e-4)
    model.export_embeddings('embed/cer')                     # final-U.dat, final-V.dat, final-E.dat
    rows = model.embed_items(new_features)                   # an item that was no line of vid: v = E^T f

    every item j:  (G_U + (a - b) sum_{u in L_j} u u^T + lv I) v = a sum_{u in L_j} u + lv Fe_j,  Fe = F E;  an item without likes too
    E = (lv F^T F + le I)^-1 (lv F^T V)
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
from utils import export_embed_to_file, get_embed_from_file, get_id_dict_from_file, tprint

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


def half_step(X, Y, like_ptr, like_cols, rated_y, *, w=None, ridge_in_G, ridge, a, b, want_loss=False, prior=None, w_prior=0.0):
    """one gram plus one solve, in place on X: G = b sum over the rows rated_y of Y of y y^T + ridge_in_G I, then for every row r of X
    with likes (G + (a - b) sum y y^T + ridge I) x = a sum y.  All arguments device tensors (rated_y int32, or None: every row of Y);
    w: a Work to reuse between calls.  -> (row_loss float64 [n_x] or None, status int64 [2]: the words of the two launches, -1 = nothing
    refused).  Nothing is read back here: the caller looks at the status when it next synchronises (check_status).
    prior (fp32 [n_x, k]) and w_prior: K21 -- the right-hand side of row r adds w_prior prior[r], its loss 1/2 w_prior |x - prior[r]|^2, and
    the rows WITHOUT likes are solved too (tkr_hip.als_solve_rows_prior).  None: the calls above and no others."""
    w = Work() if w is None else w
    n_x, k = int(X.shape[0]), int(Y.shape[1])
    n_listed = int(Y.shape[0]) if rated_y is None else int(rated_y.numel())
    n_likes = int(like_cols.numel())
    need = tkr_hip.als_workspace_bytes(0, k, (n_listed + tkr_hip.ALS_GRAM_SLAB - 1) // tkr_hip.ALS_GRAM_SLAB)
    slabs = None
    if w.heavy_from <= n_likes:
        slabs = w.heavy_slabs(like_ptr)
        need = max(need, tkr_hip.als_workspace_bytes(n_x, k, slabs))
    if prior is not None:
        need = max(need, tkr_hip.als_prior_workspace_bytes(0 if slabs is None else n_x, k, slabs or 0))
    ws = w.room(need, Y.device)
    if w.G is None or w.G.shape != (k, k) or w.G.device != Y.device:
        w.G = torch.empty((k, k), dtype=torch.float32, device=Y.device)
    _, s0 = tkr_hip.als_gram(Y, rated_y, scale=b, ridge=ridge_in_G, workspace=ws, out=w.G, check=False)
    if prior is not None:
        loss, s1 = tkr_hip.als_solve_rows_prior(Y, w.G, like_ptr, like_cols, X, prior, w_like=a - b, w_rhs=a, w_prior=w_prior, ridge=ridge,
                                                heavy_from=w.heavy_from, want_loss=want_loss, workspace=ws, heavy_slabs=slabs, check=False)
        return loss, torch.cat([s0, s1])
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


# ---- CER (K21) ---------------------------------------------------------------------------------------------------------------------------
def cer_train_bytes(n_users, n_items, k, d):
    """device bytes CER.train allocates for a model of this shape -> (dense, tables): dense = 8 (d^2 + n_items d), the fp64 features and
    FF = lv F^T F + le I (factorised in its place); tables = 4 k (n_users + 2 n_items + d), U, V, Fe and E in fp32"""
    n_users, n_items, k, d = int(n_users), int(n_items), int(k), int(d)
    return 8 * (d * d + n_items * d), 4 * k * (n_users + 2 * n_items + d)


class CER(WMF):
    """single/cer.py:16-85.  The start: load_training_data(seed=) draws fue and fie as WMF does, and the SAME generator, carried on,
    draws E standard normal fp32 [d, k] in train() when no final-E.dat was imported -- one seed fixes all three."""

    def __init__(self, k: int, d: int, lu: float = 0.01, lv: float = 10, le: float = 10e3, a: float = 1, b: float = 0.01) -> None:
        super().__init__(k, lu, lv, a, b)
        if not isinstance(d, (int, np.integer)) or d < 1:
            raise ValueError('CER: d = %r, the width of the content features, must be a positive integer' % (d,))
        if not lv > 0:
            raise ValueError('CER: lv = %r must be positive (the weight of the prior v ~ E^T f)' % (lv,))
        if not le > 0:
            raise ValueError('CER: le = %r must be positive (it makes lv F^T F + le I positive definite whatever the features are)' % (le,))
        self.__sn = 'cer'
        self.d, self.le = int(d), float(le)
        self.E = None
        self.feat = None
        self._rng = None

    def load_training_data(self, uid_file: str, iid_file: str, tr_file: str, seed=None) -> None:
        super().load_training_data(uid_file, iid_file, tr_file, seed=seed)
        self._rng = np.random.Generator(np.random.PCG64(seed))                  # carried past the two tables WMF drew: E comes next
        self._rng.random((self.n_users, self.k), dtype=np.float32)
        self._rng.random((self.n_items, self.k), dtype=np.float32)

    def _check_E(self, where):
        if np.shape(self.E) != (self.d, self.k):
            raise ValueError('%s: E has shape %s, the model needs (d, k) = (%d, %d)' % (where, np.shape(self.E), self.d, self.k))

    # ------------------------------------------------------------------ train (cer.py:24-73)
    def train(self, max_iter: int = 200, tol: float = 1e-4, model_path: str = None, verbose: bool = True, device=None, heavy_from=None) -> None:
        if self._csr is None:
            raise ValueError('CER.train: load_training_data() first')
        if self.feat is None:
            raise ValueError('CER.train: load_content_data() first')
        if np.shape(self.feat) != (self.n_items, self.d):
            raise ValueError('CER.train: feat has shape %s, the model needs (%d, %d)' % (np.shape(self.feat), self.n_items, self.d))
        if model_path is not None and os.path.isdir(model_path):
            self.import_embeddings(model_path)
        for name, table, rows in (('fue', self.fue, self.n_users), ('fie', self.fie, self.n_items)):
            if np.shape(table) != (rows, self.k):
                raise ValueError('CER.train: %s has shape %s, the model needs (%d, %d)' % (name, np.shape(table), rows, self.k))
        if self.E is None:
            self.E = self._rng.standard_normal((self.d, self.k), dtype=np.float32)
        self._check_E('CER.train')
        device = foldin._device(device, 'CER.train')
        dense, tables = cer_train_bytes(self.n_users, self.n_items, self.k, self.d)
        free = torch.cuda.mem_get_info(device)[0]
        if dense + tables > free:
            raise ValueError('CER.train: the fp64 features and FF need %d bytes (8 (d^2 + n_items d), d = %d, n_items = %d) and the tables '
                             '%d; %d are free on %s' % (dense, self.d, self.n_items, tables, free, device))
        up, uc, ip, ic = (foldin._upload(x, device) for x in self._csr)
        u_rated = foldin._upload(np.asarray(self.u_rated, dtype=np.int32), device)
        i_rated = foldin._upload(np.asarray(self.i_rated, dtype=np.int32), device)
        U, V = foldin._upload(self.fue, device, np.float32), foldin._upload(self.fie, device, np.float32)
        E = foldin._upload(np.ascontiguousarray(self.E, dtype=np.float32), device, np.float32)
        # the dense linear algebra is the library's, in fp64, rounded once: FF = lv F^T F + le I and its Cholesky factor, once per call
        F = foldin._upload(np.ascontiguousarray(self.feat, dtype=np.float32), device, np.float32).double()
        FF = torch.addmm(torch.eye(self.d, dtype=torch.float64, device=device), F.t(), F, beta=self.le, alpha=self.lv)
        FF = torch.linalg.cholesky(FF)
        w = Work(heavy_from)
        hyper = dict(a=self.a, b=self.b, w=w)
        loss, self.losses = np.exp(50), []
        for it in range(max_iter):
            t1 = time.time()
            loss_old = loss
            Fe = (F @ E.double()).float()
            _, su = half_step(U, V, up, uc, i_rated, ridge_in_G=self.lu, ridge=0.0, **hyper)
            rows, sv = half_step(V, U, ip, ic, u_rated, ridge_in_G=0.0, ridge=self.lv, want_loss=True, prior=Fe, w_prior=self.lv, **hyper)
            E = torch.cholesky_solve(self.lv * (F.t() @ V.double()), FF).float()
            # cer.py:63-65: the new E beside the Fe that entered the solve
            total = rows.sum() + 0.5 * self.lu * U.double().square().sum() + 0.5 * self.le * E.double().square().sum()
            down = torch.cat([total.reshape(1), su.double(), sv.double()]).cpu().numpy()      # one copy: the loss, the four status words behind it
            check_status(down[1:], ('the user step of iteration %d' % it, 'the item step of iteration %d' % it))
            loss = float(down[0])
            self.losses.append(loss)
            cond = abs(loss_old - loss) / loss_old
            if verbose:
                tprint('Iter %3d, loss %.6f, time %.2fs' % (it, loss, time.time() - t1))
            if cond < tol:
                break
        Fe = (F @ E.double()).float()                              # cer.py:70-73: an item without a training like gets its content's row
        cold = np.setdiff1d(np.arange(self.n_items), np.asarray(self.i_rated, dtype=np.int64))
        if len(cold):
            at = foldin._upload(cold.astype(np.int64), device)
            V[at] = Fe[at]
        self.fue, self.fie, self.E = U.cpu().numpy(), V.cpu().numpy(), E.cpu().numpy()

    def embed_items(self, feat):
        """fp32 [m, d] content features -> fp32 [m, k] = feat E, the fp64 product rounded once: the row of an item that was no line of
        vid, by the rule train() gives an item without a training like"""
        if self.E is None:
            raise ValueError('CER.embed_items: train() or import_embeddings() first')
        self._check_E('CER.embed_items')
        feat = np.asarray(feat, dtype=np.float32)
        if feat.ndim != 2 or feat.shape[1] != self.d:
            raise ValueError('CER.embed_items: feat has shape %s, the model needs (m, %d)' % (feat.shape, self.d))
        return (feat.astype(np.float64) @ np.asarray(self.E, dtype=np.float64)).astype(np.float32)

    def export_model(self, model_path: str) -> None:
        if os.path.isdir(model_path) and self.E is not None:
            target = os.path.join(model_path, 'final-E.dat')
            tprint('Saving content projection matrix to %s' % target)
            export_embed_to_file(target, self.E)

    def import_model(self, model_path: str) -> None:
        source = os.path.join(model_path, 'final-E.dat')
        if os.path.exists(source):
            tprint('Loading content projection matrix from %s' % source)
            E = get_embed_from_file(source)
            if np.shape(E) != (self.d, self.k):
                raise ValueError('CER.import_model: %s holds a matrix of shape %s, the model needs (d, k) = (%d, %d)'
                                 % (source, np.shape(E), self.d, self.k))
            self.E = E
