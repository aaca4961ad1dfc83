"""SMF -- softmax matrix factorisation for implicit feedback, trained on MI355X (K27, csrc/smf.hip): the listwise model -- the
multinomial likelihood of Mult-DAE / Mult-VAE and of sampled-softmax retrieval, here with the FULL softmax -- beside BPR's pairwise
ranking, the squared error of WMF, CER and DPM and LMF's pointwise logistic loss.

    from smf import SMF
    model = SMF(k=30)
    model.load_training_data('data/uid', 'data/vid', 'data/f0tr.txt', seed=0)
    model.train(max_iter=30)
    model.export_embeddings('embed/smf')                     # final-U.dat, final-V.dat, final-B.dat, smf.npz

p(i | u) = softmax_i(x_u . y_i + beta_i) over the WHOLE catalogue: the items of one user compete for probability mass.  With n_u the
likes of user u and lse_u = log sum_i exp(s_ui), the objective is

    F = sum_u (n_u lse_u - sum_{likes of u} s_ui) + 1/2 lam (|X|^2 + |Y|^2 + |beta|^2)

The tables are augmented to k + 1 columns, a user row [x, 1] and an item row [y, beta_i], so a score is one dot product and the bias
is a column like any other; the users' column of ones is never updated.  One iteration is a user half-step and an item half-step of
full-gradient AdaGrad.  The gradient's dense part, sum over ALL rows of the other table of softmax(s) y, is a log-sum-exp pass
(tkr_hip.smf_lse_rows) and a fused kernel -- two chained products on the exact-fp32 MFMA with exp(s - lse) between them, the score
matrix never in memory (tkr_hip.smf_dense_rows); the likes' part, the update and the loss terms are a wave per row
(tkr_hip.smf_step_rows).  There is no sampler and no plan: training is deterministic.  Tables, slots, both like CSRs, the like counts
and their logarithms stay on the device for the loop; one download per iteration carries the loss and the status words.

The model directory serves evaluate.py, recommend.py and fuse.py as BPR's does: final-B.dat holds the item biases.  Both AdaGrad
slots, lam, lr, the seed and the iteration count are kept in smf.npz, so that a second train(model_path=...) continues with its slots.
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

MAX_K = tkr_hip.SMF_MAX_K


def _check_hyper(k, lam, lr):
    if not isinstance(k, (int, np.integer)) or isinstance(k, bool) or not 1 <= k <= MAX_K:
        raise ValueError('SMF: k = %r, 1 <= k <= %d is supported (TKR_SMF_MAX_K: a row block of the gradient lives in the registers of '
                         'one workgroup)' % (k, MAX_K))
    if not (np.isfinite(lam) and lam >= 0):
        raise ValueError('SMF: lam = %r must be finite and not negative' % (lam,))
    if not (np.isfinite(lr) and lr > 0):
        raise ValueError('SMF: lr = %r must be positive and finite' % (lr,))


def _work(work, X, Y):
    """the workspace and the D and lse of X's shape, kept in the dict `work` between calls"""
    k = int(X.shape[1]) - 1
    ws = work['ws'] = tkr_hip.workspace_room(work.get('ws'), tkr_hip.smf_workspace_bytes(int(X.shape[0]), k, int(Y.shape[0])), X.device)
    D = work.get(('D', X.shape))
    if D is None or D.device != X.device:
        D = work[('D', X.shape)] = torch.empty_like(X)
    return ws, D


def user_step(X, H, Y, like_ptr, like_cols, *, lam, lr, heavy_from=None, want_loss=False, work=None):
    """one user half-step in place on X and its slot H against the frozen item table Y, all device tensors [., k + 1] -> (lse fp32
    [n_x] at the X that came in, row_loss float64 [n_x] or None, status).  Nothing is read back"""
    work = {} if work is None else work
    ws, D = _work(work, X, Y)
    lse = tkr_hip.smf_lse_rows(X, Y, workspace=ws)
    tkr_hip.smf_dense_rows(X, Y, row_off=lse, workspace=ws, out=D)
    rows, status = tkr_hip.smf_step_rows(Y, D, like_ptr, like_cols, X, H, fixed=int(X.shape[1]) - 1, scale_by_likes=True, lam=lam, lr=lr,
                                         heavy_from=heavy_from, want_loss=want_loss, workspace=ws, check=False)
    return lse, rows, status


def item_step(Y, H, X, log_n, like_ptr, like_cols, *, lam, lr, heavy_from=None, work=None):
    """one item half-step in place on the item table Y and its slot H against the frozen users X; log_n fp32 [n_users]: the logarithm
    of the users' like counts (-inf for a user without likes: it weighs +0) -> status.  Nothing is read back"""
    work = {} if work is None else work
    ws, _ = _work(work, X, Y)
    off = tkr_hip.smf_lse_rows(X, Y, workspace=ws) - log_n
    ws, D = _work(work, Y, X)
    tkr_hip.smf_dense_rows(Y, X, col_off=off, workspace=ws, out=D)
    return tkr_hip.smf_step_rows(X, D, like_ptr, like_cols, Y, H, fixed=-1, scale_by_likes=False, lam=lam, lr=lr, heavy_from=heavy_from,
                                 workspace=ws, check=False)[1]


class SMF(REC):
    def __init__(self, k: int = 30, lam: float = 0.01, lr: float = 0.1) -> None:
        _check_hyper(k, lam, lr)
        self.__sn = 'smf'
        self.k = int(k)
        self.lam, self.lr = float(lam), float(lr)
        self.uids = self.iids = None
        self.n_users = self.n_items = self.n_likes = None
        self.fue = self.fie = self.fib = None                         # factors [n, k], item biases [n_items, 1]
        self.hu = self.hi = None                                      # the AdaGrad slots, [n_users, k + 1] and [n_items, k + 1]
        self.seed = None
        self.iters_done = 0
        self.losses = []
        self._csr = None                                              # host CSRs: (user ptr, user cols, item ptr, item cols)

    # ------------------------------------------------------------------ data
    def load_training_data(self, uid_file: str, iid_file: str, tr_file: str, seed=None) -> None:
        tprint('Load training data from %s' % (tr_file))
        self.uids = get_id_dict_from_file(uid_file)
        self.iids = get_id_dict_from_file(iid_file)
        self.n_users, self.n_items = len(self.uids), len(self.iids)
        if self.n_users < 1 or self.n_items < 1:
            raise ValueError('SMF: %s / %s list no users or no items' % (uid_file, iid_file))
        R = textio.parse_ratings(tr_file, self.uids, self.iids)
        up, uc = foldin.liked_csr(R, self.n_users, self.n_items, by='user')
        ip, ic = foldin.liked_csr(R, self.n_items, self.n_users, by='item')
        self._csr = (up, uc, ip, ic)
        self.n_likes = int(len(uc))
        rng = np.random.Generator(np.random.PCG64(seed))
        self.seed = seed
        self.fue = rng.standard_normal((self.n_users, self.k), dtype=np.float32) * np.float32(0.01)
        self.fie = rng.standard_normal((self.n_items, self.k), dtype=np.float32) * np.float32(0.01)
        self.fib = np.zeros((self.n_items, 1), dtype=np.float32)
        self.hu = np.ones((self.n_users, self.k + 1), dtype=np.float32)
        self.hi = np.ones((self.n_items, self.k + 1), dtype=np.float32)
        self.iters_done = 0
        tprint('Loading finished!')

    def build_graph(self) -> None:
        tprint('%s does not require build_graph method!' % self.__sn)

    # ------------------------------------------------------------------ the augmented tables
    def _tables(self):
        """-> (users [n_users, k + 1] = [x, 1], items [n_items, k + 1] = [y, beta_i]), fp32 host arrays"""
        k = self.k
        if self.fib is not None and np.size(self.fib) == self.n_items:
            self.fib = np.asarray(self.fib, dtype=np.float32).reshape(-1, 1)
        shapes = (('fue', self.fue, (self.n_users, k)), ('fie', self.fie, (self.n_items, k)), ('fib', self.fib, (self.n_items, 1)),
                  ('hu', self.hu, (self.n_users, k + 1)), ('hi', self.hi, (self.n_items, k + 1)))
        for name, table, shape in shapes:
            if np.shape(table) != shape:
                raise ValueError('SMF: %s has shape %s, the model needs %s' % (name, np.shape(table), shape))
        Xa = np.ones((self.n_users, k + 1), dtype=np.float32)
        Ya = np.empty((self.n_items, k + 1), dtype=np.float32)
        Xa[:, :k] = self.fue
        Ya[:, :k], Ya[:, k] = self.fie, self.fib[:, 0]
        return Xa, Ya

    def _take(self, Xa, Ya, Hx, Hy):
        k = self.k
        Xa, Ya = Xa.cpu().numpy(), Ya.cpu().numpy()
        self.fue = np.ascontiguousarray(Xa[:, :k])
        self.fie, self.fib = np.ascontiguousarray(Ya[:, :k]), np.ascontiguousarray(Ya[:, k:k + 1])
        self.hu, self.hi = Hx.cpu().numpy(), Hy.cpu().numpy()

    # ------------------------------------------------------------------ train
    def train(self, max_iter: int = 30, tol: float = None, model_path: str = None, verbose: bool = True, device=None, heavy_from=None) -> None:
        if self._csr is None:
            raise ValueError('SMF.train: load_training_data() first')
        if model_path is not None and os.path.isdir(model_path):
            self.import_embeddings(model_path)
        device = foldin._device(device, 'SMF.train')
        Xa, Ya = (foldin._upload(t, device, np.float32) for t in self._tables())
        Hx, Hy = foldin._upload(self.hu, device, np.float32), foldin._upload(self.hi, device, np.float32)
        up, uc, ip, ic = (foldin._upload(x, device) for x in self._csr)
        n_u = (up[1:] - up[:-1]).double()                             # the users' like counts, and their logarithms: -inf for none
        log_n = torch.log(n_u.float())
        hyper = dict(lam=self.lam, lr=self.lr, heavy_from=heavy_from, work={})
        loss, self.losses = np.exp(50), []
        for it in range(max_iter):
            t1 = time.time()
            loss_old = loss
            reg = 0.5 * self.lam * Ya.double().square().sum()         # F at the tables entering the iteration
            lse, rows, su = user_step(Xa, Hx, Ya, up, uc, want_loss=True, **hyper)
            total = (n_u * lse.double()).sum() + rows.sum() + reg
            sv = item_step(Ya, Hy, Xa, log_n, ip, ic, **hyper)
            down = torch.cat([total.reshape(1), su.double(), sv.double()]).cpu().numpy()      # one copy: the loss, the status words behind it
            for word, what in zip(down[1:], ('the user step of iteration %d', 'the item step of iteration %d')):
                tkr_hip.status_check('SMF.train, %s' % (what % it), tkr_hip._SMF_REFUSED, tkr_hip.SmfRefused, int(word))
            loss = float(down[0])
            if not np.isfinite(loss):
                raise tkr_hip.TkrError('SMF.train: the loss of iteration %d is %r; lower lr (%g)' % (it, loss, self.lr))
            self.losses.append(loss)
            self.iters_done += 1
            cond = abs(loss_old - loss) / loss_old
            if verbose:
                tprint('Iter %3d, loss %.6f, converge %.6f, time %.2fs' % (it, loss, cond, time.time() - t1))
            if tol is not None and cond < tol:
                break
        self._take(Xa, Ya, Hx, Hy)

    # ------------------------------------------------------------------ fold-in
    def fold_in(self, histories, steps: int = 30, device=None, heavy_from=None):
        """rows for users the model was not trained on, from the items they like: `steps` user half-steps (lse, dense, step) from zero
        rows (slots 1.0) against the frozen item table.  histories: a list of item-index sequences, one per user, or the (ptr, cols)
        pair of foldin.group_history.  -> rows fp32 [n_new, k].  A user without likes only shrinks: its row stays zero"""
        if self.fie is None:
            raise ValueError('SMF.fold_in: load_training_data() and train() first')
        if not isinstance(steps, (int, np.integer)) or isinstance(steps, bool) or steps < 0:
            raise ValueError('SMF.fold_in: steps = %r must be an integer, at least 0' % (steps,))
        device = foldin._device(device, 'SMF.fold_in')
        k = self.k
        ptr, cols = histories if isinstance(histories, tuple) else foldin.history_csr(histories, self.n_items)
        X = torch.zeros((len(ptr) - 1, k + 1), dtype=torch.float32, device=device)
        if len(ptr) == 1:
            return X[:, :k].cpu().numpy()
        X[:, k] = 1
        H = torch.ones_like(X)
        Ya = foldin._upload(self._tables()[1], device, np.float32)
        ptr, cols = foldin._upload(ptr, device), foldin._upload(cols, device)
        work, words = {}, []
        for _ in range(int(steps)):
            words.append(user_step(X, H, Ya, ptr, cols, lam=self.lam, lr=self.lr, heavy_from=heavy_from, work=work)[2])
        X = X.cpu().numpy()
        for word in (torch.cat(words).cpu().numpy() if words else ()):
            tkr_hip.status_check('SMF.fold_in', tkr_hip._SMF_REFUSED, tkr_hip.SmfRefused, int(word))
        return np.ascontiguousarray(X[:, :k])

    # ------------------------------------------------------------------ smf.npz
    def export_model(self, model_path: str) -> None:
        target = os.path.join(model_path, 'smf.npz')
        tprint('Saving AdaGrad slots and hyper-parameters to %s' % target)
        np.savez(target, hu=np.asarray(self.hu, dtype=np.float32), hi=np.asarray(self.hi, dtype=np.float32), lam=np.float64(self.lam),
                 lr=np.float64(self.lr), seed=np.int64(-1 if self.seed is None else self.seed), iters=np.int64(self.iters_done))

    def import_model(self, model_path: str) -> None:
        source = os.path.join(model_path, 'smf.npz')
        if not os.path.exists(source):
            return
        tprint('Loading AdaGrad slots from %s' % source)
        with np.load(source) as z:
            hu, hi = z['hu'].astype(np.float32), z['hi'].astype(np.float32)
            want = ((self.n_users, self.k + 1), (self.n_items, self.k + 1))
            if self.n_users is not None and (hu.shape, hi.shape) != want:
                raise ValueError('SMF: %s holds arrays of shapes %s, the model needs %s' % (source, (hu.shape, hi.shape), want))
            self.hu, self.hi = hu, hi
            self.iters_done = int(z['iters'])
