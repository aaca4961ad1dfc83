"""LMF -- logistic matrix factorisation for implicit feedback (Johnson, 2014), trained on MI355X (K25, csrc/lmf.hip): the pointwise
logistic model beside BPR's pairwise ranking and the squared error of WMF, CER and DPM.

    from lmf import LMF
    model = LMF(k=30)
    model.load_training_data('data/uid', 'data/vid', 'data/f0tr.txt', seed=0)
    model.train(max_iter=30)
    model.export_embeddings('embed/lmf')                     # final-U.dat, final-V.dat, final-B.dat, lmf.npz

p(like) = sigma(x_u . y_i + beta_u + beta_i), and the objective sums over EVERY (user, item) pair, not a sample:

    loss = sum_{all u, i} (1 + alpha r_ui) softplus(s_ui) - alpha sum_{likes} s_ui + 1/2 lam (|X|^2 + |beta_u|^2 + |Y|^2 + |beta_i|^2)

The tables are augmented to k + 2 columns, a user row [x, beta_u, 1] and an item row [y, 1, beta_i], so a score is one dot product and
the biases are columns like any other; the column of ones on each side is never updated.  One iteration is a user half-step and an
item half-step of full-gradient AdaGrad.  The gradient's dense part, sum over ALL rows of the other table of sigma(s) y, is a fused
kernel -- two chained products on the exact-fp32 MFMA with sigma between them, the score matrix never in memory
(tkr_hip.lmf_dense_rows); the likes' part, the update and the loss terms are a wave per row (tkr_hip.lmf_step_rows).  There is no
sampler and no plan: training is deterministic.  Tables, slots and both like CSRs stay on the device for the loop; one download per
iteration carries the loss and the status words.

The model directory serves evaluate.py, recommend.py and fuse.py as BPR's does: final-B.dat holds the item biases.  The user bias is
constant along a user's row of scores and changes no ranking, so scoring drops it; it is kept, with both AdaGrad slots, alpha, lam,
lr, the seed and the iteration count, in lmf.npz, so that a second train(model_path=...) continues with its slots.
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

MAX_K = tkr_hip.LMF_MAX_K


def _check_hyper(k, lam, alpha, lr):
    if not isinstance(k, (int, np.integer)) or isinstance(k, bool) or not 1 <= k <= MAX_K:
        raise ValueError('LMF: k = %r, 1 <= k <= %d is supported (TKR_LMF_MAX_K: a row block of the gradient lives in the registers of '
                         'one workgroup)' % (k, MAX_K))
    if not (np.isfinite(lam) and lam >= 0):
        raise ValueError('LMF: lam = %r must be finite and not negative' % (lam,))
    if alpha is not None and not (np.isfinite(alpha) and alpha > 0):
        raise ValueError('LMF: alpha = %r must be positive and finite, or None for the value that balances likes against the rest' % (alpha,))
    if not (np.isfinite(lr) and lr > 0):
        raise ValueError('LMF: lr = %r must be positive and finite' % (lr,))


def balance_alpha(n_users, n_items, n_likes):
    """the weight of a like at which the likes weigh as much as all the other pairs together (the paper's choice)"""
    if n_likes < 1:
        raise ValueError('LMF: the training file holds no like; alpha = None cannot balance the classes')
    return (n_users * n_items - n_likes) / n_likes


def half_step(X, H, Y, like_ptr, like_cols, *, fixed, alpha, lam, lr, heavy_from=None, want_loss=False, work=None):
    """one half-step in place on X and its slot H against the frozen Y, all device tensors [., k + 2] -> (loss terms or None, status):
    the loss terms are a device scalar, sum over the rows of X of (sum over ALL rows of Y of softplus(s)) + alpha sum_likes softplus(s)
    - alpha sum_likes s + 1/2 lam |x non-fixed|^2, at the X that came in.  work: a dict reused between calls (workspace, D).
    Nothing is read back here"""
    work = {} if work is None else work
    k = int(X.shape[1]) - 2
    ws = work['ws'] = tkr_hip.workspace_room(work.get('ws'), tkr_hip.lmf_workspace_bytes(int(X.shape[0]), k, int(Y.shape[0])), X.device)
    D = work.get(('D', X.shape))
    if D is None or D.device != X.device:
        D = work[('D', X.shape)] = torch.empty_like(X)
    out = tkr_hip.lmf_dense_rows(X, Y, want_loss=want_loss, workspace=ws, out=D)
    rows, status = tkr_hip.lmf_step_rows(Y, D, like_ptr, like_cols, X, H, fixed=fixed, alpha=alpha, lam=lam, lr=lr, heavy_from=heavy_from,
                                         want_loss=want_loss, workspace=ws, check=False)
    return (out[1].sum() + rows.sum() if want_loss else None), status


class LMF(REC):
    def __init__(self, k: int = 30, lam: float = 0.6, alpha: float = None, lr: float = 1.0) -> None:
        _check_hyper(k, lam, alpha, lr)
        self.__sn = 'lmf'
        self.k = int(k)
        self.lam, self.lr = float(lam), float(lr)
        self.alpha = None if alpha is None else float(alpha)
        self.alpha_ = self.alpha                                      # the value in use: alpha, or the balance value of the data
        self.uids = self.iids = None
        self.n_users = self.n_items = self.n_likes = None
        self.fue = self.fie = self.fib = self.fub = None              # factors [n, k], item biases [n_items, 1], user biases [n_users]
        self.hu = self.hi = None                                      # the AdaGrad slots, [n_users, k + 2] and [n_items, k + 2]
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
            raise ValueError('LMF: %s / %s list no users or no items' % (uid_file, iid_file))
        R = textio.parse_ratings(tr_file, self.uids, self.iids)
        up, uc = foldin.liked_csr(R, self.n_users, self.n_items, by='user')
        ip, ic = foldin.liked_csr(R, self.n_items, self.n_users, by='item')
        self._csr = (up, uc, ip, ic)
        self.n_likes = int(len(uc))
        self.alpha_ = balance_alpha(self.n_users, self.n_items, self.n_likes) if self.alpha is None else self.alpha
        rng = np.random.Generator(np.random.PCG64(seed))
        self.seed = seed
        self.fue = rng.standard_normal((self.n_users, self.k), dtype=np.float32) * np.float32(0.01)
        self.fie = rng.standard_normal((self.n_items, self.k), dtype=np.float32) * np.float32(0.01)
        self.fub = np.zeros(self.n_users, dtype=np.float32)
        self.fib = np.zeros((self.n_items, 1), dtype=np.float32)
        self.hu = np.ones((self.n_users, self.k + 2), dtype=np.float32)
        self.hi = np.ones((self.n_items, self.k + 2), dtype=np.float32)
        self.iters_done = 0
        tprint('Loading finished!')

    def build_graph(self) -> None:
        tprint('%s does not require build_graph method!' % self.__sn)

    # ------------------------------------------------------------------ the augmented tables
    def _tables(self):
        """-> (users [n_users, k + 2] = [x, beta_u, 1], items [n_items, k + 2] = [y, 1, beta_i]), fp32 host arrays"""
        k = self.k
        if self.fib is not None and np.size(self.fib) == self.n_items:
            self.fib = np.asarray(self.fib, dtype=np.float32).reshape(-1, 1)
        shapes = (('fue', self.fue, (self.n_users, k)), ('fie', self.fie, (self.n_items, k)), ('fib', self.fib, (self.n_items, 1)),
                  ('fub', self.fub, (self.n_users,)), ('hu', self.hu, (self.n_users, k + 2)), ('hi', self.hi, (self.n_items, k + 2)))
        for name, table, shape in shapes:
            if np.shape(table) != shape:
                raise ValueError('LMF: %s has shape %s, the model needs %s' % (name, np.shape(table), shape))
        Xa = np.ones((self.n_users, k + 2), dtype=np.float32)
        Ya = np.ones((self.n_items, k + 2), dtype=np.float32)
        Xa[:, :k], Xa[:, k] = self.fue, self.fub
        Ya[:, :k], Ya[:, k + 1] = self.fie, np.asarray(self.fib, dtype=np.float32).reshape(-1)
        return Xa, Ya

    def _take(self, Xa, Ya, Hx, Hy):
        k = self.k
        Xa, Ya = Xa.cpu().numpy(), Ya.cpu().numpy()
        self.fue, self.fub = np.ascontiguousarray(Xa[:, :k]), np.ascontiguousarray(Xa[:, k])
        self.fie, self.fib = np.ascontiguousarray(Ya[:, :k]), np.ascontiguousarray(Ya[:, k + 1:k + 2])
        self.hu, self.hi = Hx.cpu().numpy(), Hy.cpu().numpy()

    # ------------------------------------------------------------------ train
    def train(self, max_iter: int = 30, tol: float = None, model_path: str = None, verbose: bool = True, device=None, heavy_from=None) -> None:
        if self._csr is None:
            raise ValueError('LMF.train: load_training_data() first')
        if model_path is not None and os.path.isdir(model_path):
            self.import_embeddings(model_path)
        device = foldin._device(device, 'LMF.train')
        k = self.k
        Xa, Ya = (foldin._upload(t, device, np.float32) for t in self._tables())
        Hx, Hy = foldin._upload(self.hu, device, np.float32), foldin._upload(self.hi, device, np.float32)
        up, uc, ip, ic = (foldin._upload(x, device) for x in self._csr)
        hyper = dict(alpha=self.alpha_, lam=self.lam, lr=self.lr, heavy_from=heavy_from, work={})
        loss, self.losses = np.exp(50), []
        for it in range(max_iter):
            t1 = time.time()
            loss_old = loss
            _, su = half_step(Xa, Hx, Ya, up, uc, fixed=k + 1, **hyper)
            part, sv = half_step(Ya, Hy, Xa, ip, ic, fixed=k, want_loss=True, **hyper)
            total = part + 0.5 * self.lam * Xa[:, :k + 1].double().square().sum()
            down = torch.cat([total.reshape(1), su.double(), sv.double()]).cpu().numpy()      # one copy: the loss, the status words behind it
            for word, what in zip(down[1:], ('the user step of iteration %d', 'the item step of iteration %d')):
                tkr_hip.status_check('LMF.train, %s' % (what % it), tkr_hip._LMF_REFUSED, tkr_hip.LmfRefused, int(word))
            loss = float(down[0])
            if not np.isfinite(loss):
                raise tkr_hip.TkrError('LMF.train: the loss of iteration %d is %r; lower lr (%g)' % (it, loss, self.lr))
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
        """rows for users the model was not trained on, from the items they like: `steps` user half-steps from zero (slots 1.0) against
        the frozen item table.  histories: a list of item-index sequences, one per user, or the (ptr, cols) pair of
        foldin.group_history.  -> (rows fp32 [n_new, k], user biases fp32 [n_new]).  A user without likes still steps: it has a gradient"""
        if self.fie is None:
            raise ValueError('LMF.fold_in: load_training_data() and train() first')
        if not isinstance(steps, (int, np.integer)) or isinstance(steps, bool) or steps < 0:
            raise ValueError('LMF.fold_in: steps = %r must be an integer, at least 0' % (steps,))
        device = foldin._device(device, 'LMF.fold_in')
        k = self.k
        ptr, cols = histories if isinstance(histories, tuple) else foldin.history_csr(histories, self.n_items)
        X = torch.zeros((len(ptr) - 1, k + 2), dtype=torch.float32, device=device)
        if len(ptr) == 1:
            return X[:, :k].cpu().numpy(), X[:, k].cpu().numpy()
        X[:, k + 1] = 1
        H = torch.ones_like(X)
        Ya = foldin._upload(self._tables()[1], device, np.float32)
        ptr, cols = foldin._upload(ptr, device), foldin._upload(cols, device)
        work, words = {}, []
        for _ in range(int(steps)):
            words.append(half_step(X, H, Ya, ptr, cols, fixed=k + 1, alpha=self.alpha_, lam=self.lam, lr=self.lr, heavy_from=heavy_from, work=work)[1])
        X = X.cpu().numpy()
        for word in (torch.cat(words).cpu().numpy() if words else ()):
            tkr_hip.status_check('LMF.fold_in', tkr_hip._LMF_REFUSED, tkr_hip.LmfRefused, int(word))
        return np.ascontiguousarray(X[:, :k]), np.ascontiguousarray(X[:, k])

    # ------------------------------------------------------------------ lmf.npz
    def export_model(self, model_path: str) -> None:
        target = os.path.join(model_path, 'lmf.npz')
        tprint('Saving user biases, AdaGrad slots and hyper-parameters to %s' % target)
        np.savez(target, fub=np.asarray(self.fub, dtype=np.float32), hu=np.asarray(self.hu, dtype=np.float32), hi=np.asarray(self.hi, dtype=np.float32),
                 alpha=np.float64(self.alpha_), lam=np.float64(self.lam), lr=np.float64(self.lr),
                 seed=np.int64(-1 if self.seed is None else self.seed), iters=np.int64(self.iters_done))

    def import_model(self, model_path: str) -> None:
        source = os.path.join(model_path, 'lmf.npz')
        if not os.path.exists(source):
            return
        tprint('Loading user biases and AdaGrad slots from %s' % source)
        with np.load(source) as z:
            fub, hu, hi = z['fub'].astype(np.float32), z['hu'].astype(np.float32), z['hi'].astype(np.float32)
            want = ((self.n_users,), (self.n_users, self.k + 2), (self.n_items, self.k + 2))
            if self.n_users is not None and (fub.shape, hu.shape, hi.shape) != want:
                raise ValueError('LMF: %s holds arrays of shapes %s, the model needs %s' % (source, (fub.shape, hu.shape, hi.shape), want))
            self.fub, self.hu, self.hi = fub, hu, hi
            self.iters_done = int(z['iters'])
