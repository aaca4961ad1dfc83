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

import numpy as np
import torch

import tkr_hip
from adagrad_mf import AdagradMF, dense_room

MAX_K = tkr_hip.SMF_MAX_K


def _work(work, X, Y):
    """the workspace and the D of X's shape, kept in the dict `work` between calls"""
    return dense_room(work, X, Y, int(X.shape[1]) - 1, tkr_hip.smf_workspace_bytes)


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


class SMF(AdagradMF):
    EXTRA, MAX_K = 1, MAX_K
    REFUSED, RAISES = tkr_hip._SMF_REFUSED, tkr_hip.SmfRefused

    def __init__(self, k: int = 30, lam: float = 0.01, lr: float = 0.1) -> None:
        super().__init__(k, lam, lr)

    # ------------------------------------------------------------------ the augmented tables
    def _tables(self):
        """-> (users [n_users, k + 1] = [x, 1], items [n_items, k + 1] = [y, beta_i]), fp32 host arrays"""
        k = self.k
        self._check_shapes()
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

    # ------------------------------------------------------------------ one iteration: F at the tables entering it, then the two steps
    def _prepare(self, run, heavy_from):
        run.n_u = (run.up[1:] - run.up[:-1]).double()                 # the users' like counts, and their logarithms: -inf for none
        run.log_n = torch.log(run.n_u.float())
        run.hyper = dict(lam=self.lam, lr=self.lr, heavy_from=heavy_from, work={})

    def _iteration(self, run):
        reg = 0.5 * self.lam * run.Ya.double().square().sum()         # F at the tables entering the iteration
        lse, rows, su = user_step(run.Xa, run.Hx, run.Ya, run.up, run.uc, want_loss=True, **run.hyper)
        total = (run.n_u * lse.double()).sum() + rows.sum() + reg
        return total, su, item_step(run.Ya, run.Hy, run.Xa, run.log_n, run.ip, run.ic, **run.hyper)

    # ------------------------------------------------------------------ fold-in
    def fold_in(self, histories, steps: int = 30, device=None, heavy_from=None):
        """rows for users the model was not trained on, from the items they like: `steps` user half-steps (lse, dense, step) from zero
        rows (slots 1.0) against the frozen item table.  histories: a list of item-index sequences, one per user, or the (ptr, cols)
        pair of foldin.group_history.  -> rows fp32 [n_new, k].  A user without likes only shrinks: its row stays zero"""
        return np.ascontiguousarray(self._fold_in(histories, steps, device, heavy_from)[:, :self.k])

    def _fold_start(self, X):
        X[:, self.k] = 1

    def _fold_step(self, X, H, Ya, ptr, cols, heavy_from, work):
        return user_step(X, H, Ya, ptr, cols, lam=self.lam, lr=self.lr, heavy_from=heavy_from, work=work)[2]
