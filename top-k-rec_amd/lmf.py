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

import numpy as np

import tkr_hip
from adagrad_mf import AdagradMF, dense_room

MAX_K = tkr_hip.LMF_MAX_K


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
    ws, D = dense_room({} if work is None else work, X, Y, int(X.shape[1]) - 2, tkr_hip.lmf_workspace_bytes)
    out = tkr_hip.lmf_dense_rows(X, Y, want_loss=want_loss, workspace=ws, out=D)
    rows, status = tkr_hip.lmf_step_rows(Y, D, like_ptr, like_cols, X, H, fixed=fixed, alpha=alpha, lam=lam, lr=lr, heavy_from=heavy_from,
                                         want_loss=want_loss, workspace=ws, check=False)
    return (out[1].sum() + rows.sum() if want_loss else None), status


class LMF(AdagradMF):
    EXTRA, MAX_K = 2, MAX_K
    REFUSED, RAISES = tkr_hip._LMF_REFUSED, tkr_hip.LmfRefused
    ARRAYS, ARRAYS_TEXT = ('fub', 'hu', 'hi'), ('user biases', 'AdaGrad slots')
    SCALARS = (('alpha', 'alpha_'), 'lam', 'lr')

    def __init__(self, k: int = 30, lam: float = 0.6, alpha: float = None, lr: float = 1.0) -> None:
        super().__init__(k, lam, lr)
        if alpha is not None and not (np.isfinite(alpha) and alpha > 0):
            raise ValueError('LMF: alpha = %r must be positive and finite, or None for the value that balances likes against the rest' % (alpha,))
        self.alpha = None if alpha is None else float(alpha)
        self.alpha_ = self.alpha                                      # the value in use: alpha, or the balance value of the data
        self.fub = None                                               # user biases [n_users]

    def _on_data(self):
        self.alpha_ = balance_alpha(self.n_users, self.n_items, self.n_likes) if self.alpha is None else self.alpha
        self.fub = np.zeros(self.n_users, dtype=np.float32)

    # ------------------------------------------------------------------ the augmented tables
    def _tables(self):
        """-> (users [n_users, k + 2] = [x, beta_u, 1], items [n_items, k + 2] = [y, 1, beta_i]), fp32 host arrays"""
        k = self.k
        self._check_shapes()
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

    # ------------------------------------------------------------------ one iteration: two half-steps and the regulariser of X
    def _prepare(self, run, heavy_from):
        run.hyper = dict(alpha=self.alpha_, lam=self.lam, lr=self.lr, heavy_from=heavy_from, work={})

    def _iteration(self, run):
        k = self.k
        _, su = half_step(run.Xa, run.Hx, run.Ya, run.up, run.uc, fixed=k + 1, **run.hyper)
        part, sv = half_step(run.Ya, run.Hy, run.Xa, run.ip, run.ic, fixed=k, want_loss=True, **run.hyper)
        return part + 0.5 * self.lam * run.Xa[:, :k + 1].double().square().sum(), su, sv

    # ------------------------------------------------------------------ fold-in
    def fold_in(self, histories, steps: int = 30, device=None, heavy_from=None):
        """rows for users the model was not trained on, from the items they like: `steps` user half-steps from zero (slots 1.0) against
        the frozen item table.  histories: a list of item-index sequences, one per user, or the (ptr, cols) pair of
        foldin.group_history.  -> (rows fp32 [n_new, k], user biases fp32 [n_new]).  A user without likes still steps: it has a gradient"""
        X = self._fold_in(histories, steps, device, heavy_from)
        return np.ascontiguousarray(X[:, :self.k]), np.ascontiguousarray(X[:, self.k])

    def _fold_start(self, X):
        X[:, self.k + 1] = 1

    def _fold_step(self, X, H, Ya, ptr, cols, heavy_from, work):
        return half_step(X, H, Ya, ptr, cols, fixed=self.k + 1, alpha=self.alpha_, lam=self.lam, lr=self.lr, heavy_from=heavy_from, work=work)[1]
