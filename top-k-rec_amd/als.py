"""WMF, CER and DPM -- weighted matrix factorisation for implicit feedback by alternating least squares, and its two content-aware
forms (collaborative embedding regression: a linear map of the item's features; DPM: an MLP on them), trained on MI355X (K20 and K21,
csrc/als.hip; K22, csrc/mlp.hip).

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

``WMF(k, ..., solver='cg', cg_steps=3)`` (K24, csrc/als_cg.hip and the wide Gram of csrc/als.hip; the same keywords on CER and DPM)
takes cg_steps steps of conjugate gradients per row and half-step from the row's previous value in place of the per-row Gram + Cholesky: no k x k matrix per row, so
k <= 512 for WMF and CER.  The default, 'cholesky', is the path above with its bits and its bound k <= 128.

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

``CER(k, d, ..., estep='cg', e_steps=8)`` (K26, csrc/sparse.hip) keeps the features sparse from the pickle to the device: feat is a
canonical fp32 scipy.sparse.csr_matrix, F and F^T are CSRs on the GPU, Fe = F E is one sparse x dense product and the E-step takes
e_steps steps of conjugate gradients on (lv F^T F + le I) E = lv F^T V from the E of the iteration before.  Nothing of size d x d or
n_items x d exists, so d = 200,000 trains (cer_sparse_train_bytes).  The default, 'cholesky', is the dense path above with its bits.

``DPM`` (single/dpm.py:10-76) puts ``MLP`` (single/mlp.py), a dense network d -> 2000 -> 1000 -> k with sigmoid hidden layers, where CER
has E: the prior of item j is encoder(f_j), and after every alternation the encoder takes one epoch of mini-batch RMSProp towards the
item table:

    model = DPM(k=50, d=20000)
    model.load_training_data('data/uid', 'data/vid', 'data/f0tr.txt')
    model.load_content_data('data/meta.pkl', 'data/vid')
    model.train(MLP, max_iter=200)
    model.export_embeddings('embed/dpm')                     # final-U.dat, final-V.dat, mlp.npz (the encoder, exact fp32)
    rows = model.embed_items(new_features)
"""
from __future__ import annotations

import os
import time
import types

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
        self.workspace = tkr_hip.workspace_room(self.workspace, need, device)
        return self.workspace

    def gram(self, k, device):
        if self.G is None or self.G.shape != (k, k) or self.G.device != device:
            self.G = torch.empty((k, k), dtype=torch.float32, device=device)
        return self.G


def half_step(X, Y, like_ptr, like_cols, rated_y, *, w=None, ridge_in_G, ridge, a, b, want_loss=False, prior=None, w_prior=0.0,
              solver='cholesky', cg_steps=tkr_hip.ALS_CG_STEPS):
    """one gram plus one solve, in place on X: G = b sum over the rows rated_y of Y of y y^T + ridge_in_G I, then for every row r of X
    with likes (G + (a - b) sum y y^T + ridge I) x = a sum y.  All arguments device tensors (rated_y int32, or None: every row of Y);
    w: a Work to reuse between calls.  -> (row_loss float64 [n_x] or None, status int64 [2]: the words of the two launches, -1 = nothing
    refused).  Nothing is read back here: the caller looks at the status when it next synchronises (check_status).
    prior (fp32 [n_x, k]) and w_prior: K21 -- the right-hand side of row r adds w_prior prior[r], its loss 1/2 w_prior |x - prior[r]|^2, and
    the rows WITHOUT likes are solved too (tkr_hip.als_solve_rows_prior).  None: the calls above and no others.
    solver 'cg' (K24): the same system by cg_steps steps of conjugate gradients from the value X holds, k up to tkr_hip.ALS_CG_MAX_K
    (tkr_hip.als_gram_wide + tkr_hip.als_cg_rows); the default takes the calls above and no others."""
    w = Work() if w is None else w
    n_x, k = int(X.shape[0]), int(Y.shape[1])
    n_listed = int(Y.shape[0]) if rated_y is None else int(rated_y.numel())
    n_slabs = (n_listed + tkr_hip.ALS_GRAM_SLAB - 1) // tkr_hip.ALS_GRAM_SLAB
    if solver == 'cg':
        ws = w.room(tkr_hip.als_gram_wide_workspace_bytes(k, n_slabs), Y.device)
        gram, solve, more = tkr_hip.als_gram_wide, tkr_hip.als_cg_rows, dict(steps=int(cg_steps), prior=prior, w_prior=w_prior)
    elif solver == 'cholesky':
        need = tkr_hip.als_workspace_bytes(0, k, n_slabs)
        slabs = None
        if w.heavy_from <= int(like_cols.numel()):
            slabs = w.heavy_slabs(like_ptr)
            need = max(need, tkr_hip.als_workspace_bytes(n_x, k, slabs))
        if prior is not None:
            need = max(need, tkr_hip.als_prior_workspace_bytes(0 if slabs is None else n_x, k, slabs or 0))
        ws = w.room(need, Y.device)
        gram, solve, more = tkr_hip.als_gram, tkr_hip.als_solve_rows, dict(heavy_from=w.heavy_from, workspace=ws, heavy_slabs=slabs)
        if prior is not None:
            solve, more = tkr_hip.als_solve_rows_prior, dict(more, prior=prior, w_prior=w_prior)
    else:
        raise ValueError("half_step: solver = %r, 'cholesky' and 'cg' are the ones there are" % (solver,))
    _, s0 = gram(Y, rated_y, scale=b, ridge=ridge_in_G, workspace=ws, out=w.gram(k, Y.device), check=False)
    loss, s1 = solve(Y, w.G, like_ptr, like_cols, X, w_like=a - b, w_rhs=a, ridge=ridge, want_loss=want_loss, check=False, **more)
    return loss, torch.cat([s0, s1])


def check_status(words, what):
    """words: the status words of half-steps, as integers, (gram, solve) pairs in call order; raises for the first that is not -1"""
    for i, word in enumerate(words):
        tkr_hip.status_check('%s, %s' % (what[i // 2], 'als_solve_rows' if i & 1 else 'als_gram (row = position in the rated list)'),
                             tkr_hip._ALS_REFUSED, tkr_hip.AlsRefused, int(word))


SOLVERS = ('cholesky', 'cg')
CG_MAX_K = tkr_hip.ALS_CG_MAX_K


def _check_hyper(k, lu, lv, a, b, solver='cholesky', cg_steps=tkr_hip.ALS_CG_STEPS):
    if solver not in SOLVERS:
        raise ValueError("WMF: solver = %r, 'cholesky' (per-row Gram + Cholesky, K20) and 'cg' (conjugate gradients, K24) are the ones "
                         'there are' % (solver,))
    if not isinstance(cg_steps, (int, np.integer)) or isinstance(cg_steps, bool) or cg_steps < 1:
        raise ValueError('WMF: cg_steps = %r must be an integer, at least 1' % (cg_steps,))
    if solver == 'cg':
        if not isinstance(k, (int, np.integer)) or not 1 <= k <= CG_MAX_K:
            raise ValueError("WMF: k = %r, 1 <= k <= %d is supported under solver='cg' (TKR_ALS_CG_MAX_K: a row's x and r are 8 registers "
                             'per lane each)' % (k, CG_MAX_K))
    elif not isinstance(k, (int, np.integer)) or not 1 <= k <= MAX_K:
        raise ValueError('WMF: k = %r, 1 <= k <= %d is supported (TKR_ALS_MAX_K: the k x k system of a row lives in the LDS of one '
                         'workgroup)' % (k, MAX_K))
    if not b > 0:
        raise ValueError('WMF: b = %r must be positive (the weight of an unobserved pair)' % (b,))
    if not a > b:
        raise ValueError('WMF: a = %r must exceed b = %r (a like weighs more than an unobserved pair)' % (a, b))
    if not (lu >= 0 and lv >= 0):
        raise ValueError('WMF: lu = %r and lv = %r must not be negative' % (lu, lv))


class WMF(REC):
    def __init__(self, k: int, lu: float = 0.01, lv: float = 0.01, a: float = 1, b: float = 0.01, *, solver: str = 'cholesky',
                 cg_steps: int = tkr_hip.ALS_CG_STEPS) -> None:
        _check_hyper(k, lu, lv, a, b, solver, cg_steps)
        self.__sn = 'wmf'
        self.k = int(k)
        self.solver, self.cg_steps = solver, int(cg_steps)
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
        self._need_data('WMF.train')
        self._train('WMF.train', max_iter, tol, model_path, verbose, device, heavy_from)

    def _need_data(self, who):
        if self._csr is None:
            raise ValueError('%s: load_training_data() first' % who)

    # The one training loop of WMF, CER and DPM.  What the content-aware models add goes through the hooks below; `run` is the device
    # state of one call: device, U, V and what _prepare puts beside them.
    def _train(self, who, max_iter, tol, model_path, verbose, device, heavy_from, **options):
        if model_path is not None and os.path.isdir(model_path):
            self.import_embeddings(model_path)
        for name, table, rows in (('fue', self.fue, self.n_users), ('fie', self.fie, self.n_items)):
            if np.shape(table) != (rows, self.k):
                raise ValueError('%s: %s has shape %s, the model needs (%d, %d)' % (who, name, np.shape(table), rows, self.k))
        run = self._prepare(who, device, **options)
        device = run.device
        up, uc, ip, ic = (foldin._upload(x, device) for x in self._csr)
        u_rated = foldin._upload(np.asarray(self.u_rated, dtype=np.int32), device)
        i_rated = foldin._upload(np.asarray(self.i_rated, dtype=np.int32), device)
        U, V = run.U, run.V = foldin._upload(self.fue, device, np.float32), foldin._upload(self.fie, device, np.float32)
        hyper = dict(a=self.a, b=self.b, w=Work(heavy_from), solver=self.solver, cg_steps=self.cg_steps)
        steps = ('the user step of iteration %d', 'the item step of iteration %d')
        loss, self.losses = np.exp(50), []
        for it in range(max_iter):
            t1 = time.time()
            loss_old = loss
            prior = self._prior(run)
            _, su = half_step(U, V, up, uc, i_rated, ridge_in_G=self.lu, ridge=0.0, **hyper)
            rows, sv = half_step(V, U, ip, ic, u_rated, ridge_in_G=0.0, ridge=self.lv, want_loss=True, **prior, **hyper)
            term, words = self._after_steps(run)
            total = rows.sum() + 0.5 * self.lu * U.double().square().sum() + term
            down = torch.cat([total.reshape(1), su.double(), sv.double()] + [x.double() for x in words]).cpu().numpy()      # one copy: the loss, the status words behind it
            check_status(down[1:5], tuple(x % it for x in steps))
            loss = float(down[0])
            self._check_iteration(who, it, loss, down[5:])
            self.losses.append(loss)
            cond = abs(loss_old - loss) / loss_old if self.STOPS_ON_TOL else None
            if verbose:
                tprint('Iter %3d, loss %.6f, %stime %.2fs' % (it, loss, 'converge %.6f, ' % cond if self.LOGS_CONVERGE else '', time.time() - t1))
            if self.STOPS_ON_TOL and cond < tol:
                break
        Fe = self._cold_rows(run)
        if Fe is not None:
            cold = np.setdiff1d(np.arange(self.n_items), np.asarray(self.i_rated, dtype=np.int64))
            if len(cold):
                at = foldin._upload(cold.astype(np.int64), device)
                V[at] = Fe[at]
        self.fue, self.fie = U.cpu().numpy(), V.cpu().numpy()

    STOPS_ON_TOL = LOGS_CONVERGE = True                            # the stopping test on tol; `converge` in the log line

    def _prepare(self, who, device):
        """-> the run: its device, and whatever else the model keeps on it for the loop (checked and uploaded here)"""
        return types.SimpleNamespace(device=foldin._device(device, who))

    def _prior(self, run):
        """at the head of an iteration -> the keywords of the item half-step: none, or prior and w_prior"""
        return {}

    def _after_steps(self, run):
        """behind the two half-steps -> (the model's own term of the loss, a device scalar; its own status words, a list of tensors)"""
        return 0.5 * self.lv * run.V.double().square().sum(), []

    def _check_iteration(self, who, it, loss, words):
        """the downloaded loss and the words of _after_steps: raises where they say the iteration failed"""

    def _cold_rows(self, run):
        """behind the loop -> the table whose rows the items without a training like get, or None: they stay as they are"""
        return None

    # ------------------------------------------------------------------ fold-in (new: the reference can only retrain)
    def fold_in(self, histories, device=None, heavy_from=None, steps=None):
        """rows for users who were not in the training file, from the items they like: one user half-step against the trained item
        table (the kernel of train()).  histories: a list of item-index sequences, one per user, or the (ptr, cols) pair of
        foldin.group_history.  -> fp32 [n_new, k]; a user without likes gets a row of zeros.  steps (solver='cg' only): the rows start
        from zero, not from a trained value, so the default is k steps, the bound at which conjugate gradients end in exact arithmetic;
        a row whose residual is gone (rho < 1e-20) stops sooner"""
        if steps is not None and (self.solver != 'cg' or not isinstance(steps, (int, np.integer)) or steps < 1):
            raise ValueError("WMF.fold_in: steps = %r is the step count of solver='cg', an integer of at least 1" % (steps,))
        if self.fie is None or self._csr is None:
            raise ValueError('WMF.fold_in: load_training_data() and train() first')
        device = foldin._device(device, 'WMF.fold_in')
        ptr, cols = histories if isinstance(histories, tuple) else foldin.history_csr(histories, self.n_items)
        X = torch.zeros((len(ptr) - 1, self.k), dtype=torch.float32, device=device)
        if len(ptr) == 1:
            return X.cpu().numpy()
        _, status = half_step(X, foldin._upload(self.fie, device, np.float32), foldin._upload(ptr, device), foldin._upload(cols, device),
                              foldin._upload(np.asarray(self.i_rated, dtype=np.int32), device), w=Work(heavy_from), ridge_in_G=self.lu, ridge=0.0,
                              a=self.a, b=self.b, solver=self.solver, cg_steps=self.k if steps is None else int(steps))
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


def cer_sparse_train_bytes(n_users, n_items, k, d, nnz):
    """device bytes CER.train allocates under estep='cg' -> (sparse, tables, workspace): sparse = 16 nnz + 8 (n_items + d + 2), the CSR
    of the features and of their transpose (int64 ptr, int32 col, fp32 val each); tables = 4 k (n_users + 2 n_items + d), U, V, Fe and E
    in fp32; workspace = tkr_hip.estep_cg_workspace_bytes(n_items, d, k), the E-step's: T = F P [n_items, k], five tables of E's shape
    (B, R, P, Q and the E being built), two [ceil(d / 1024), k] tables of dot-product partials and the list of heavy rows.  Nothing
    grows with d^2 or n_items d"""
    n_users, n_items, k, d, nnz = int(n_users), int(n_items), int(k), int(d), int(nnz)
    return 16 * nnz + 8 * (n_items + d + 2), 4 * k * (n_users + 2 * n_items + d), tkr_hip.estep_cg_workspace_bytes(n_items, d, k)


ESTEPS = ('cholesky', 'cg')
ESTEP_HEAVY_FROM = 512      # the E-step's heavy_from: a row of F^T with more nonzeros gets a workgroup (scripts/time_cer_sparse.py; tkr_hip's default is 2,048)


def canonical_csr(feat):
    """a scipy.sparse matrix or a dense array -> the canonical fp32 scipy.sparse.csr_matrix of it: ascending columns, no duplicates, no
    stored zeros (a copy: the argument is left as it is)"""
    import scipy.sparse as ss
    m = ss.csr_matrix(feat, dtype=np.float32, copy=True) if ss.issparse(feat) else ss.csr_matrix(np.asarray(feat, dtype=np.float32))
    m.sum_duplicates()
    m.eliminate_zeros()
    m.sort_indices()
    return m


def _need_content(model, who):
    if model.feat is None:
        raise ValueError('%s: load_content_data() first' % who)
    if np.shape(model.feat) != (model.n_items, model.d):
        raise ValueError('%s: feat has shape %s, the model needs (%d, %d)' % (who, np.shape(model.feat), model.n_items, model.d))


class CER(WMF):
    """single/cer.py:16-85.  The start: load_training_data(seed=) draws fue and fie as WMF does, and the SAME generator, carried on,
    draws E standard normal fp32 [d, k] in train() when no final-E.dat was imported -- one seed fixes all three."""

    def __init__(self, k: int, d: int, lu: float = 0.01, lv: float = 10, le: float = 10e3, a: float = 1, b: float = 0.01, *,
                 solver: str = 'cholesky', cg_steps: int = tkr_hip.ALS_CG_STEPS, estep: str = 'cholesky', e_steps: int = tkr_hip.ESTEP_STEPS) -> None:
        super().__init__(k, lu, lv, a, b, solver=solver, cg_steps=cg_steps)
        if estep not in ESTEPS:
            raise ValueError("CER: estep = %r, 'cholesky' (a dense d x d factor, K21) and 'cg' (conjugate gradients on the sparse features, "
                             'K26) are the ones there are' % (estep,))
        if not isinstance(e_steps, (int, np.integer)) or isinstance(e_steps, bool) or e_steps < 1:
            raise ValueError('CER: e_steps = %r must be an integer, at least 1' % (e_steps,))
        self.estep, self.e_steps = estep, int(e_steps)
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

    def load_content_data(self, content_file: str, iid_file: str) -> None:
        """estep='cg': the features stay sparse -- self.feat is the canonical fp32 scipy.sparse.csr_matrix [n_items, d] with the rows
        placed at the model's item indices as the dense loader places them (a dense pickle is converted; for a sparse one nothing of
        size n_items x d is allocated).  estep='cholesky': REC's dense loader, as it is"""
        if self.estep != 'cg':
            return super().load_content_data(content_file, iid_file)
        import pickle
        import scipy.sparse as ss
        tprint('Load content data from %s' % (content_file))
        feature_ids = get_id_dict_from_file(iid_file)
        with open(content_file, 'rb') as fh:
            raw = pickle.load(fh, encoding='latin1')
        dst = np.asarray([idx for iid, idx in self.iids.items() if iid in feature_ids], dtype=np.int64)
        src = [feature_ids[iid] for iid in self.iids if iid in feature_ids]
        sub = (raw.tocsr()[src, :] if ss.issparse(raw) else ss.csr_matrix(np.asarray(raw)[src, :])).tocoo()
        if sub.shape[1] != self.d:
            raise ValueError('CER.load_content_data: %s holds features of width %d, the model needs d = %d' % (content_file, sub.shape[1], self.d))
        self.feat = canonical_csr(ss.coo_matrix((sub.data, (dst[sub.row], sub.col)), shape=(self.n_items, self.d)))
        tprint('Loading finished!')

    def _check_E(self, where):
        if np.shape(self.E) != (self.d, self.k):
            raise ValueError('%s: E has shape %s, the model needs (d, k) = (%d, %d)' % (where, np.shape(self.E), self.d, self.k))

    # ------------------------------------------------------------------ train (cer.py:24-73)
    def train(self, max_iter: int = 200, tol: float = 1e-4, model_path: str = None, verbose: bool = True, device=None, heavy_from=None) -> None:
        self._need_data('CER.train')
        _need_content(self, 'CER.train')
        self._train('CER.train', max_iter, tol, model_path, verbose, device, heavy_from)

    def _prepare(self, who, device):
        if self.E is None:
            self.E = self._rng.standard_normal((self.d, self.k), dtype=np.float32)
        self._check_E(who)
        device = foldin._device(device, who)
        if self.estep == 'cg':
            return self._prepare_sparse(who, device)
        dense, tables = cer_train_bytes(self.n_users, self.n_items, self.k, self.d)
        free = torch.cuda.mem_get_info(device)[0]
        if dense + tables > free:
            raise ValueError('%s: the fp64 features and FF need %d bytes (8 (d^2 + n_items d), d = %d, n_items = %d) and the tables '
                             '%d; %d are free on %s' % (who, dense, self.d, self.n_items, tables, free, device))
        E = foldin._upload(np.ascontiguousarray(self.E, dtype=np.float32), device, np.float32)
        # the dense linear algebra is the library's, in fp64, rounded once: FF = lv F^T F + le I and its Cholesky factor, once per call
        F = foldin._upload(np.ascontiguousarray(self.feat, dtype=np.float32), device, np.float32).double()
        FF = torch.addmm(torch.eye(self.d, dtype=torch.float64, device=device), F.t(), F, beta=self.le, alpha=self.lv)
        return types.SimpleNamespace(device=device, E=E, F=F, FF=torch.linalg.cholesky(FF))

    def _prepare_sparse(self, who, device):
        """estep='cg' (K26): F and F^T as CSRs on the device, the transpose taken once on the host; nothing of size d^2 or n_items d"""
        feat = canonical_csr(self.feat)
        sparse, tables, ws = cer_sparse_train_bytes(self.n_users, self.n_items, self.k, self.d, feat.nnz)
        free = torch.cuda.mem_get_info(device)[0]
        if sparse + tables + ws > free:
            raise ValueError('%s: the two CSRs of the features need %d bytes (nnz = %d), the tables %d and the E-step %d; %d are free on %s'
                             % (who, sparse, feat.nnz, tables, ws, free, device))
        E = foldin._upload(np.ascontiguousarray(self.E, dtype=np.float32), device, np.float32)
        return types.SimpleNamespace(device=device, E=E, F=tkr_hip.csr_upload(feat, device), Ft=tkr_hip.csr_upload(canonical_csr(feat.T), device),
                                     ws=tkr_hip.workspace_room(None, ws, device))

    def _fe(self, run, check):
        return tkr_hip.csr_spmm(run.F, run.E, workspace=run.ws, check=check)

    def _prior(self, run):
        if self.estep == 'cg':
            Fe, run.fe_status = self._fe(run, False)
            return dict(prior=Fe, w_prior=self.lv)
        return dict(prior=(run.F @ run.E.double()).float(), w_prior=self.lv)

    def _after_steps(self, run):
        if self.estep == 'cg':                                     # warm-started: run.E is the E of the iteration before
            _, status = tkr_hip.estep_cg(run.F, run.Ft, run.V, run.E, lv=self.lv, le=self.le, steps=self.e_steps, heavy_from=ESTEP_HEAVY_FROM, workspace=run.ws,
                                         check=False)
            return 0.5 * self.le * run.E.double().square().sum(), [run.fe_status, status]
        run.E = torch.cholesky_solve(self.lv * (run.F.t() @ run.V.double()), run.FF).float()
        return 0.5 * self.le * run.E.double().square().sum(), []      # cer.py:63-65: the new E beside the Fe that entered the solve

    LOGS_CONVERGE = False

    def _check_iteration(self, who, it, loss, words):
        if self.estep == 'cg':
            tkr_hip.status_check('the prior F E of iteration %d' % it, tkr_hip._SPMM_REFUSED, tkr_hip.EstepRefused, int(words[0]))
            tkr_hip.status_check('the E-step of iteration %d' % it, tkr_hip._ESTEP_REFUSED, tkr_hip.EstepRefused, int(words[1]))

    def _cold_rows(self, run):                                     # cer.py:70-73: an item without a training like gets its content's row
        self.E = run.E.cpu().numpy()
        if self.estep == 'cg':
            return self._fe(run, True)
        return (run.F @ run.E.double()).float()

    def embed_items(self, feat, device=None):
        """fp32 [m, d] content features -> fp32 [m, k] = feat E, the fp64 product rounded once: the row of an item that was no line of
        vid, by the rule train() gives an item without a training like.  A scipy.sparse matrix stays sparse: feat E is one
        tkr_hip.csr_spmm on the GPU (`device`: None = the current one), a row the fp32 chain over its nonzeros in column order"""
        if self.E is None:
            raise ValueError('CER.embed_items: train() or import_embeddings() first')
        self._check_E('CER.embed_items')
        import scipy.sparse as ss
        if ss.issparse(feat):
            if feat.shape[1] != self.d:
                raise ValueError('CER.embed_items: feat has shape %s, the model needs (m, %d)' % (feat.shape, self.d))
            if feat.shape[0] == 0:
                return np.zeros((0, self.k), dtype=np.float32)
            device = foldin._device(device, 'CER.embed_items')
            E = foldin._upload(np.ascontiguousarray(self.E, dtype=np.float32), device, np.float32)
            return tkr_hip.csr_spmm(tkr_hip.csr_upload(canonical_csr(feat), device), E).cpu().numpy()
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


# ---- MLP and DPM (K22) ----------------------------------------------------------------------------------------------------------------------
MLP_MAX_HIDDEN = tkr_hip.MLP_MAX_LAYERS - 1
MLP_MAX_BATCH = tkr_hip.MLP_MAX_BATCH
_MLP_PARTS = ('W', 'bias', 'msW', 'msb')


def _check_batch(who, batch_size):
    if not isinstance(batch_size, (int, np.integer)) or not 1 <= batch_size <= MLP_MAX_BATCH:
        raise ValueError('%s: batch_size = %r, 1 <= batch_size <= %d is supported (TKR_MLP_MAX_BATCH)' % (who, batch_size, MLP_MAX_BATCH))


def _cuda(device, who):
    device = torch.device(foldin._device(device, who))
    return torch.device('cuda', torch.cuda.current_device()) if device.index is None else device


def epoch_order(seed, epoch, n):
    """the row order of MLP.fit's epoch `epoch` (counted from 0 over the life of the encoder, saved with it)"""
    return np.random.Generator(np.random.PCG64(np.random.SeedSequence([int(seed), int(epoch)]))).permutation(int(n)).astype(np.int32)


class MLP:
    """the content encoder of single/mlp.py:7-43 (d -> hidden layers with a sigmoid -> k, linear), trained by dense RMSProp in
    mini-batches; forward, gradients and the fused update are K22 (csrc/mlp.hip).  The reference's class cannot be instantiated
    (encoder.py:23 names the abstract method `pertrain`, mlp.py:42 defines `pretrain`: both names work here) and sizes the buffer of
    out() by the columns of X (mlp.py:26: by its rows here); `lbd` is accepted and unused, as there.

    The start is tf.layers.dense's: W Glorot-uniform, (2 r - 1) * fp32(sqrt(6 / (in + out))) in fp32 with r = Generator(PCG64(seed))
    .random(fp32) drawn layer by layer, biases 0; RMSProp slots 1.  fit() draws the order of epoch e as epoch_order(seed, e, n): a
    saved encoder resumes on the same stream.  Parameters and slots live on the device between calls."""

    def __init__(self, k: int, d: int, lr: float = 1e-4, lbd: float = 1e-4, hidden_layers=(2000, 1000), seed=None) -> None:
        hidden = list(hidden_layers)
        if not isinstance(k, (int, np.integer)) or not 1 <= k <= MAX_K:
            raise ValueError('MLP: k = %r, 1 <= k <= %d is supported (the ALS half-steps the encoder feeds)' % (k, MAX_K))
        if not isinstance(d, (int, np.integer)) or d < 1:
            raise ValueError('MLP: d = %r, the width of the content features, must be a positive integer' % (d,))
        if len(hidden) > MLP_MAX_HIDDEN:
            raise ValueError('MLP: %d hidden layers, at most %d are supported (TKR_MLP_MAX_LAYERS)' % (len(hidden), MLP_MAX_HIDDEN))
        if any(not isinstance(h, (int, np.integer)) or h < 1 for h in hidden):
            raise ValueError('MLP: hidden_layers = %r, every width must be a positive integer' % (hidden,))
        if not (np.isfinite(lr) and lr >= 0):
            raise ValueError('MLP: lr = %r must be finite and not negative' % (lr,))
        if seed is not None and not 0 <= int(seed) < 2 ** 63:
            raise ValueError('MLP: seed = %r, 0 <= seed < 2^63' % (seed,))
        self.k, self.d, self.lr, self.lbd = int(k), int(d), float(lr), float(lbd)
        self.hidden_layers = tuple(int(h) for h in hidden)
        self.seed = int(np.random.SeedSequence().generate_state(1, np.uint64)[0] >> 1) if seed is None else int(seed)
        self.epochs_done = 0
        rng = np.random.Generator(np.random.PCG64(self.seed))
        self._host, self._dev, self._net, self._ws = [], None, None, None
        for fan_in, fan_out in zip(self.widths, self.widths[1:]):
            limit = np.float32(np.sqrt(6.0 / (fan_in + fan_out)))
            W = (np.float32(2) * rng.random((fan_in, fan_out), dtype=np.float32) - np.float32(1)) * limit
            self._host.append(dict(W=W.astype(np.float32), bias=np.zeros(fan_out, np.float32), msW=np.ones((fan_in, fan_out), np.float32),
                                   msb=np.ones(fan_out, np.float32)))

    @property
    def widths(self):
        return (self.d,) + self.hidden_layers + (self.k,)

    # ------------------------------------------------------------------ state
    def _layers_host(self):
        if self._dev is None:
            return self._host
        return [{name: t.cpu().numpy() for name, t in layer.items()} for layer in self._dev]

    def state(self):
        """-> a dict of NumPy arrays: the parameters and slots (exact fp32), the widths, lr, seed and epochs_done"""
        out = dict(widths=np.asarray(self.widths, dtype=np.int64), lr=np.float64(self.lr), lbd=np.float64(self.lbd), seed=np.int64(self.seed),
                   epochs_done=np.int64(self.epochs_done))
        for l, layer in enumerate(self._layers_host()):
            for name in _MLP_PARTS:
                out['%s%d' % (name, l)] = np.array(layer[name], dtype=np.float32)
        return out

    def load_state(self, state):
        widths = [int(w) for w in np.asarray(state['widths']).reshape(-1)]
        if len(widths) < 2 or widths[0] != self.d or widths[-1] != self.k:
            raise ValueError('MLP.load_state: the state is a net of widths %s, this encoder maps d = %d to k = %d' % (widths, self.d, self.k))
        if len(widths) - 2 > MLP_MAX_HIDDEN or min(widths) < 1:
            raise ValueError('MLP.load_state: widths %s' % (widths,))
        host = []
        for l, (fan_in, fan_out) in enumerate(zip(widths, widths[1:])):
            layer = {}
            for name, shape in (('W', (fan_in, fan_out)), ('bias', (fan_out,)), ('msW', (fan_in, fan_out)), ('msb', (fan_out,))):
                a = np.asarray(state['%s%d' % (name, l)])
                if a.shape != shape or a.dtype != np.float32:
                    raise ValueError('MLP.load_state: %s%d is %s %s, the net needs float32 %s' % (name, l, a.dtype, a.shape, shape))
                layer[name] = np.array(a)
            host.append(layer)
        self.hidden_layers = tuple(widths[1:-1])
        self.lr, self.lbd = float(state['lr']), float(state['lbd'])
        self.seed, self.epochs_done = int(state['seed']), int(state['epochs_done'])
        self._host, self._dev, self._net, self._ws = host, None, None, None

    def _on(self, device):
        if self._dev is None or self._dev[0]['W'].device != device:
            host = self._layers_host()
            self._dev = [{name: foldin._upload(np.ascontiguousarray(layer[name], dtype=np.float32), device) for name in _MLP_PARTS} for layer in host]
            self._host, self._ws = None, None
            self._net = tkr_hip.mlp_net(self._dev)
        return self._net

    def _room(self, need, device):
        self._ws = tkr_hip.workspace_room(self._ws, need, device)
        return self._ws

    @staticmethod
    def _table(who, name, X, width):
        """a host array or a device tensor, checked -> a float32 [n, width] array, or the tensor made contiguous"""
        if isinstance(X, torch.Tensor):
            if X.dtype != torch.float32 or X.dim() != 2 or X.shape[1] != width or not X.is_cuda:
                raise ValueError('%s: %s is a %s tensor of shape %s on %s, the encoder needs float32 (n, %d) on the GPU'
                                 % (who, name, X.dtype, tuple(X.shape), X.device, width))
            return X.contiguous()
        X = np.ascontiguousarray(X, dtype=np.float32)
        if X.ndim != 2 or X.shape[1] != width:
            raise ValueError('%s: %s has shape %s, the encoder needs (n, %d)' % (who, name, X.shape, width))
        return X

    # ------------------------------------------------------------------ mlp.py:24-43
    def out(self, X, device=None):
        """fp32 [rows of X, k] = the network applied to every row of X (fp32 [n, d]): a NumPy array for a host array, a tensor on X's
        device for a device tensor"""
        X = self._table('MLP.out', 'X', X, self.d)
        from_host = not isinstance(X, torch.Tensor)
        if from_host:
            X = foldin._upload(X, _cuda(device, 'MLP.out'))
        if X.shape[0] == 0:
            F = torch.zeros((0, self.k), dtype=torch.float32, device=X.device)
        else:
            net = self._on(X.device)
            F = tkr_hip.mlp_forward(net, X, workspace=self._room(tkr_hip.mlp_workspace_bytes(net, int(X.shape[0])), X.device))
        return F.cpu().numpy() if from_host else F

    def _fit_device(self, X, Y, batch_size, order=None):
        """one epoch on device tensors -> (batch_loss float64 [batches], status int64 [1]) on the device; nothing is read back"""
        n = int(X.shape[0])
        if order is None:
            order = epoch_order(self.seed, self.epochs_done, n)
        if not isinstance(order, torch.Tensor):
            order = foldin._upload(np.ascontiguousarray(np.asarray(order).reshape(-1), dtype=np.int32), X.device)
        net = self._on(X.device)
        ws = self._room(tkr_hip.mlp_workspace_bytes(net, 0, int(batch_size)), X.device)
        self.epochs_done += 1
        return tkr_hip.mlp_fit(net, X, Y, order, int(batch_size), np.float32(self.lr), workspace=ws, check=False)

    def fit(self, X, Y, batch_size: int = 64, order=None, device=None) -> float:
        """one epoch of mlp.py:32-40 over the rows of X (fp32 [n, d]) and Y (fp32 [n, k]), host arrays or device tensors, in the order
        `order` (None: epoch_order(seed, epochs_done, n)) -> the sum of the batch objectives 1/2 sum (y - F)^2, each taken before its
        batch's step"""
        _check_batch('MLP.fit', batch_size)
        X, Y = self._table('MLP.fit', 'X', X, self.d), self._table('MLP.fit', 'Y', Y, self.k)
        if Y.shape[0] != X.shape[0] or X.shape[0] < 1:
            raise ValueError('MLP.fit: X has %d rows and Y %d; both need the same number, at least one' % (X.shape[0], Y.shape[0]))
        on = [t.device for t in (X, Y) if isinstance(t, torch.Tensor)]
        device = on[0] if on else _cuda(device, 'MLP.fit')
        X, Y = (t.to(device) if isinstance(t, torch.Tensor) else foldin._upload(t, device) for t in (X, Y))
        loss, status = self._fit_device(X, Y, batch_size, order)
        down = torch.cat([loss.sum().reshape(1), status.double()]).cpu().numpy()
        if int(down[1]) != -1:
            self.epochs_done -= 1                                  # (nothing was written: the epoch did not happen)
            tkr_hip.status_check('MLP.fit', tkr_hip._MLP_REFUSED, tkr_hip.MlpRefused, int(down[1]))
        if not np.isfinite(down[0]):
            raise FloatingPointError('MLP.fit: the objective of epoch %d is %r' % (self.epochs_done - 1, float(down[0])))
        return float(down[0])

    def pretrain(self, X=None, Y=None) -> None:
        tprint('MLP encoder does not implement pretrain method')

    pertrain = pretrain                                            # encoder.py:23 spells the abstract method this way


def dpm_train_bytes(n_users, n_items, k, d, widths, batch_size):
    """device bytes DPM.train allocates for a model of this shape -> (features, tables, encoder): features = 4 n_items d; tables =
    4 k (n_users + 2 n_items), U, V and Fe; encoder = 16 bytes per parameter (W, bias and their slots) and the workspace of K22"""
    net = tkr_hip.MlpNet()
    net.n_layers = len(widths) - 1
    for l, w in enumerate(widths):
        net.width[l] = int(w)
    params = sum(a * b + b for a, b in zip(widths, widths[1:]))
    return 4 * int(n_items) * int(d), 4 * int(k) * (int(n_users) + 2 * int(n_items)), 16 * params + tkr_hip.mlp_workspace_bytes(net, int(n_items), int(batch_size))


class DPM(WMF):
    """single/dpm.py:10-76: WMF whose item rows have the prior v_j ~ encoder(f_j), the encoder an MLP on the item's content features
    trained on the item table after every alternation.  `le` is accepted and unused, as in the reference."""

    def __init__(self, k: int, d: int, lu: float = 0.01, lv: float = 10, le: float = 10e3, a: float = 1, b: float = 0.01, *,
                 solver: str = 'cholesky', cg_steps: int = tkr_hip.ALS_CG_STEPS) -> None:
        if solver == 'cg' and isinstance(k, (int, np.integer)) and k > MAX_K:
            raise ValueError("DPM: k = %r, 1 <= k <= %d is supported under either solver: the encoder als.MLP is bounded there "
                             "(TKR_ALS_MAX_K), whatever solver='cg' allows WMF and CER" % (k, MAX_K))
        super().__init__(k, lu, lv, a, b, solver=solver, cg_steps=cg_steps)
        if not isinstance(d, (int, np.integer)) or d < 1:
            raise ValueError('DPM: d = %r, the width of the content features, must be a positive integer' % (d,))
        if not lv > 0:
            raise ValueError('DPM: lv = %r must be positive (the weight of the prior v ~ encoder(f))' % (lv,))
        self.__sn = 'dpm'
        self.d, self.le = int(d), float(le)
        self.encoder = None
        self.feat = None

    def _check_encoder(self, where):
        if not isinstance(self.encoder, MLP):
            raise ValueError('%s: the encoder is %r; als.MLP (the class, or an instance) is the one there is' % (where, self.encoder))
        if (self.encoder.d, self.encoder.k) != (self.d, self.k):
            raise ValueError('%s: the encoder maps d = %d to k = %d, the model needs (d, k) = (%d, %d)'
                             % (where, self.encoder.d, self.encoder.k, self.d, self.k))

    # ------------------------------------------------------------------ train (dpm.py:20-64)
    def train(self, encoder=MLP, max_iter: int = 200, model_path: str = None, verbose: bool = True, device=None, heavy_from=None,
              batch_size: int = 64) -> None:
        self._need_data('DPM.train')
        _need_content(self, 'DPM.train')
        _check_batch('DPM.train', batch_size)
        self.encoder = encoder(self.k, self.d) if isinstance(encoder, type) else encoder
        self._check_encoder('DPM.train')
        self._train('DPM.train', max_iter, None, model_path, verbose, device, heavy_from, batch_size=batch_size)

    STOPS_ON_TOL = LOGS_CONVERGE = False                           # no stopping test: dpm.py:31-60 runs every iteration

    def _prepare(self, who, device, batch_size):
        device = _cuda(device, who)
        features, tables, enc = dpm_train_bytes(self.n_users, self.n_items, self.k, self.d, self.encoder.widths, batch_size)
        free = torch.cuda.mem_get_info(device)[0]
        if features + tables + enc > free:
            raise ValueError('%s: the features need %d bytes (4 n_items d, d = %d, n_items = %d), the tables %d and the encoder with its '
                             'workspace %d; %d are free on %s' % (who, features, self.d, self.n_items, tables, enc, free, device))
        F = foldin._upload(np.ascontiguousarray(self.feat, dtype=np.float32), device, np.float32)
        return types.SimpleNamespace(device=device, F=F, batch_size=batch_size)

    def _prior(self, run):
        Fe = self.encoder.out(run.F)
        run.V.copy_(Fe)                                            # dpm.py:33: the item table IS the encoder's output when the users are solved
        return dict(prior=Fe, w_prior=self.lv)

    def _after_steps(self, run):
        fit, se = self.encoder._fit_device(run.F, run.V, run.batch_size)
        return fit.sum(), [se]

    def _check_iteration(self, who, it, loss, words):
        tkr_hip.status_check('the encoder step of iteration %d' % it, tkr_hip._MLP_REFUSED, tkr_hip.MlpRefused, int(words[0]))
        if not np.isfinite(loss):
            raise FloatingPointError('%s: the loss of iteration %d is %r' % (who, it, loss))

    def _cold_rows(self, run):                                     # dpm.py:61-64: an item without a training like gets its content's row
        return self.encoder.out(run.F)

    def embed_items(self, feat):
        """fp32 [m, d] content features -> fp32 [m, k] = encoder.out(feat): the row of an item that was no line of vid, by the rule
        train() gives an item without a training like"""
        if self.encoder is None:
            raise ValueError('DPM.embed_items: train() or import_embeddings() first')
        feat = np.asarray(feat, dtype=np.float32)
        if feat.ndim != 2 or feat.shape[1] != self.d:
            raise ValueError('DPM.embed_items: feat has shape %s, the model needs (m, %d)' % (feat.shape, self.d))
        return self.encoder.out(feat)

    def export_model(self, model_path: str) -> None:
        if os.path.isdir(model_path) and self.encoder is not None:
            target = os.path.join(model_path, 'mlp.npz')
            tprint('Saving the encoder to %s' % target)
            np.savez(target, **self.encoder.state())

    def import_model(self, model_path: str) -> None:
        source = os.path.join(model_path, 'mlp.npz')
        if os.path.exists(source):
            tprint('Loading the encoder from %s' % source)
            with np.load(source) as fh:
                state = {name: fh[name] for name in fh.files}
            if self.encoder is None:
                self.encoder = MLP(self.k, self.d, hidden_layers=())
            self._check_encoder('DPM.import_model')
            self.encoder.load_state(state)
