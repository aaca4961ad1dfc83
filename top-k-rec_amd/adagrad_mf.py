"""What LMF (lmf.py, K25) and SMF (smf.py, K27) share, written once: two tables augmented by a few columns and moved by alternating
half-steps of full-gradient AdaGrad over every (user, item) pair.  AdagradMF holds the hyper-parameters both have, the data, the
training loop, the fold-in loop and <name>.npz; a model adds the layout of its augmented tables (_tables, _take), what one iteration
launches and how its loss is put together (_prepare, _iteration), and the start row, the step and the return value of its fold-in.
The class name is the model's name in messages, its lower case the name of the .npz.  Tables, slots and both like CSRs stay on the
device for the loop; one download per iteration carries the loss and the status words.
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
from utils import get_id_dict_from_file, tprint


def dense_room(work, X, Y, k, sizer):
    """-> the workspace (room for sizer(n_x, k, n_y) bytes) and the D of X's shape, kept in the dict `work` between calls"""
    ws = work['ws'] = tkr_hip.workspace_room(work.get('ws'), sizer(int(X.shape[0]), k, int(Y.shape[0])), X.device)
    D = work.get(('D', X.shape))
    if D is None or D.device != X.device:
        D = work[('D', X.shape)] = torch.empty_like(X)
    return ws, D


def _listed(names):
    return ' and '.join([', '.join(names[:-1]), names[-1]] if len(names) > 1 else names)


class AdagradMF(REC):
    EXTRA = None                 # the columns a table holds beside its k factors
    MAX_K = None                 # ... and the widest k, TKR_<NAME>_MAX_K
    REFUSED = RAISES = None      # the messages of the step's status word (tkr_hip._*_REFUSED) and the class they raise
    ARRAYS = ('hu', 'hi')        # the arrays <name>.npz keeps beside the text matrices, in its order, and what its log lines call them
    ARRAYS_TEXT = ('AdaGrad slots',)
    SCALARS = ('lam', 'lr')      # ... and the hyper-parameters: (key, attribute) where the two differ

    def __init__(self, k, lam, lr) -> None:
        name = type(self).__name__
        if not isinstance(k, (int, np.integer)) or isinstance(k, bool) or not 1 <= k <= self.MAX_K:
            raise ValueError('%s: k = %r, 1 <= k <= %d is supported (TKR_%s_MAX_K: a row block of the gradient lives in the registers of '
                             'one workgroup)' % (name, k, self.MAX_K, name))
        if not (np.isfinite(lam) and lam >= 0):
            raise ValueError('%s: lam = %r must be finite and not negative' % (name, lam))
        if not (np.isfinite(lr) and lr > 0):
            raise ValueError('%s: lr = %r must be positive and finite' % (name, lr))
        self.__sn = name.lower()
        self.k = int(k)
        self.lam, self.lr = float(lam), float(lr)
        self.uids = self.iids = None
        self.n_users = self.n_items = self.n_likes = None
        self.fue = self.fie = self.fib = None                         # factors [n, k], item biases [n_items, 1]
        self.hu = self.hi = None                                      # the AdaGrad slots, [n_users, k + EXTRA] and [n_items, k + EXTRA]
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
            raise ValueError('%s: %s / %s list no users or no items' % (type(self).__name__, uid_file, iid_file))
        R = textio.parse_ratings(tr_file, self.uids, self.iids)
        up, uc = foldin.liked_csr(R, self.n_users, self.n_items, by='user')
        ip, ic = foldin.liked_csr(R, self.n_items, self.n_users, by='item')
        self._csr = (up, uc, ip, ic)
        self.n_likes = int(len(uc))
        self._on_data()
        rng = np.random.Generator(np.random.PCG64(seed))
        self.seed = seed
        self.fue = rng.standard_normal((self.n_users, self.k), dtype=np.float32) * np.float32(0.01)
        self.fie = rng.standard_normal((self.n_items, self.k), dtype=np.float32) * np.float32(0.01)
        self.fib = np.zeros((self.n_items, 1), dtype=np.float32)
        self.hu = np.ones((self.n_users, self.k + self.EXTRA), dtype=np.float32)
        self.hi = np.ones((self.n_items, self.k + self.EXTRA), dtype=np.float32)
        self.iters_done = 0
        tprint('Loading finished!')

    def _on_data(self):
        """behind the like CSRs of load_training_data: what else the model derives from the data or starts at"""

    def build_graph(self) -> None:
        tprint('%s does not require build_graph method!' % self.__sn)

    def _shapes(self):
        k, K = self.k, self.k + self.EXTRA
        return dict(fue=(self.n_users, k), fie=(self.n_items, k), fib=(self.n_items, 1), fub=(self.n_users,), hu=(self.n_users, K), hi=(self.n_items, K))

    def _check_shapes(self):
        """the head of _tables: fib as a column, and every host array of the model in the shape the model needs"""
        if self.fib is not None and np.size(self.fib) == self.n_items:
            self.fib = np.asarray(self.fib, dtype=np.float32).reshape(-1, 1)
        shapes = self._shapes()
        for name in ('fue', 'fie', 'fib') + self.ARRAYS:
            if np.shape(getattr(self, name)) != shapes[name]:
                raise ValueError('%s: %s has shape %s, the model needs %s' % (type(self).__name__, name, np.shape(getattr(self, name)), shapes[name]))

    # ------------------------------------------------------------------ train
    # The one training loop of LMF and SMF.  `run` is the device state of one call: the tables Xa and Ya, their slots Hx and Hy, the
    # like CSRs (up, uc) and (ip, ic), and what _prepare puts beside them.
    def train(self, max_iter: int = 30, tol: float = None, model_path: str = None, verbose: bool = True, device=None, heavy_from=None) -> None:
        who = '%s.train' % type(self).__name__
        if self._csr is None:
            raise ValueError('%s: load_training_data() first' % who)
        if model_path is not None and os.path.isdir(model_path):
            self.import_embeddings(model_path)
        device = foldin._device(device, who)
        run = types.SimpleNamespace()
        run.Xa, run.Ya = (foldin._upload(t, device, np.float32) for t in self._tables())
        run.Hx, run.Hy = foldin._upload(self.hu, device, np.float32), foldin._upload(self.hi, device, np.float32)
        run.up, run.uc, run.ip, run.ic = (foldin._upload(x, device) for x in self._csr)
        self._prepare(run, heavy_from)
        loss, self.losses = np.exp(50), []
        for it in range(max_iter):
            t1 = time.time()
            loss_old = loss
            total, su, sv = self._iteration(run)
            down = torch.cat([total.reshape(1), su.double(), sv.double()]).cpu().numpy()      # one copy: the loss, the status words behind it
            for word, what in zip(down[1:], ('the user step of iteration %d', 'the item step of iteration %d')):
                tkr_hip.status_check('%s, %s' % (who, what % it), self.REFUSED, self.RAISES, int(word))
            loss = float(down[0])
            if not np.isfinite(loss):
                raise tkr_hip.TkrError('%s: the loss of iteration %d is %r; lower lr (%g)' % (who, it, loss, self.lr))
            self.losses.append(loss)
            self.iters_done += 1
            cond = abs(loss_old - loss) / loss_old
            if verbose:
                tprint('Iter %3d, loss %.6f, converge %.6f, time %.2fs' % (it, loss, cond, time.time() - t1))
            if tol is not None and cond < tol:
                break
        self._take(run.Xa, run.Ya, run.Hx, run.Hy)

    def _prepare(self, run, heavy_from):
        """behind the uploads: run.hyper, the keywords of every step of the loop, and whatever else the model keeps on the device"""
        raise NotImplementedError

    def _iteration(self, run):
        """the launches of one iteration -> (its loss, a device scalar; the status tensor of the user step; of the item step)"""
        raise NotImplementedError

    # ------------------------------------------------------------------ fold-in
    def _fold_in(self, histories, steps, device, heavy_from):
        """`steps` user half-steps (_fold_step) from zero rows with _fold_start's columns set (slots 1.0) against the frozen item table
        -> the rows [n_new, k + EXTRA] on the host"""
        who = '%s.fold_in' % type(self).__name__
        if self.fie is None:
            raise ValueError('%s: load_training_data() and train() first' % who)
        if not isinstance(steps, (int, np.integer)) or isinstance(steps, bool) or steps < 0:
            raise ValueError('%s: steps = %r must be an integer, at least 0' % (who, steps))
        device = foldin._device(device, who)
        ptr, cols = histories if isinstance(histories, tuple) else foldin.history_csr(histories, self.n_items)
        X = torch.zeros((len(ptr) - 1, self.k + self.EXTRA), dtype=torch.float32, device=device)
        if len(ptr) == 1:
            return X.cpu().numpy()
        self._fold_start(X)
        H = torch.ones_like(X)
        Ya = foldin._upload(self._tables()[1], device, np.float32)
        ptr, cols = foldin._upload(ptr, device), foldin._upload(cols, device)
        work, words = {}, []
        for _ in range(int(steps)):
            words.append(self._fold_step(X, H, Ya, ptr, cols, heavy_from, work))
        X = X.cpu().numpy()
        for word in (torch.cat(words).cpu().numpy() if words else ()):
            tkr_hip.status_check(who, self.REFUSED, self.RAISES, int(word))
        return X

    # ------------------------------------------------------------------ <name>.npz
    def export_model(self, model_path: str) -> None:
        target = os.path.join(model_path, '%s.npz' % self.__sn)
        tprint('Saving %s to %s' % (_listed(self.ARRAYS_TEXT + ('hyper-parameters',)), target))
        stored = {name: np.asarray(getattr(self, name), dtype=np.float32) for name in self.ARRAYS}
        stored.update((key, np.float64(getattr(self, attr))) for key, attr in (x if isinstance(x, tuple) else (x, x) for x in self.SCALARS))
        np.savez(target, **stored, seed=np.int64(-1 if self.seed is None else self.seed), iters=np.int64(self.iters_done))

    def import_model(self, model_path: str) -> None:
        source = os.path.join(model_path, '%s.npz' % self.__sn)
        if not os.path.exists(source):
            return
        tprint('Loading %s from %s' % (_listed(self.ARRAYS_TEXT), source))
        with np.load(source) as z:
            arrays = tuple(z[name].astype(np.float32) for name in self.ARRAYS)
            have, want = tuple(x.shape for x in arrays), tuple(self._shapes()[name] for name in self.ARRAYS)
            if self.n_users is not None and have != want:
                raise ValueError('%s: %s holds arrays of shapes %s, the model needs %s' % (type(self).__name__, source, have, want))
            for name, x in zip(self.ARRAYS, arrays):
                setattr(self, name, x)
            self.iters_done = int(z['iters'])
