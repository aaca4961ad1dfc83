"""ItemKNN -- the item-neighbourhood model (item-to-item collaborative filtering), built and served on MI355X (K28 / K29, csrc/knn.hip):
the yardstick of the recommender literature beside the latent-factor models of this package.

    from knn import ItemKNN
    model = ItemKNN(n_neighbors=100, shrink=0.0, similarity='cosine')
    model.load_training_data('data/uid', 'data/vid', 'data/f0tr.txt')
    model.train()
    model.export_model('embed/knn')                            # knn.npz

For every item the N most similar items are kept,

    sim(i, j) = c_ij / (norm_i norm_j + shrink),        c_ij = the number of users who like both,

with norm_i = sqrt(n_i) ('cosine'; n_i the likers of i) or 1 and shrink = 0 ('cooc': the raw count).  A user's score of item j is the
sum of sim(i, j) over the items i of the history that have j among their N nearest.  There is no iteration, no learning rate and no
seed: training is one pass over the likes (tkr_hip.knn_build), deterministic by construction, and a user who arrives after training is
served from the history alone (tkr_hip.knn_score) -- no fold-in step.  The co-occurrence matrix is never in memory (DESIGN.md section 4
K28/K29).

There is no final-*.dat: a directory that holds knn.npz IS a neighbourhood model, for evaluate.py and recommend.py.  The file holds the
table (nbr_ids int32 [n_items, N], -1 padded; nbr_w fp32), n_likers int64 [n_items] and the three hyper-parameters.
"""
from __future__ import annotations

import os

import numpy as np
import torch

import foldin
import textio
import tkr_hip
from utils import get_id_dict_from_file, tprint

FILE = 'knn.npz'
SIMILARITIES = ('cosine', 'cooc')
MAX_N = tkr_hip.KNN_MAX_N


def is_model_dir(path):
    """a directory with knn.npz is a neighbourhood model"""
    return path is not None and os.path.exists(os.path.join(path, FILE))


def _check_hyper(n_neighbors, shrink, similarity):
    if not isinstance(n_neighbors, (int, np.integer)) or isinstance(n_neighbors, bool) or not 1 <= n_neighbors <= MAX_N:
        raise ValueError('ItemKNN: n_neighbors = %r, 1 <= n_neighbors <= %d is supported (TKR_KNN_MAX_N)' % (n_neighbors, MAX_N))
    if not (np.isfinite(shrink) and shrink >= 0):
        raise ValueError('ItemKNN: shrink = %r must be finite and not negative' % (shrink,))
    if similarity not in SIMILARITIES:
        raise ValueError('ItemKNN: similarity = %r, one of %s is supported' % (similarity, ', '.join(SIMILARITIES)))


def norms(n_likers, similarity):
    """what K28 is given for `norm` and `shrink`'s companion: sqrt(n_i) in float64 by NumPy ('cosine'; an item nobody likes has no
    candidates, its norm is 1), or 1 ('cooc')"""
    n = np.asarray(n_likers, dtype=np.float64)
    return np.sqrt(np.maximum(n, 1.0)) if similarity == 'cosine' else np.ones_like(n)


def check_table(nbr_ids, nbr_w, n_likers, where='ItemKNN'):
    """refuse a table whose shapes, dtypes, id range or finiteness are wrong -> (n_items, N)"""
    if nbr_ids.dtype != np.int32 or nbr_w.dtype != np.float32 or n_likers.dtype != np.int64:
        raise ValueError('%s: nbr_ids, nbr_w and n_likers must be int32, float32 and int64, not %s, %s and %s'
                         % (where, nbr_ids.dtype, nbr_w.dtype, n_likers.dtype))
    if nbr_ids.ndim != 2 or nbr_ids.shape != nbr_w.shape or n_likers.shape != nbr_ids.shape[:1]:
        raise ValueError('%s: nbr_ids, nbr_w and n_likers have shapes %s, %s and %s; the model needs (n_items, N) twice and (n_items,)'
                         % (where, nbr_ids.shape, nbr_w.shape, n_likers.shape))
    n_items, N = nbr_ids.shape
    if n_items < 1 or not 1 <= N <= MAX_N:
        raise ValueError('%s: a table of %d items and %d neighbours; at least one item and 1 <= N <= %d' % (where, n_items, N, MAX_N))
    if nbr_ids.min() < -1 or nbr_ids.max() >= n_items:
        raise ValueError('%s: nbr_ids holds an id outside [-1, %d)' % (where, n_items))
    if not np.isfinite(nbr_w).all():
        raise ValueError('%s: nbr_w holds a weight that is not finite' % where)
    if n_likers.min() < 0:
        raise ValueError('%s: n_likers holds a negative count' % where)
    return n_items, N


class ItemKNN:
    def __init__(self, n_neighbors: int = 100, shrink: float = 0.0, similarity: str = 'cosine') -> None:
        _check_hyper(n_neighbors, shrink, similarity)
        self.n_neighbors, self.shrink, self.similarity = int(n_neighbors), float(shrink), similarity
        self.uids = self.iids = None
        self.n_users = self.n_items = self.n_likes = None
        self.nbr_ids = self.nbr_w = self.n_likers = None              # the table: int32 / fp32 [n_items, N], int64 [n_items]
        self._csr = None                                              # host CSRs: (user ptr, user cols, item ptr, item rows)
        self._dev = None                                              # the table on a device, for recommend()

    # ------------------------------------------------------------------ data
    def load_training_data(self, uid_file: str, iid_file: str, tr_file: str) -> None:
        """the like == 1 entries of known users and items, as sets"""
        tprint('Load training data from %s' % (tr_file))
        self.uids = get_id_dict_from_file(uid_file)
        self.iids = get_id_dict_from_file(iid_file)
        self.n_users, self.n_items = len(self.uids), len(self.iids)
        if self.n_users < 1 or self.n_items < 1:
            raise ValueError('ItemKNN: %s / %s list no users or no items' % (uid_file, iid_file))
        R = textio.parse_ratings(tr_file, self.uids, self.iids)
        self.set_likes(*foldin.liked_csr(R, self.n_users, self.n_items, by='user'), *foldin.liked_csr(R, self.n_items, self.n_users, by='item'))
        tprint('Loading finished!')

    def set_likes(self, u_ptr, u_cols, i_ptr, i_rows) -> None:
        """the likes as the CSR over users and its transpose over items (foldin.group_history's arrays), for callers without files"""
        self.n_users, self.n_items = len(u_ptr) - 1, len(i_ptr) - 1
        self._csr = (np.asarray(u_ptr, np.int64), np.asarray(u_cols, np.int32), np.asarray(i_ptr, np.int64), np.asarray(i_rows, np.int32))
        self.n_likes = int(len(self._csr[1]))

    # ------------------------------------------------------------------ train
    def train(self, model_path: str = None, device=None, heavy_from=None, slab_cols=None) -> None:
        """one call of K28.  model_path: a directory the model is written to afterwards (export_model)"""
        if self._csr is None:
            raise ValueError('ItemKNN.train: load_training_data() first')
        device = foldin._device(device, 'ItemKNN.train')
        up, uc, ip, ir = (foldin._upload(x, device) for x in self._csr)
        self.n_likers = np.diff(self._csr[2]).astype(np.int64)
        norm = foldin._upload(norms(self.n_likers, self.similarity), device, np.float64)
        shrink = self.shrink if self.similarity == 'cosine' else 0.0
        ids, w = tkr_hip.knn_build(up, uc, ip, ir, norm, self.n_neighbors, shrink=shrink, heavy_from=heavy_from, slab_cols=slab_cols)
        self.nbr_ids, self.nbr_w = ids.cpu().numpy(), w.cpu().numpy()
        self._dev = (ids, w)
        if model_path is not None:
            self.export_model(model_path)

    # ------------------------------------------------------------------ knn.npz
    def export_model(self, model_path: str) -> None:
        if self.nbr_ids is None:
            raise ValueError('ItemKNN.export_model: train() or import_model() first')
        if not os.path.isdir(model_path):
            os.makedirs(model_path)
        target = os.path.join(model_path, FILE)
        tprint('Saving the neighbour table and the hyper-parameters to %s' % target)
        np.savez(target, nbr_ids=self.nbr_ids, nbr_w=self.nbr_w, n_likers=self.n_likers, n_neighbors=np.int64(self.n_neighbors),
                 shrink=np.float64(self.shrink), similarity=np.str_(self.similarity))

    def import_model(self, model_path: str) -> None:
        source = os.path.join(model_path, FILE)
        with np.load(source) as z:
            missing = [name for name in ('nbr_ids', 'nbr_w', 'n_likers', 'n_neighbors', 'shrink', 'similarity') if name not in z.files]
            if missing:
                raise ValueError('ItemKNN: %s lacks %s' % (source, ', '.join(missing)))
            nbr_ids, nbr_w, n_likers = z['nbr_ids'], z['nbr_w'], z['n_likers']
            n_neighbors, shrink, similarity = int(z['n_neighbors']), float(z['shrink']), str(z['similarity'])
        _check_hyper(n_neighbors, shrink, similarity)
        n_items, N = check_table(nbr_ids, nbr_w, n_likers, 'ItemKNN: %s' % source)
        if N != n_neighbors:
            raise ValueError('ItemKNN: %s keeps %d neighbours per item and says n_neighbors = %d' % (source, N, n_neighbors))
        if self.n_items is not None and n_items != self.n_items:
            raise ValueError('ItemKNN: %s is a table of %d items, the id list holds %d' % (source, n_items, self.n_items))
        self.nbr_ids, self.nbr_w, self.n_likers = np.ascontiguousarray(nbr_ids), np.ascontiguousarray(nbr_w), np.ascontiguousarray(n_likers)
        self.n_neighbors, self.shrink, self.similarity, self.n_items = n_neighbors, shrink, similarity, n_items
        self._dev = None

    # ------------------------------------------------------------------ serve
    def table(self, device):
        """(nbr_ids, nbr_w) on `device`, uploaded once"""
        if self.nbr_ids is None:
            raise ValueError('ItemKNN: train() or import_model() first')
        if self._dev is None or self._dev[0].device != torch.device(device):
            self._dev = (foldin._upload(self.nbr_ids, device, np.int32), foldin._upload(self.nbr_w, device, np.float32))
        return self._dev

    def recommend(self, histories, total: int, exclude=None, device=None):
        """the `total` best catalogue items of every history, best first -> (ids int32 [n, total], scores fp32 [n, total]) as numpy,
        padded -1 / -inf.  histories: a list of item-index sequences, one per user, or the (ptr, cols) pair of foldin.group_history;
        exclude: the same, the items a line must not list (default: the history itself; a list of empty sequences excludes nothing)"""
        device = foldin._device(device, 'ItemKNN.recommend')
        ids_dev, w_dev = self.table(device)
        hist = histories if isinstance(histories, tuple) else foldin.history_csr(histories, self.n_items)
        n = len(hist[0]) - 1
        if n == 0:
            return np.zeros((0, total), np.int32), np.zeros((0, total), np.float32)
        excl = hist if exclude is None else (exclude if isinstance(exclude, tuple) else foldin.history_csr(exclude, self.n_items))
        if len(excl[0]) - 1 != n:
            raise ValueError('ItemKNN.recommend: %d histories and %d lists of excluded items' % (n, len(excl[0]) - 1))
        mask, pitch = tkr_hip.build_rated_mask(foldin._upload(excl[0], device, np.int64), foldin._upload(excl[1], device, np.int32), n, self.n_items)
        ids, scores = tkr_hip.knn_score(foldin._upload(hist[0], device, np.int64), foldin._upload(hist[1], device, np.int32), ids_dev, w_dev,
                                        int(total), mask=mask, mask_pitch=pitch, want_scores=True)
        return ids.cpu().numpy(), scores.cpu().numpy()


def load(model_dir):
    """the ItemKNN of a model directory (knn.npz)"""
    model = ItemKNN()
    model.import_model(model_dir)
    return model
