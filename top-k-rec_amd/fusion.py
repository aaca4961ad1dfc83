"""Fusion of several trained models (K16): the second half of the paper the reference implements ("Exploiting Rich Contents for
Personalized Video Recommendation": one model per content feature, their scores fused), old/methods/{a,p,b,e}fusion.py there.

    models = load_models('data', ['embed/bpr', 'embed/vbpr_cnn', 'embed/vbpr_mfcc'])
    w = learn_pairwise(models, csr, n_items)                       # bfusion: one weight per model, learned by BPR on the scores
    U, V = fuse(models, w)
    write_fused('embed/fused', U, V, dict(method='b', ...))        # an ordinary model directory: evaluate.py / recommend.py run on it

Every fusion here is linear in the per-model scores, sum_m w_m (<U_m[u], V_m[i]> + b_m[i]), which is the inner product of two
concatenated tables: ``fuse`` builds them with torch elementwise ops and the fused model is served by K4 / K5 / K8 / K12 unchanged.
Learning the weights is the part with a hot path (csrc/fusion.hip; include/tkr.h K16).

What differs from the reference, on purpose:
  * ``learn_pairwise`` mirrors the loop of ranking_fusion.py:48-54, which stops while ``(z + 1) * batch < n_samples``: the LAST batch
    is dropped (999 batches for the defaults 10,000,000 / 10,000, not 1,000).  ``epochs`` is unused there and absent here.  The
    triplets are K1's stream (the draw of BPR.train), negatives over the whole ``vid`` (the reference draws over f?tr.idl).
  * ``learn_per_user`` takes the users' likes as SETS (foldin.liked_csr); the reference's csc_matrix adds a like listed twice up to
    2.0 (efusion.py:72).
  * a user whose mean RMSE is exactly 0 (no training likes) gets the weights 1.0, the continuous value of exp(-(r - mean)); the
    reference leaves them 0 (efusion.py:79), which erases that user's ranking.
  * sfusion.py (an SVM from scikit-learn on the score differences of sampled triplets) lives in svmfusion.py (K23): the same
    objective minimised by Newton's method on sums formed on the GPU, no library; ``fuse.py --method s``.
"""
from __future__ import annotations

import json
import os

import numpy as np
import torch

import textio
import tkr_hip

CHUNK_BYTES = 256 << 20       # the features of one chunk of learn_pairwise: D fp32 [rows, M] stays below this
METHODS = ('a', 'p', 'b', 'e', 'w')


def load_models(data_dir, model_dirs):
    """-> [(U fp32 [n_users, k_m], V fp32 [n_items, k_m], b fp32 [n_items] | None)] from every directory's final-U.dat, final-V.dat and
    optional final-B.dat, rows addressed through DATA/uid and DATA/vid as evaluate.py addresses them (textio.read_matrix)."""
    from evaluate import read_ids, read_model
    uids, vids = read_ids(os.path.join(data_dir, 'uid')), read_ids(os.path.join(data_dir, 'vid'))
    models = []
    for d in model_dirs:
        U, V, b = read_model(d, uids, vids)
        if U.shape[1] != V.shape[1]:
            raise ValueError('%s: final-U.dat has %d columns, final-V.dat %d' % (d, U.shape[1], V.shape[1]))
        models.append((U, V, None if b is None else b.reshape(-1)))
    return models


def fixed_weights(M, method, p=None, weights=None):
    """the weights that need no training -> float32 [M]: 'a' the average 1 / M (afusion.py:27), 'p' the geometric (1 - p)^m * p in
    the order the models are given (pfusion.py:62-69), 'w' the weights passed in"""
    if M < 1:
        raise ValueError('at least one model required')
    if method == 'a':
        return np.full(M, 1.0 / M, dtype=np.float32)
    if method == 'p':
        if p is None:
            raise ValueError("method 'p' needs p")
        out = np.zeros(M, dtype=np.float32)
        for m in range(M):
            out[m] = np.power(1 - p, m) * p
        return out
    if method == 'w':
        w = np.asarray([] if weights is None else weights, dtype=np.float32).reshape(-1)
        if len(w) != M:
            raise ValueError("method 'w' needs one weight per model (%d given, %d models)" % (len(w), M))
        return w
    raise ValueError("fixed_weights: method must be 'a', 'p' or 'w', not %r" % (method,))


def n_batches_of(n_samples, batch_size):
    """the number of z >= 0 with (z + 1) * batch_size < n_samples (ranking_fusion.py:48): the last batch is dropped"""
    return max((int(n_samples) - 1) // int(batch_size), 0)


def _device(device, who):
    if device is None and not torch.cuda.is_available():
        raise tkr_hip.TkrError('%s runs on the GPU through libtkr_hip.so; no MI355X is visible' % who)
    return torch.device('cuda', torch.cuda.current_device()) if device is None else device


def _on_device(models, device):
    def up(a, flat=False):
        if a is None:
            return None
        t = torch.as_tensor(a)
        t = t.reshape(-1) if flat else t
        return t.to(device=device, dtype=torch.float32).contiguous()
    return [(up(U), up(V), up(b, flat=True)) for U, V, b in models]


def learn_pairwise(models, csr, n_items, *, n_samples=10_000_000, batch_size=10_000, lr=1e-4, lambda_w=0.0025, seed=0, want_loss=False,
                   chunk_bytes=None):
    """bfusion.py + ranking_fusion.py -> W float32 [M] (with want_loss: (W, the loss of every batch)).  ``csr`` is the TrainingCSR of
    the training likes (BPR.load_training_data + BPR._make_csr).  W starts at zeros; triplet t of the run is triplet t of K1's stream
    under ``seed``; batch z is the triplets [z B, (z + 1) B) with B = min(batch_size, number of training pairs)
    (ranking_fusion.py:40-42); n_batches_of(n_samples, B) batches run -- the reference drops the last one.
    Features (tkr_hip.fusion_features) and steps (tkr_hip.fusion_sgd) alternate chunk by chunk on one stream; a chunk is a whole
    number of batches whose features stay below ``chunk_bytes`` (default CHUNK_BYTES).  The result does not depend on the chunking."""
    device = csr.tr_users.device
    models = _on_device(models, device)
    M = len(models)
    B = int(batch_size)
    if B < 1:
        raise tkr_hip.TkrError('learn_pairwise: batch_size >= 1 required, got %d' % B)
    B = min(B, int(csr.nnz)) if csr.nnz > 0 else B
    nb = n_batches_of(n_samples, B)
    W = torch.zeros(M, dtype=torch.float32, device=device)
    losses = []
    limit = CHUNK_BYTES if chunk_bytes is None else int(chunk_bytes)
    per_chunk = max(1, limit // (4 * M * B))
    for z0 in range(0, nb, per_chunk):
        n = min(per_chunk, nb - z0)
        D = tkr_hip.fusion_features(models, csr, n_items, seed, z0 * B, n * B)
        out = tkr_hip.fusion_sgd(D, B, n, lr, lambda_w, W, want_loss=want_loss)
        if want_loss:
            losses.append(out[1])
        del D
    W = W.cpu().numpy()
    if want_loss:
        return W, (torch.cat(losses).cpu().numpy() if losses else np.zeros(0, np.float32))
    return W


def learn_per_user(models, like_ptr, like_cols, device=None):
    """efusion.py:57-82 -> (w float32 [n_users, M], rmse float32 [n_users, M]): per user the root mean squared error of every model's
    scores against 1 on the user's training likes, and the weights exp(-(rmse - its mean over the models)).  The like CSR comes from
    foldin.liked_csr(textio.parse_ratings(...), n_users, n_items)."""
    device = _device(device, 'learn_per_user')
    ptr = torch.as_tensor(np.ascontiguousarray(like_ptr, dtype=np.int64)).to(device)
    cols = torch.as_tensor(np.ascontiguousarray(like_cols, dtype=np.int32)).to(device)
    rmse, w = tkr_hip.fusion_user_weights(_on_device(models, device), ptr, cols)
    return w.cpu().numpy(), rmse.cpu().numpy()


def fuse(models, weights, dtype=torch.float32):
    """-> (U~ [n_users, K], V~ [n_items, K]) with <U~[u], V~[i]> = sum_m w_m (<U_m[u], V_m[i]> + b_m[i]): U~ is the concatenation of
    w_m * U_m, V~ that of V_m, and every model with a bias adds one column, w_m in U~ and b_m in V~ (so a fused model has no
    final-B.dat, and per-user weights work too).  ``weights`` is [M] or [n_users, M].  numpy in, numpy out; tensors stay tensors."""
    as_numpy = not isinstance(models[0][0], torch.Tensor)
    M = len(models)
    n_users = int(models[0][0].shape[0])
    dev = models[0][0].device if not as_numpy else None
    w = torch.as_tensor(np.asarray(weights) if not isinstance(weights, torch.Tensor) else weights).to(device=dev, dtype=dtype)
    if w.dim() == 1:
        w = w.reshape(1, -1).expand(n_users, -1)
    if tuple(w.shape) != (n_users, M):
        raise ValueError('fuse: weights must be [M] or [n_users, M] for %d users and %d models, not %s' % (n_users, M, tuple(w.shape)))
    left, right = [], []
    for m, (U, V, b) in enumerate(models):
        left.append(torch.as_tensor(U).to(dtype) * w[:, m:m + 1])
        right.append(torch.as_tensor(V).to(dtype))
    for m, (U, V, b) in enumerate(models):
        if b is not None:
            left.append(w[:, m:m + 1])
            right.append(torch.as_tensor(b).to(dtype).reshape(-1, 1))
    Uf, Vf = torch.cat(left, dim=1).contiguous(), torch.cat(right, dim=1).contiguous()
    return (Uf.numpy(), Vf.numpy()) if as_numpy else (Uf, Vf)


def write_fused(out_dir, U, V, meta, user_weights=None):
    """an ordinary model directory: final-U.dat and final-V.dat ('%f ' text, textio.write_matrix), fusion.json (``meta``: method,
    model directories, global weights, hyper-parameters, seed, number of batches) and, for per-user weights, final-W.dat.  The
    directory is created like REC.export_embeddings creates it (os.mkdir: the parent must exist)."""
    if not os.path.exists(out_dir):
        os.mkdir(out_dir)
    textio.write_matrix(os.path.join(out_dir, 'final-U.dat'), U)
    textio.write_matrix(os.path.join(out_dir, 'final-V.dat'), V)
    if user_weights is not None:
        textio.write_matrix(os.path.join(out_dir, 'final-W.dat'), np.asarray(user_weights, dtype=np.float32))
    with open(os.path.join(out_dir, 'fusion.json'), 'w') as fh:
        json.dump(meta, fh, indent=1, sort_keys=True)
        fh.write('\n')
