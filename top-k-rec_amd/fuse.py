"""fuse.py -- fuse several trained models into one model directory; the learned weights are learned on MI355X (K16, fusion.py; K23,
svmfusion.py).

    python fuse.py -d DATA -m MODEL [MODEL ...] -o OUT [-f FOLD] --method a|p|b|e|w|s
                   [--p 0.5] [--weights w1 w2 ...] [--samples N] [--batch B] [--lr LR] [--lambda-w L] [--svm-c C] [--seed S]

Inputs: ``DATA/uid``, ``DATA/vid``, every ``MODEL/final-U.dat``, ``final-V.dat``, optional ``final-B.dat`` and, for the methods b, e
and s only, ``DATA/f{FOLD}tr.txt``.  Methods (the reference's old/methods/):

    a   the average, 1 / M                                                 (afusion.py)
    p   (1 - p)^m * p in the order of -m                                   (pfusion.py, --p)
    w   the weights of --weights
    b   one weight per model learned by BPR on the models' scores          (bfusion.py + ranking_fusion.py; --samples --batch --lr
                                                                            --lambda-w --seed)
    e   a weight per user and model from the model's RMSE on the user's training likes   (efusion.py)
    s   one weight per model from a linear SVM on the score differences of sampled triplets   (sfusion.py; --samples --svm-c --seed)

OUT becomes an ordinary model directory (final-U.dat, final-V.dat; fusion.json; final-W.dat for method e):
``python evaluate.py -d DATA -m OUT -sl im om`` and ``python recommend.py -d DATA -m OUT ...`` run on it as on any other.  The weights
are printed on stdout (method e: their mean over the users, one value per model).
"""
from __future__ import annotations

import argparse
import os

import numpy as np
import torch

import foldin
import fusion
import svmfusion
import textio
import tkr_hip


def main(argv=None):
    parser = argparse.ArgumentParser(description="Fuse trained models into one model directory.")
    parser.add_argument('-d', '--data', required=True, help="The data path (uid, vid, f{fold}tr.txt)")
    parser.add_argument('-m', '--models', required=True, nargs='+', help="The model directories to fuse")
    parser.add_argument('-o', '--out', required=True, help="The directory of the fused model")
    parser.add_argument('-f', '--fold', type=int, default=0, help="The index of the training fold (methods b, e and s)")
    parser.add_argument('--method', required=True, choices=fusion.METHODS + svmfusion.METHODS,
                        help="a: average, p: geometric, b: BPR on the scores, e: per-user RMSE, w: given, s: linear SVM on the scores")
    parser.add_argument('--p', type=float, default=0.5, help="Method p: the ratio of the geometric weights")
    parser.add_argument('--weights', type=float, nargs='+', default=None, help="Method w: one weight per model")
    parser.add_argument('--samples', type=int, default=None, help="Methods b and s: the number of sampled triplets (default: b 10,000,000, s 1,000,000)")
    parser.add_argument('--batch', type=int, default=10_000, help="Method b: the batch size")
    parser.add_argument('--lr', type=float, default=1e-4, help="Method b: the learning rate")
    parser.add_argument('--lambda-w', type=float, default=0.0025, help="Method b: the regulariser of the weights")
    parser.add_argument('--svm-c', type=float, default=0.01, help="Method s: the C of the SVM")
    parser.add_argument('--seed', type=int, default=0, help="Methods b and s: the seed of the triplets")
    args = parser.parse_args(argv)
    if args.samples is None:
        args.samples = 1_000_000 if args.method == 's' else 10_000_000
    M = len(args.models)
    if M > tkr_hip.FUSION_MAX_MODELS:
        parser.error('at most %d models' % tkr_hip.FUSION_MAX_MODELS)
    if args.method == 'w' and (args.weights is None or len(args.weights) != M):
        parser.error('--method w needs --weights with one value per model')
    if args.method == 'p' and not 0.0 < args.p < 1.0:
        parser.error('--p must lie inside (0, 1)')
    if args.method == 'b' and (args.batch < 1 or args.samples < 0):
        parser.error('--batch must be at least 1 and --samples non-negative')
    if args.method == 's' and (args.samples < 1 or not args.svm_c > 0.0):
        parser.error('--samples must be at least 1 and --svm-c positive')
    if args.method in ('b', 'e', 's') and not torch.cuda.is_available():
        raise tkr_hip.TkrError('fuse.py learns the weights on the GPU through libtkr_hip.so; no MI355X is visible')

    models = fusion.load_models(args.data, args.models)
    n_users, n_items = models[0][0].shape[0], models[0][1].shape[0]
    meta = dict(method=args.method, models=[os.path.abspath(m) for m in args.models], fold=args.fold)
    user_weights = None
    tr_file = os.path.join(args.data, 'f%dtr.txt' % args.fold)
    if args.method in ('a', 'p', 'w'):
        w = fusion.fixed_weights(M, args.method, p=args.p, weights=args.weights)
        if args.method == 'p':
            meta['p'] = args.p
    elif args.method in ('b', 's'):
        from single import BPR
        device = torch.device('cuda', torch.cuda.current_device())
        data = BPR(k=1)                                              # the training likes as BPR.train draws from them
        data.load_training_data(os.path.join(args.data, 'uid'), os.path.join(args.data, 'vid'), tr_file)
        if not data.tr_users:
            raise ValueError('%s holds no training like of a known user and item' % tr_file)
        csr = data._make_csr(data.tr_users, device)
        if args.method == 's':
            w, info = svmfusion.learn_svm(models, csr, n_items, n_samples=args.samples, C=args.svm_c, seed=args.seed, want_info=True)
            meta.update(C=args.svm_c, samples=args.samples, seed=args.seed, intercept=info['intercept'], iterations=info['iterations'],
                        grad_norm=info['grad'], active=info['active'], objective=info['objective'])
        else:
            w = fusion.learn_pairwise(models, csr, n_items, n_samples=args.samples, batch_size=args.batch, lr=args.lr, lambda_w=args.lambda_w,
                                      seed=args.seed)
            B = min(args.batch, csr.nnz)
            meta.update(samples=args.samples, batch=B, lr=args.lr, lambda_w=args.lambda_w, seed=args.seed,
                        n_batches=fusion.n_batches_of(args.samples, B))
    else:
        from evaluate import read_ids
        uids, vids = read_ids(os.path.join(args.data, 'uid')), read_ids(os.path.join(args.data, 'vid'))
        ptr, cols = foldin.liked_csr(textio.parse_ratings(tr_file, uids, vids), n_users, n_items)
        user_weights, _ = fusion.learn_per_user(models, ptr, cols)
        w = user_weights.mean(axis=0, dtype=np.float64).astype(np.float32)
    meta['weights'] = [float(x) for x in w]                          # method e: the mean over the users; final-W.dat has every user's
    U, V = fusion.fuse(models, user_weights if user_weights is not None else w)
    fusion.write_fused(args.out, U, V, meta, user_weights=user_weights)
    print(' '.join('%.9g' % float(x) for x in w))
    return user_weights if user_weights is not None else w


if __name__ == '__main__':
    main()
