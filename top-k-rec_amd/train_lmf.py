"""Training driver for LMF, logistic matrix factorisation (K25), after train_als.py:

    cd top-k-rec_amd && python train_lmf.py -d data -o embed/lmf -k 30 --iters 30
    cd top-k-rec_amd && python train_lmf.py -d data -o embed/lmf -k 64 --iters 50 --lam 0.6 --alpha 20 --lr 1.0 --tol 1e-4 --seed 0

reads DATA/uid, DATA/vid and DATA/f<FOLD>tr.txt, trains lmf.LMF on the GPU and writes OUT/final-U.dat, OUT/final-V.dat, OUT/final-B.dat
(the item biases) and OUT/lmf.npz (user biases, AdaGrad slots, hyper-parameters), a model directory for evaluate.py, recommend.py and
fuse.py.  An OUT that already holds a model is the warm start: training continues with its slots.  Without --alpha the weight of a like
is the value that balances the likes against all other pairs; without --tol all --iters iterations run.
"""
import argparse
import os

from lmf import LMF


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('-d', '--data', default='data', help='directory with uid, vid and f<FOLD>tr.txt')
    ap.add_argument('-o', '--out', default='embed/lmf', help='model directory to write (read first when it holds a model)')
    ap.add_argument('-k', type=int, default=30, help='factors, at most 128')
    ap.add_argument('--iters', type=int, default=30, help='iterations at most (max_iter)')
    ap.add_argument('--lam', type=float, default=0.6, help='the regulariser of factors and biases')
    ap.add_argument('--alpha', type=float, default=None, help='weight of a like (default: the value that balances the two classes)')
    ap.add_argument('--lr', type=float, default=1.0, help="AdaGrad's step")
    ap.add_argument('--tol', type=float, default=None, help='stop when the loss changes by less than this, relatively (default: run all iterations)')
    ap.add_argument('--seed', type=int, default=None, help='seed of the N(0, 0.01) start')
    ap.add_argument('-f', '--fold', type=int, default=0)
    args = ap.parse_args(argv)
    try:
        model = LMF(k=args.k, lam=args.lam, alpha=args.alpha, lr=args.lr)
    except ValueError as e:
        ap.error(str(e))
    model.load_training_data(os.path.join(args.data, 'uid'), os.path.join(args.data, 'vid'), os.path.join(args.data, 'f%dtr.txt' % args.fold),
                             seed=args.seed)
    model.train(max_iter=args.iters, tol=args.tol, model_path=args.out if os.path.isdir(args.out) else None)
    parent = os.path.dirname(os.path.abspath(args.out))
    if not os.path.isdir(parent):
        os.makedirs(parent)                                       # (export_embeddings makes OUT itself, not its parents)
    model.export_embeddings(args.out)
    return model


if __name__ == '__main__':
    main()
