"""Training driver for SMF, softmax matrix factorisation (K27), after train_lmf.py:

    cd top-k-rec_amd && python train_smf.py -d data -o embed/smf -k 30 --iters 30
    cd top-k-rec_amd && python train_smf.py -d data -o embed/smf -k 64 --iters 50 --lam 0.01 --lr 0.1 --tol 1e-4 --seed 0

reads DATA/uid, DATA/vid and DATA/f<FOLD>tr.txt, trains smf.SMF on the GPU and writes OUT/final-U.dat, OUT/final-V.dat, OUT/final-B.dat
(the item biases) and OUT/smf.npz (AdaGrad slots, hyper-parameters), a model directory for evaluate.py, recommend.py and fuse.py.  An
OUT that already holds a model is the warm start: training continues with its slots.  Without --tol all --iters iterations run.
"""
import argparse
import os

from smf import SMF


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('-d', '--data', default='data', help='directory with uid, vid and f<FOLD>tr.txt')
    ap.add_argument('-o', '--out', default='embed/smf', help='model directory to write (read first when it holds a model)')
    ap.add_argument('-k', type=int, default=30, help='factors, at most 128')
    ap.add_argument('--iters', type=int, default=30, help='iterations at most (max_iter)')
    ap.add_argument('--lam', type=float, default=0.01, help='the regulariser of factors and biases')
    ap.add_argument('--lr', type=float, default=0.1, help="AdaGrad's step")
    ap.add_argument('--tol', type=float, default=None, help='stop when the loss changes by less than this, relatively (default: run all iterations)')
    ap.add_argument('--seed', type=int, default=None, help='seed of the N(0, 0.01) start')
    ap.add_argument('-f', '--fold', type=int, default=0)
    args = ap.parse_args(argv)
    try:
        model = SMF(k=args.k, lam=args.lam, lr=args.lr)
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
