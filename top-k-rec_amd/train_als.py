"""Training driver for WMF -- the reference's train.py:18-22 with its constants as options:

    cd top-k-rec_amd && python train_als.py -d data -o embed/wmf -k 50 --iters 200 --tol 1e-4

reads DATA/uid, DATA/vid and DATA/f<FOLD>tr.txt, trains als.WMF on the GPU and writes OUT/final-U.dat and OUT/final-V.dat, a model
directory for evaluate.py, recommend.py and fuse.py.  An OUT that already holds a model is the warm start (train.py:22, wmf.py:65-66).
"""
import argparse
import os

from als import WMF


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('-d', '--data', default='data', help='directory with uid, vid and f<FOLD>tr.txt')
    ap.add_argument('-o', '--out', default='embed/wmf', help='model directory to write (read first when it holds a model)')
    ap.add_argument('-k', type=int, default=50, help='factors, at most 128')
    ap.add_argument('--iters', type=int, default=200, help='iterations at most (max_iter)')
    ap.add_argument('--tol', type=float, default=1e-4, help='stop when the loss changes by less than this, relatively')
    ap.add_argument('--lu', type=float, default=0.01)
    ap.add_argument('--lv', type=float, default=0.01)
    ap.add_argument('--a', type=float, default=1.0, help='weight of a like')
    ap.add_argument('--b', type=float, default=0.01, help='weight of an unobserved pair')
    ap.add_argument('--seed', type=int, default=None, help='seed of the uniform [0, 1) start')
    ap.add_argument('-f', '--fold', type=int, default=0)
    args = ap.parse_args(argv)
    try:
        model = WMF(k=args.k, lu=args.lu, lv=args.lv, a=args.a, b=args.b)
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
