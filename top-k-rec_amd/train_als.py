"""Training driver for WMF and CER -- the reference's train.py:18-29 with its constants as options:

    cd top-k-rec_amd && python train_als.py -d data -o embed/wmf -k 50 --iters 200 --tol 1e-4
    cd top-k-rec_amd && python train_als.py --model cer --content data/meta.pkl --dim 20000 -d data -o embed/cer -k 50

reads DATA/uid, DATA/vid and DATA/f<FOLD>tr.txt, trains als.WMF (or als.CER, with the pickled content features of --content, their rows
in the order of DATA/vid) on the GPU and writes OUT/final-U.dat and OUT/final-V.dat (CER: and OUT/final-E.dat), a model directory for
evaluate.py, recommend.py and fuse.py.  An OUT that already holds a model is the warm start (train.py:22, wmf.py:65-66).
"""
import argparse
import os

from als import CER, WMF


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('-d', '--data', default='data', help='directory with uid, vid and f<FOLD>tr.txt')
    ap.add_argument('-o', '--out', default='embed/wmf', help='model directory to write (read first when it holds a model)')
    ap.add_argument('-k', type=int, default=50, help='factors, at most 128')
    ap.add_argument('--iters', type=int, default=200, help='iterations at most (max_iter)')
    ap.add_argument('--tol', type=float, default=1e-4, help='stop when the loss changes by less than this, relatively')
    ap.add_argument('--lu', type=float, default=0.01)
    ap.add_argument('--lv', type=float, default=None, help="default: the model's own, 0.01 for wmf and 10 for cer")
    ap.add_argument('--model', choices=('wmf', 'cer'), default='wmf')
    ap.add_argument('--content', default=None, metavar='FILE', help='cer: the pickled [n, d] content features (dense or scipy sparse)')
    ap.add_argument('--dim', type=int, default=None, metavar='D', help='cer: the width d of the content features')
    ap.add_argument('--le', type=float, default=10e3, help='cer: the ridge of the content projection E')
    ap.add_argument('--a', type=float, default=1.0, help='weight of a like')
    ap.add_argument('--b', type=float, default=0.01, help='weight of an unobserved pair')
    ap.add_argument('--seed', type=int, default=None, help='seed of the uniform [0, 1) start')
    ap.add_argument('-f', '--fold', type=int, default=0)
    args = ap.parse_args(argv)
    cer = args.model == 'cer'
    if cer != (args.content is not None):
        ap.error('--content FILE goes with --model cer, and --model cer needs it')
    if cer and args.dim is None:
        ap.error('--model cer needs --dim D, the width of the content features')
    lv = args.lv if args.lv is not None else (10.0 if cer else 0.01)
    try:
        model = CER(k=args.k, d=args.dim, lu=args.lu, lv=lv, le=args.le, a=args.a, b=args.b) if cer else WMF(k=args.k, lu=args.lu, lv=lv, a=args.a, b=args.b)
    except ValueError as e:
        ap.error(str(e))
    model.load_training_data(os.path.join(args.data, 'uid'), os.path.join(args.data, 'vid'), os.path.join(args.data, 'f%dtr.txt' % args.fold),
                             seed=args.seed)
    if cer:
        model.load_content_data(args.content, os.path.join(args.data, 'vid'))
    model.train(max_iter=args.iters, tol=args.tol, model_path=args.out if os.path.isdir(args.out) else None)
    parent = os.path.dirname(os.path.abspath(args.out))
    if not os.path.isdir(parent):
        os.makedirs(parent)                                       # (export_embeddings makes OUT itself, not its parents)
    model.export_embeddings(args.out)
    return model


if __name__ == '__main__':
    main()
