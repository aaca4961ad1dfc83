"""Training driver for WMF, CER and DPM -- the reference's train.py:18-36 with its constants as options:

    cd top-k-rec_amd && python train_als.py -d data -o embed/wmf -k 50 --iters 200 --tol 1e-4
    cd top-k-rec_amd && python train_als.py -d data -o embed/wmf256 -k 256 --solver cg --cg-steps 3
    cd top-k-rec_amd && python train_als.py --model cer --content data/meta.pkl --dim 20000 -d data -o embed/cer -k 50
    cd top-k-rec_amd && python train_als.py --model cer --estep cg --e-steps 8 --content data/meta.pkl --dim 200000 -d data -o embed/cer -k 50
    cd top-k-rec_amd && python train_als.py --model dpm --content data/meta.pkl --dim 20000 -d data -o embed/dpm -k 50 --hidden 2000 1000

reads DATA/uid, DATA/vid and DATA/f<FOLD>tr.txt, trains als.WMF (or als.CER / als.DPM, with the pickled content features of --content,
their rows in the order of DATA/vid) on the GPU and writes OUT/final-U.dat and OUT/final-V.dat (CER: and OUT/final-E.dat; DPM: and
OUT/mlp.npz, the encoder), a model directory for evaluate.py, recommend.py and fuse.py.  An OUT that already holds a model is the warm
start (train.py:22, wmf.py:65-66).  DPM runs all --iters iterations: dpm.py has no stopping test, --tol is not looked at.
"""
import argparse
import os

from als import CER, DPM, MLP, WMF


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('-d', '--data', default='data', help='directory with uid, vid and f<FOLD>tr.txt')
    ap.add_argument('-o', '--out', default='embed/wmf', help='model directory to write (read first when it holds a model)')
    ap.add_argument('-k', type=int, default=50, help="factors, at most 128 (512 for wmf and cer under --solver cg)")
    ap.add_argument('--solver', choices=('cholesky', 'cg'), default='cholesky', help='the half-step: per-row Gram + Cholesky (K20), or conjugate gradients (K24)')
    ap.add_argument('--cg-steps', type=int, default=3, metavar='N', help='--solver cg: steps of conjugate gradients per half-step')
    ap.add_argument('--iters', type=int, default=200, help='iterations at most (max_iter)')
    ap.add_argument('--tol', type=float, default=1e-4, help='stop when the loss changes by less than this, relatively')
    ap.add_argument('--lu', type=float, default=0.01)
    ap.add_argument('--lv', type=float, default=None, help="default: the model's own, 0.01 for wmf and 10 for cer and dpm")
    ap.add_argument('--model', choices=('wmf', 'cer', 'dpm'), default='wmf')
    ap.add_argument('--content', default=None, metavar='FILE', help='cer, dpm: the pickled [n, d] content features (dense or scipy sparse)')
    ap.add_argument('--dim', type=int, default=None, metavar='D', help='cer, dpm: the width d of the content features')
    ap.add_argument('--le', type=float, default=10e3, help='cer: the ridge of the content projection E')
    ap.add_argument('--estep', choices=('cholesky', 'cg'), default=None,
                    help='cer: the E-step: a dense d x d Cholesky factor (K21, the default), or conjugate gradients on the sparse features (K26)')
    ap.add_argument('--e-steps', type=int, default=None, metavar='N', help='cer, --estep cg: steps of conjugate gradients per E-step (default 8)')
    ap.add_argument('--hidden', type=int, nargs='*', default=None, metavar='H', help="dpm: the encoder's hidden widths (default 2000 1000)")
    ap.add_argument('--mlp-lr', type=float, default=None, help="dpm: the encoder's RMSProp learning rate (default 1e-4)")
    ap.add_argument('--batch', type=int, default=None, help="dpm: the encoder's mini-batch, at most 256 (default 64)")
    ap.add_argument('--mlp-seed', type=int, default=None, help="dpm: seed of the encoder's start and epoch orders (default: --seed)")
    ap.add_argument('--a', type=float, default=1.0, help='weight of a like')
    ap.add_argument('--b', type=float, default=0.01, help='weight of an unobserved pair')
    ap.add_argument('--seed', type=int, default=None, help='seed of the uniform [0, 1) start')
    ap.add_argument('-f', '--fold', type=int, default=0)
    args = ap.parse_args(argv)
    cer, dpm = args.model == 'cer', args.model == 'dpm'
    if (cer or dpm) != (args.content is not None):
        ap.error('--content FILE goes with --model cer or dpm, and they need it')
    if (cer or dpm) and args.dim is None:
        ap.error('--model %s needs --dim D, the width of the content features' % args.model)
    if not dpm and (args.hidden is not None or args.mlp_lr is not None or args.batch is not None or args.mlp_seed is not None):
        ap.error('--hidden, --mlp-lr, --batch and --mlp-seed go with --model dpm')
    if not cer and (args.estep is not None or args.e_steps is not None):
        ap.error('--estep and --e-steps go with --model cer: the E-step is the ridge regression of its content projection')
    if args.e_steps is not None and args.estep != 'cg':
        ap.error('--e-steps N goes with --estep cg')
    lv = args.lv if args.lv is not None else (10.0 if cer or dpm else 0.01)
    encoder, batch = None, 64 if args.batch is None else args.batch
    how = dict(solver=args.solver, cg_steps=args.cg_steps)
    try:
        if dpm:
            if not 1 <= batch <= 256:
                raise ValueError('--batch %d: 1 <= batch <= 256 is supported' % batch)
            model = DPM(k=args.k, d=args.dim, lu=args.lu, lv=lv, le=args.le, a=args.a, b=args.b, **how)
            encoder = MLP(args.k, args.dim, lr=1e-4 if args.mlp_lr is None else args.mlp_lr, hidden_layers=(2000, 1000) if args.hidden is None else args.hidden,
                          seed=args.seed if args.mlp_seed is None else args.mlp_seed)
        elif cer:
            if args.estep is not None:
                how['estep'] = args.estep
            if args.e_steps is not None:
                how['e_steps'] = args.e_steps
            model = CER(k=args.k, d=args.dim, lu=args.lu, lv=lv, le=args.le, a=args.a, b=args.b, **how)
        else:
            model = WMF(k=args.k, lu=args.lu, lv=lv, a=args.a, b=args.b, **how)
    except ValueError as e:
        ap.error(str(e))
    model.load_training_data(os.path.join(args.data, 'uid'), os.path.join(args.data, 'vid'), os.path.join(args.data, 'f%dtr.txt' % args.fold),
                             seed=args.seed)
    if cer or dpm:
        model.load_content_data(args.content, os.path.join(args.data, 'vid'))
    model_path = args.out if os.path.isdir(args.out) else None
    if dpm:
        model.train(encoder, max_iter=args.iters, model_path=model_path, batch_size=batch)
    else:
        model.train(max_iter=args.iters, tol=args.tol, model_path=model_path)
    parent = os.path.dirname(os.path.abspath(args.out))
    if not os.path.isdir(parent):
        os.makedirs(parent)                                       # (export_embeddings makes OUT itself, not its parents)
    model.export_embeddings(args.out)
    return model


if __name__ == '__main__':
    main()
