"""Training driver for ItemKNN, the item-neighbourhood model (K28), after train_lmf.py:

    cd top-k-rec_amd && python train_knn.py -d data -o embed/knn
    cd top-k-rec_amd && python train_knn.py -d data -o embed/knn -N 100 --shrink 0 --similarity cosine -f 0

reads DATA/uid, DATA/vid and DATA/f<FOLD>tr.txt, builds knn.ItemKNN on the GPU in one pass over the likes and writes OUT/knn.npz (the
neighbour table, the likers per item, the hyper-parameters): a model directory for evaluate.py and recommend.py.  There is nothing to
warm-start and no seed.
"""
import argparse
import os

from knn import SIMILARITIES, ItemKNN


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('-d', '--data', default='data', help='directory with uid, vid and f<FOLD>tr.txt')
    ap.add_argument('-o', '--out', default='embed/knn', help='model directory to write')
    ap.add_argument('-N', '--neighbors', type=int, default=100, help='neighbours kept per item, at most 512')
    ap.add_argument('--shrink', type=float, default=0.0, help='added to the denominator of the cosine')
    ap.add_argument('--similarity', default='cosine', choices=SIMILARITIES, help='cosine, or cooc: the raw co-occurrence count')
    ap.add_argument('-f', '--fold', type=int, default=0)
    args = ap.parse_args(argv)
    try:
        model = ItemKNN(n_neighbors=args.neighbors, shrink=args.shrink, similarity=args.similarity)
    except ValueError as e:
        ap.error(str(e))
    model.load_training_data(os.path.join(args.data, 'uid'), os.path.join(args.data, 'vid'), os.path.join(args.data, 'f%dtr.txt' % args.fold))
    model.train()
    model.export_model(args.out)
    return model


if __name__ == '__main__':
    main()
