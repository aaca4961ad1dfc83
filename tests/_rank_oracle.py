"""NumPy oracle of the full-rank evaluation (K8 + rankmetrics.py): filtered ranks from a stable argsort read backwards, and every
metric by a direct loop over the ranked list -- no formula shared with top-k-rec_amd/rankmetrics.py.  Not a test module."""
import math
import os

import numpy as np

from oracle import ref_np as R

METRICS = ('acc', 'auc', 'mrr', 'ndcg', 'map')


def kept_order(scores_row, rated):
    """the unrated columns in the canonical order: descending score, ties -> higher column first"""
    order = np.argsort(np.asarray(scores_row), kind='stable')[::-1]
    if len(rated) == 0:
        return order
    is_rated = np.zeros(len(order), dtype=bool)
    is_rated[np.fromiter(rated, dtype=np.int64, count=len(rated))] = True
    return order[~is_rated[order]]


def like_ranks_np(scores_row, rated, likes):
    """filtered rank of every like in ascending column order; -1 for a like that is rated"""
    kept = kept_order(scores_row, rated)
    pos = np.full(len(scores_row), -1, dtype=np.int64)
    pos[kept] = np.arange(len(kept))
    return pos[np.sort(np.fromiter(likes, dtype=np.int64, count=len(likes)))]


def raw_ranks_np(scores_row, rated_cols, kept_ids):
    """what K6 (tkr_raw_ranks) returns for one row: for every entry of kept_ids (unrated columns, -1 padded) its position among ALL
    columns of the row in the canonical order, rated ones counted; a -1 stays -1"""
    order = np.argsort(np.asarray(scores_row), kind='stable')[::-1]
    pos = np.empty(len(order), dtype=np.int64)
    pos[order] = np.arange(len(order))
    kept = np.asarray(kept_ids, dtype=np.int64)
    live = kept >= 0
    assert not np.isin(kept[live], np.asarray(list(rated_cols), dtype=np.int64)).any(), 'a kept column is rated'
    out = np.full(len(kept), -1, dtype=np.int32)
    out[live] = pos[kept[live]]
    return out


def load_lines(data_dir, model_dir, fold, scenario, scoring='blas'):
    """the reference's view of one scenario -> (scores [n_users, n_cols], [(user row, rated column set, liked column set)]) for the
    test lines with at least one like.  scoring: 'blas' (np.dot, as evaluate.py:78), 'chain' (the kernels' fma chain), 'f64'"""
    uids = R.read_id_list(os.path.join(data_dir, 'uid'))
    vids = R.read_id_list(os.path.join(data_dir, 'vid'))
    rated = R.read_history(os.path.join(data_dir, 'f%dtr.txt' % fold))
    umat = R.read_embed_text(os.path.join(model_dir, 'final-U.dat'), uids)
    vmat = R.read_embed_text(os.path.join(model_dir, 'final-V.dat'), vids)
    bpath = os.path.join(model_dir, 'final-B.dat')
    bmat = R.read_embed_text(bpath, vids) if os.path.exists(bpath) else None
    teids = R.read_id_list(os.path.join(data_dir, 'f%dte.%s.idl' % (fold, scenario)))
    tests = R.read_test_likes(os.path.join(data_dir, 'f%dte.%s.txt' % (fold, scenario)), teids)
    if scoring == 'blas':
        scores = R.scenario_scores(umat, vmat, bmat, vids, teids)
    else:
        temat = np.zeros((len(teids), vmat.shape[1]), dtype=np.float32)
        tebias = np.zeros(len(teids), dtype=np.float32)
        for vid, col in teids.items():
            temat[col] = vmat[vids[vid]]
            if bmat is not None:
                tebias[col] = bmat.reshape(-1)[vids[vid]]
        if scoring == 'chain':
            scores = R.mfma_chain_scores(umat, temat, tebias if bmat is not None else None)
        else:
            scores = umat.astype(np.float64) @ temat.astype(np.float64).T + tebias.astype(np.float64)
    lines = []
    for uid, likes in tests:
        if len(likes):
            lines.append((uids[uid], {teids[v] for v in rated[uid] if v in teids}, set(likes)))
    return scores, lines


def csr_ranks(scores, lines):
    """-> (ranks in like-CSR order, like_ptr, rated_ptr): what K8 returns for these lines and what rankmetrics.rank_sums takes"""
    ranks, like_ptr, rated_ptr = [], [0], [0]
    for row, rated, likes in lines:
        ranks.extend(like_ranks_np(scores[row], rated, likes).tolist())
        like_ptr.append(like_ptr[-1] + len(likes))
        rated_ptr.append(rated_ptr[-1] + len(rated))
    return np.array(ranks, dtype=np.int64), np.array(like_ptr, dtype=np.int64), np.array(rated_ptr, dtype=np.int64)


def direct_sums(scores, lines, step, total):
    """{metric: (sum, count)} by walking every line's ranked list: hits per bucket as evaluate.py:99-103, AUC as a count of
    (like, non-like) pairs in the right order, reciprocal rank of the first like, DCG / ideal DCG and average precision at
    K = step, 2 step, ..."""
    interval = total // step
    grid = [step * (b + 1) for b in range(interval)]
    hits, n_likes = [0] * interval, 0
    auc_sum, auc_n, mrr_sum, lines_n = 0.0, 0, 0.0, 0
    ndcg, ap = [0.0] * interval, [0.0] * interval
    for row, rated, likes in lines:
        kept = [int(c) for c in kept_order(scores[row], rated)]
        n_likes += len(likes)
        h = R.bucket_hits(kept[:total], likes, step, interval)
        hits = [a + b for a, b in zip(hits, h)]
        rel = [c in likes for c in kept]
        P = sum(rel)
        if P == 0:
            continue
        lines_n += 1
        mrr_sum += 1.0 / (rel.index(True) + 1)
        right = pairs = 0
        for a, ra in enumerate(rel):                               # every (like, non-like) pair: right when the like comes first
            if ra:
                for b, rb in enumerate(rel):
                    if not rb:
                        pairs += 1
                        right += a < b
        if pairs:
            auc_sum += right / pairs
            auc_n += 1
        for b, K in enumerate(grid):
            dcg = sum(1.0 / math.log2(p + 2) for p in range(min(K, len(rel))) if rel[p])
            idcg = sum(1.0 / math.log2(p + 2) for p in range(min(P, K)))
            ndcg[b] += dcg / idcg
            seen, prec = 0, 0.0
            for p in range(min(K, len(rel))):
                if rel[p]:
                    seen += 1
                    prec += seen / (p + 1)
            ap[b] += prec / min(P, K)
    return {'acc': (np.array(hits, dtype=np.int64), n_likes), 'auc': (auc_sum, auc_n), 'mrr': (mrr_sum, lines_n),
            'ndcg': (np.array(ndcg), lines_n), 'map': (np.array(ap), lines_n)}


def metric_lines(data_dir, model_dir, fold, step, total, scenarios, metrics=METRICS):
    """the lines evaluate.py -M prints after the reference's: 'S.metric,%.6f[,...]' per scenario, per metric"""
    out = []
    for sc in scenarios:
        scores, lines = load_lines(data_dir, model_dir, fold, sc)
        sums = direct_sums(scores, lines, step, total)
        for m in metrics:
            s, c = sums[m]
            out.append('%s.%s' % (sc, m) + ''.join(',%.6f' % (float(v) / c) for v in np.asarray(s, dtype=np.float64).reshape(-1)))
    return out
