"""NumPy oracle of K12 (tkr_rank_candidates), tkr_hip.topk_from_ranks, recommend.py --candidates and evaluate.py --negatives: the
scores through oracle.ref_np.mfma_chain_scores, the ranks by their definition (a loop over pairs), the metrics by a loop over rows.
Not a test module."""
import math
import os

import numpy as np

from oracle import ref_np as R


def csr(rows, dtype=np.int32):
    ptr = np.zeros(len(rows) + 1, np.int64)
    np.cumsum([len(x) for x in rows], out=ptr[1:])
    cols = np.concatenate([np.asarray(x, dtype) for x in rows] + [np.zeros(0, dtype)]).astype(dtype)
    return ptr, cols


def scores_np(U, V, bias, user_rows, cands, full=None):
    """the chain score of every (row, candidate): a list of fp32 arrays.  full: mfma_chain_scores(U, V, bias), when the caller has it"""
    s = R.mfma_chain_scores(np.asarray(U)[np.asarray(user_rows)], V, bias) if full is None else full[np.asarray(user_rows)]
    return [s[r][np.asarray(c, dtype=np.int64)] for r, c in enumerate(cands)]


def ranks_of(scores, cols, masked):
    """one list: -1 for a masked entry, otherwise the number of unmasked other entries with a larger score, or an equal score and a
    larger column"""
    out = []
    for e in range(len(cols)):
        if masked[e]:
            out.append(-1)
            continue
        out.append(sum(1 for f in range(len(cols))
                       if f != e and not masked[f] and (scores[f] > scores[e] or (scores[f] == scores[e] and cols[f] > cols[e]))))
    return np.array(out, dtype=np.int32)


def ranks_fast(scores, cols, masked):
    """the same by broadcasting (long lists)"""
    s, c, m = np.asarray(scores), np.asarray(cols), np.asarray(masked, dtype=bool)
    ahead = (s[None, :] > s[:, None]) | ((s[None, :] == s[:, None]) & (c[None, :] > c[:, None]))
    r = (ahead & ~m[None, :]).sum(axis=1).astype(np.int32)
    r[m] = -1
    return r


def ranks_sorted(scores, cols, masked):
    """the same from one sort (lists too long for the pair matrix): ascending by (score, column), read backwards"""
    s, c, m = np.asarray(scores), np.asarray(cols), np.asarray(masked, dtype=bool)
    order = np.lexsort((c, s))[::-1]
    order = order[~m[order]]
    r = np.full(len(c), -1, dtype=np.int32)
    r[order] = np.arange(len(order), dtype=np.int32)
    return r


def rank_candidates_np(U, V, bias, user_rows, cands, rated=None, full=None):
    """-> (scores fp32 [nnz], ranks int32 [nnz]) in CSR order; rated: per row, the masked columns"""
    sc = scores_np(U, V, bias, user_rows, cands, full)
    ranks = []
    for r, c in enumerate(cands):
        masked = np.isin(c, np.asarray(list(rated[r]), dtype=np.int64)) if rated is not None else np.zeros(len(c), dtype=bool)
        ranks.append(ranks_of(sc[r], c, masked) if len(c) <= 20 else ranks_fast(sc[r], c, masked) if len(c) <= 4096 else ranks_sorted(sc[r], c, masked))
    return (np.concatenate(sc + [np.zeros(0, np.float32)]).astype(np.float32),
            np.concatenate(ranks + [np.zeros(0, np.int32)]).astype(np.int32))


def topk_from_ranks_np(ptr, cols, scores, ranks, K):
    n = len(ptr) - 1
    ids = np.full((n, K), -1, dtype=np.int32)
    out = np.full((n, K), -np.inf, dtype=np.float32)
    for r in range(n):
        for e in range(int(ptr[r]), int(ptr[r + 1])):
            if 0 <= ranks[e] < K:
                ids[r, ranks[e]] = cols[e]
                out[r, ranks[e]] = scores[e]
    return ids, out


def negative_values(like_ranks, step, total):
    """{metric: list of values} of hr / ndcg / mrr from the rank of every row's like, row by row"""
    grid = [step * (b + 1) for b in range(total // step)]
    hr, ndcg, mrr = [0.0] * len(grid), [0.0] * len(grid), 0.0
    for r in like_ranks:
        r = int(r)
        mrr += 1.0 / (r + 1)
        for b, K in enumerate(grid):
            if r < K:
                hr[b] += 1.0
                ndcg[b] += 1.0 / math.log2(r + 2)
    n = len(like_ranks)
    return {'hr': [v / n for v in hr], 'ndcg': [v / n for v in ndcg], 'mrr': [mrr / n]}


def read_test_lines(path, teids):
    """per test line: (uid, liked columns, every known column on the line)"""
    out = []
    with open(path) as fh:
        for line in fh:
            fields = line.strip().split(',')
            likes, seen = set(), set()
            for tok in fields[1:]:
                vid, like = tok.split(':')[0], int(tok.split(':')[1])
                if vid in teids:
                    seen.add(teids[vid])
                    if like == 1:
                        likes.add(teids[vid])
            out.append((fields[0], likes, seen))
    return out


def negatives_inputs(data_dir, fold, scenario):
    """what rankmetrics.sample_negatives takes for one scenario, read the reference's way: the test lines with at least one like, in
    file order; per line the likes that are not train-rated, and the excluded columns (train-rated or on the line)
    -> (uid index of every line, like rows, excluded rows, n_cols)"""
    uids = R.read_id_list(os.path.join(data_dir, 'uid'))
    rated = R.read_history(os.path.join(data_dir, 'f%dtr.txt' % fold))
    teids = R.read_id_list(os.path.join(data_dir, 'f%dte.%s.idl' % (fold, scenario)))
    users, likes, excluded = [], [], []
    for uid, liked, seen in read_test_lines(os.path.join(data_dir, 'f%dte.%s.txt' % (fold, scenario)), teids):
        if not liked:
            continue
        r = {teids[v] for v in rated[uid] if v in teids}
        users.append(uids[uid])
        likes.append(sorted(liked - r))
        excluded.append(sorted(r | seen))
    return users, likes, excluded, len(teids)


def scenario_factors(data_dir, model_dir, fold, scenario):
    uids = R.read_id_list(os.path.join(data_dir, 'uid'))
    vids = R.read_id_list(os.path.join(data_dir, 'vid'))
    teids = R.read_id_list(os.path.join(data_dir, 'f%dte.%s.idl' % (fold, scenario)))
    umat = R.read_embed_text(os.path.join(model_dir, 'final-U.dat'), uids)
    vmat = R.read_embed_text(os.path.join(model_dir, 'final-V.dat'), vids)
    bpath = os.path.join(model_dir, 'final-B.dat')
    bmat = R.read_embed_text(bpath, vids) if os.path.exists(bpath) else None
    temat = np.zeros((len(teids), vmat.shape[1]), dtype=np.float32)
    tebias = np.zeros(len(teids), dtype=np.float32) if bmat is not None else None
    for vid, col in teids.items():
        temat[col] = vmat[vids[vid]]
        if bmat is not None:
            tebias[col] = bmat.reshape(-1)[vids[vid]]
    return umat, temat, tebias


def negatives_lines(data_dir, model_dir, fold, step, total, scenarios, n_neg, seed, metrics, sample_negatives):
    """the lines evaluate.py -M ... --negatives prints after the others: 'S.negN.metric,%.6f[,...]'; the rows come from
    `sample_negatives` (rankmetrics.sample_negatives), scores, ranks and metrics from this module"""
    out = []
    for sc in scenarios:
        users, likes, excluded, n_cols = negatives_inputs(data_dir, fold, sc)
        umat, temat, tebias = scenario_factors(data_dir, model_dir, fold, sc)
        cand_ptr, cand_cols, like_at = sample_negatives(*csr(likes, np.int64), *csr(excluded, np.int64), n_cols, n_neg, seed)
        row_user = np.repeat(np.asarray(users, dtype=np.int64), [len(x) for x in likes])
        s = R.mfma_chain_scores(umat, temat, tebias)
        like_ranks = []
        for q in range(len(cand_ptr) - 1):
            cols = cand_cols[cand_ptr[q]:cand_ptr[q + 1]]
            r = ranks_of(s[row_user[q]][cols], cols, np.zeros(len(cols), dtype=bool))
            like_ranks.append(int(r[like_at[q] - cand_ptr[q]]))
        vals = negative_values(like_ranks, step, total)
        for m in metrics:
            out.append('%s.neg%d.%s' % (sc, n_neg, m) + ''.join(',%.6f' % v for v in vals[m]))
    return out, like_ranks
