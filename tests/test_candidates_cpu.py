"""K12 (tkr_rank_candidates) without a GPU: the ABI and the wrapper's refusals, the negatives' draw (rankmetrics.sample_negatives), the
metric sums against hand-worked ranks, and the parser errors of recommend.py --candidates and evaluate.py --negatives."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _candidates_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

CAND_ARGTYPES = [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p,
                 C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p]


def test_header_binding_and_library_declare_rank_candidates():
    import tkr_hip
    header = open(os.path.join(ROOT, 'include', 'tkr.h')).read()
    assert 'tkr_rank_candidates' in re.findall(r'^int(?:32_t|64_t)? (tkr_\w+)\(', header, flags=re.M)
    assert int(re.search(r'#define TKR_CANDIDATES_RESIDENT (\d+)', header).group(1)) == tkr_hip.CANDIDATES_RESIDENT
    assert 'tkr_rank_candidates' in tkr_hip.EXPORTS and callable(tkr_hip.rank_candidates) and callable(tkr_hip.topk_from_ranks)
    fn = C.CDLL(tkr_hip.LIB_PATH).tkr_rank_candidates
    fn.restype = C.c_int
    fn.argtypes = CAND_ARGTYPES
    # arguments are checked before any device access and before any launch: this runs on a machine without a GPU
    assert fn(None, None, 0, None, None, 0, 0, None, None, None, 0, None, None, None) == -1
    p = 4096                                                          # never dereferenced: every call below fails its checks
    good = dict(U=p, idx=None, n_rows=4, Vt=p, bias=None, n_cols=50, k=8, ptr=p, cols=p, mask=None, pitch=0, s=p, r=p, stream=None)
    for change in (dict(U=None), dict(Vt=None), dict(ptr=None), dict(cols=None), dict(s=None), dict(r=None), dict(n_rows=0), dict(n_rows=-3),
                   dict(n_cols=0), dict(k=0), dict(k=-1), dict(mask=p, pitch=3)):
        assert fn(*dict(good, **change).values()) == -1, change


def test_wrapper_refuses_dtype_layout_and_device_before_any_device_access():
    import tkr_hip
    U, V = torch.zeros((4, 8)), torch.zeros((10, 8))
    ptr, cols = torch.tensor([0, 1, 2, 2, 3]), torch.tensor([1, 2, 3], dtype=torch.int32)
    with pytest.raises(TypeError, match='U must be torch.float32'):
        tkr_hip.rank_candidates(U.double(), V, ptr, cols)
    with pytest.raises(TypeError, match='Vt must be torch.float32'):
        tkr_hip.rank_candidates(U, V.half(), ptr, cols)
    with pytest.raises(TypeError, match='cand_ptr must be torch.int64'):
        tkr_hip.rank_candidates(U, V, ptr.int(), cols)
    with pytest.raises(TypeError, match='cand_cols must be torch.int32'):
        tkr_hip.rank_candidates(U, V, ptr, cols.long())
    with pytest.raises(TypeError, match='bias must be torch.float32'):
        tkr_hip.rank_candidates(U, V, ptr, cols, bias=torch.zeros(10, dtype=torch.float64))
    with pytest.raises(TypeError, match='user_idx must be torch.int32'):
        tkr_hip.rank_candidates(U, V, ptr, cols, user_idx=torch.zeros(4, dtype=torch.int64))
    with pytest.raises(TypeError, match='must be a tensor'):
        tkr_hip.rank_candidates(U, V, [0, 1, 2, 2, 3], cols)
    with pytest.raises(ValueError, match='Vt must be contiguous'):
        tkr_hip.rank_candidates(U, torch.zeros((8, 10)).t(), ptr, cols)
    with pytest.raises(ValueError, match='must live on the GPU'):      # host tensors: refused, never handed to the library
        tkr_hip.rank_candidates(U, V, ptr, cols)


def _lines(rng, n_lines, n_cols, n_like, n_excl):
    likes, excluded = [], []
    for _ in range(n_lines):
        ex = np.sort(rng.choice(n_cols, n_excl, replace=False))
        likes.append(np.sort(rng.choice(ex, n_like, replace=False)))      # the likes are on the line: excluded too
        excluded.append(ex)
    return likes, excluded


def _check_rows(likes, excluded, n_cols, N, out):
    cand_ptr, cand_cols, like_at = out
    q = 0
    for ln, (lk, ex) in enumerate(zip(likes, excluded)):
        eligible = n_cols - len(ex)
        for like in lk:
            row = cand_cols[cand_ptr[q]:cand_ptr[q + 1]]
            assert len(row) == 1 + min(N, eligible), (ln, like)
            assert np.all(np.diff(row) > 0) and row.min() >= 0 and row.max() < n_cols      # ascending: distinct
            assert cand_cols[like_at[q]] == like and cand_ptr[q] <= like_at[q] < cand_ptr[q + 1]
            neg = np.delete(row, like_at[q] - cand_ptr[q])
            assert not np.any(np.isin(neg, ex))                          # never train-rated, never on the test line
            q += 1
    assert q == len(cand_ptr) - 1 == len(like_at) and cand_ptr[0] == 0 and cand_ptr[-1] == len(cand_cols)
    assert cand_ptr.dtype == np.int64 and cand_cols.dtype == np.int32


@pytest.mark.parametrize('N', [1, 5, 20, 38, 39, 100])
def test_sample_negatives_rows_are_distinct_eligible_and_of_the_right_length(N):
    """60 columns, 21 excluded per line -> 39 eligible: fewer draws than half of them (the redraw path), more than half (the random
    order path), exactly all and more than all (every eligible column)"""
    import rankmetrics
    rng = np.random.Generator(np.random.PCG64(N))
    likes, excluded = _lines(rng, 40, 60, 3, 21)
    likes[7] = likes[7][:0]                                              # a line without a ranked like: no row
    excluded[9] = np.arange(60)                                          # nothing eligible: the like alone
    out = rankmetrics.sample_negatives(*O.csr(likes, np.int64), *O.csr(excluded, np.int64), 60, N, 11)
    _check_rows(likes, excluded, 60, N, out)
    again = rankmetrics.sample_negatives(*O.csr(likes, np.int64), *O.csr(excluded, np.int64), 60, N, 11)
    for a, b in zip(out, again):
        np.testing.assert_array_equal(a, b)                              # the same seed: the same rows
    other = rankmetrics.sample_negatives(*O.csr(likes, np.int64), *O.csr(excluded, np.int64), 60, N, 12)
    if N < 39:
        assert not np.array_equal(out[1], other[1])                      # another seed: other rows
    else:
        np.testing.assert_array_equal(out[1], other[1])                  # every eligible column: nothing left to the seed


def test_sample_negatives_mixed_lines_take_both_paths_in_one_call():
    import rankmetrics
    rng = np.random.Generator(np.random.PCG64(2))
    likes, excluded = [], []
    for n_excl in (2, 80, 95, 100, 40, 99):
        ex = np.sort(rng.choice(100, n_excl, replace=False))
        likes.append(ex[:2])
        excluded.append(ex)
    _check_rows(likes, excluded, 100, 10, rankmetrics.sample_negatives(*O.csr(likes, np.int64), *O.csr(excluded, np.int64), 100, 10, 5))


@pytest.mark.parametrize('n_excl,N', [(4, 3), (7, 3)])
def test_sample_negatives_draws_every_eligible_column_uniformly(n_excl, N):
    """12 columns, one like: 8 eligible columns at N = 3 (redraw path), 5 at N = 3 (random-order path).  Over 400 seeds a column is
    drawn Binomial(400, N / eligible) times: every count within 5 standard deviations (a fair draw leaves that band with
    probability < 1e-6 per column)"""
    import rankmetrics
    ex = np.arange(n_excl) * 12 // n_excl                               # spread over the range
    eligible = np.setdiff1d(np.arange(12), ex)
    count = np.zeros(12, dtype=np.int64)
    S = 400
    for seed in range(S):
        ptr, cols, at = rankmetrics.sample_negatives(np.array([0, 1]), ex[:1], np.array([0, n_excl]), ex, 12, N, seed)
        count[np.delete(cols, at[0])] += 1
    p = N / len(eligible)
    sd = np.sqrt(S * p * (1 - p))
    assert np.all(count[ex] == 0)
    assert np.all(np.abs(count[eligible] - S * p) <= 5 * sd), count


def test_negative_sums_against_hand_worked_ranks():
    import rankmetrics
    ranks = [0, 4, 5, 2, 30, 9]                                          # six rows; step 5, total 10: K = 5, 10
    sums = rankmetrics.negative_sums(ranks, 5, 10)
    l2 = np.log2
    assert sums['hr'][0].tolist() == [3.0, 5.0] and sums['hr'][1] == 6
    np.testing.assert_allclose(sums['ndcg'][0], [1 / l2(2) + 1 / l2(6) + 1 / l2(4), 1 / l2(2) + 1 / l2(6) + 1 / l2(4) + 1 / l2(7) + 1 / l2(11)],
                               rtol=1e-15)
    assert sums['mrr'] == (pytest.approx(1 + 1 / 5 + 1 / 6 + 1 / 3 + 1 / 31 + 1 / 10, rel=1e-15), 6)
    vals = rankmetrics.finish(sums, ('hr', 'ndcg', 'mrr'))
    want = O.negative_values(ranks, 5, 10)
    for m in ('hr', 'ndcg', 'mrr'):
        np.testing.assert_allclose(vals[m], want[m], rtol=1e-14)
    assert vals['hr'] == [0.5, 5 / 6]
    # the sums of two shards add up through the all-reduce vector
    a, b = rankmetrics.negative_sums(ranks[:2], 5, 10), rankmetrics.negative_sums(ranks[2:], 5, 10)
    both = rankmetrics.neg_from_vector(rankmetrics.neg_to_vector(a) + rankmetrics.neg_to_vector(b), 2)
    for m in ('hr', 'ndcg', 'mrr'):
        np.testing.assert_allclose(np.asarray(both[m][0]), np.asarray(sums[m][0]), rtol=1e-15)
        assert both[m][1] == 6
    with pytest.raises(ZeroDivisionError):
        rankmetrics.finish(rankmetrics.negative_sums([], 5, 10), ('hr',))


def test_oracle_ranks_and_topk_scatter_on_a_hand_worked_list():
    scores = np.array([0.5, 0.25, 0.5, 1.0, 0.25], np.float32)
    cols = np.array([2, 3, 7, 8, 9], np.int32)
    masked = np.array([False, False, False, True, False])
    r = O.ranks_of(scores, cols, masked)
    assert r.tolist() == [1, 3, 0, -1, 2]                                # ties: the higher column first; the masked 1.0 counts for nobody
    np.testing.assert_array_equal(O.ranks_fast(scores, cols, masked), r)
    np.testing.assert_array_equal(O.ranks_sorted(scores, cols, masked), r)
    rng = np.random.Generator(np.random.PCG64(4))                        # the three forms of the oracle agree where ties are many
    s2, m2 = rng.integers(-2, 3, 150).astype(np.float32), rng.random(150) < 0.2
    c2 = np.sort(rng.choice(1000, 150, replace=False)).astype(np.int32)
    np.testing.assert_array_equal(O.ranks_fast(s2, c2, m2), O.ranks_of(s2, c2, m2))
    np.testing.assert_array_equal(O.ranks_sorted(s2, c2, m2), O.ranks_of(s2, c2, m2))
    ids, out = O.topk_from_ranks_np(np.array([0, 5, 5]), cols, scores, r, 3)
    assert ids.tolist() == [[7, 2, 9], [-1, -1, -1]] and out[0].tolist() == [0.5, 0.5, 0.25] and np.all(np.isneginf(out[1]))


def test_cli_parser_errors(golden_dir, tmp_path, capsys):
    """refused on the host, before anything asks for a GPU"""
    import evaluate
    import recommend
    d = os.path.join(golden_dir, 'g4')
    data, model = os.path.join(d, 'data'), os.path.join(d, 'model')
    some = tmp_path / 'some'
    some.write_text('1\n')
    with pytest.raises(SystemExit):
        recommend.main(['-d', data, '-m', model, '-o', str(tmp_path / 'out.txt'), '-u', str(some), '--candidates', os.path.join(data, 'f0tr.txt')])
    assert '--candidates' in capsys.readouterr().err and not (tmp_path / 'out.txt').exists()
    with pytest.raises(SystemExit):
        evaluate.main(['-d', data, '-m', model, '-sl', 'im', '--negatives', '20'])            # without -M
    assert '--negatives needs -M' in capsys.readouterr().err
    with pytest.raises(SystemExit):
        evaluate.main(['-d', data, '-m', model, '-sl', 'im', '-M', 'hr'])                     # hr without --negatives
    with pytest.raises(SystemExit):
        evaluate.main(['-d', data, '-m', model, '-sl', 'im', '-M', 'mrr', '--negatives', '0'])
