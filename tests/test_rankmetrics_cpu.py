"""rankmetrics.py against the NumPy oracle of tests/_rank_oracle.py on the committed goldens; no GPU."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _rank_oracle as O
from oracle import ref_np as R

import rankmetrics

CASES = [('g4', 'im'), ('g4', 'om'), ('g5', 'im'), ('g5', 'om'), ('g6', 'all'), ('g7', 'sm')]
STEP_TOTAL = [(5, 30), (7, 64), (50, 300), (3, 7)]


def _paths(golden_dir, g):
    return os.path.join(golden_dir, g, 'data'), os.path.join(golden_dir, g, 'model')


@pytest.fixture(scope='module')
def loaded(golden_dir):
    out = {}
    for g, sc in CASES:
        data, model = _paths(golden_dir, g)
        scores, lines = O.load_lines(data, model, 0, sc)
        out[g, sc] = (scores, lines, O.csr_ranks(scores, lines))
    return out


def _sums(loaded, case, step, total):
    scores, lines, (ranks, like_ptr, rated_ptr) = loaded[case]
    return rankmetrics.rank_sums(ranks, like_ptr, rated_ptr, scores.shape[1], step, total)


@pytest.mark.parametrize('step,total', STEP_TOTAL)
@pytest.mark.parametrize('case', CASES)
def test_acc_from_ranks_equals_reference_cli(golden_dir, loaded, case, step, total):
    data, model = _paths(golden_dir, case[0])
    want = R.evaluate_cli(data, model, 0, step, total, scenarios=(case[1],), canonical=True)
    acc = rankmetrics.finish(_sums(loaded, case, step, total), ('acc',))['acc']
    assert [case[1] + ''.join(',%.6f' % v for v in acc)] == want


@pytest.mark.parametrize('case', CASES)
def test_golden_ranks_do_not_depend_on_the_summation_order(golden_dir, loaded, case):
    """BLAS dot, the kernels' fma chain and float64 scores rank every like of the goldens alike, and no line has an exact tie"""
    data, model = _paths(golden_dir, case[0])
    ranks = loaded[case][2][0]
    assert np.any(ranks >= 0)
    for scoring in ('chain', 'f64'):
        scores, lines = O.load_lines(data, model, 0, case[1], scoring)
        np.testing.assert_array_equal(O.csr_ranks(scores, lines)[0], ranks)
    scores, lines = loaded[case][:2]
    for row, _, _ in lines:
        assert len(np.unique(scores[row])) == scores.shape[1]


@pytest.mark.parametrize('step,total', STEP_TOTAL)
@pytest.mark.parametrize('case', CASES)
def test_metrics_equal_direct_loops(loaded, case, step, total):
    scores, lines, _ = loaded[case]
    got, want = _sums(loaded, case, step, total), O.direct_sums(scores, lines, step, total)
    for m in rankmetrics.METRICS:
        assert got[m][1] == want[m][1], m
    np.testing.assert_array_equal(got['acc'][0], want['acc'][0])
    # AUC: integer ratios, one division per line and one sum -- 1e-12
    if want['auc'][1]:
        assert abs(got['auc'][0] / got['auc'][1] - want['auc'][0] / want['auc'][1]) <= 1e-12
    for m in ('mrr', 'ndcg', 'map'):
        np.testing.assert_allclose(got[m][0], want[m][0], rtol=1e-12, atol=1e-12)


def test_g7_has_rated_likes_and_they_stay_in_the_denominator(loaded):
    scores, lines, (ranks, like_ptr, rated_ptr) = loaded['g7', 'sm']
    assert np.any(ranks < 0)
    sums = rankmetrics.rank_sums(ranks, like_ptr, rated_ptr, scores.shape[1], 5, 30)
    assert sums['acc'][1] == len(ranks) and sums['mrr'][1] <= len(lines)


@pytest.mark.parametrize('case', CASES)
def test_shard_sums_add_up(loaded, case):
    scores, lines, (ranks, like_ptr, rated_ptr) = loaded[case]
    n = len(lines)
    cut = n // 2
    whole = rankmetrics.rank_sums(ranks, like_ptr, rated_ptr, scores.shape[1], 3, 10)
    a = rankmetrics.rank_sums(ranks[:like_ptr[cut]], like_ptr[:cut + 1], rated_ptr[:cut + 1], scores.shape[1], 3, 10)
    b = rankmetrics.rank_sums(ranks[like_ptr[cut]:], like_ptr[cut:] - like_ptr[cut], rated_ptr[cut:] - rated_ptr[cut], scores.shape[1], 3, 10)
    both = rankmetrics.add_sums(a, b)
    back = rankmetrics.from_vector(rankmetrics.to_vector(a) + rankmetrics.to_vector(b), 10 // 3)
    for got in (both, back):
        for m in rankmetrics.METRICS:
            assert got[m][1] == whole[m][1], m
            np.testing.assert_allclose(got[m][0], whole[m][0], rtol=1e-13, atol=0)
        np.testing.assert_array_equal(got['acc'][0], whole['acc'][0])
    assert rankmetrics.finish(back).keys() == set(rankmetrics.METRICS)


def test_hand_worked_line():
    """one line, 10 columns, 2 rated, likes at filtered ranks 0 and 3 and one rated like: every metric by hand"""
    sums = rankmetrics.rank_sums([0, -1, 3], [0, 3], [0, 2], 10, 2, 4)
    out = rankmetrics.finish(sums)
    assert out['acc'] == [1 / 3, 2 / 3]
    assert out['auc'] == [1 - (0 + 2) / (2 * 6)]                      # C = 8, P = 2, N = 6; two non-likes in front of the second like
    assert out['mrr'] == [1.0]
    ideal = 1 + 1 / np.log2(3)
    np.testing.assert_allclose(out['ndcg'], [1 / ideal, (1 + 1 / np.log2(5)) / ideal], rtol=1e-15)
    np.testing.assert_allclose(out['map'], [1 / 2, (1 + 2 / 4) / 2], rtol=1e-15)
