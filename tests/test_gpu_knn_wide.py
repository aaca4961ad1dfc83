"""K28 / K29 on the GPU where their loops repeat (csrc/knn.hip) against tests/_knn_oracle.py, bit for bit as tests/test_gpu_knn.py.

The cases and the conditions each exists for are built and asserted without a GPU in tests/test_knn_cpu.py:
  1  wide_build_case   700 x 600: user lists above 64 and 128, items above 256 and 512 likers, the radix select on every row, ties at the
                       cut that column byte 1 decides, N = 512 (a sort of 1,024 pairs), rows split to the 64-part cap
  2  band_case         66,000 items: column byte 2, two natural slabs, dynamic LDS above 64 KB
  3  serve_case        K29 from the table of case 1: histories up to 159 items, N up to 512, 300 and 256 likes on a line, 600 columns
  4  hand_case         K29 on hand-made tables over 66,000 columns: the select, the slab merge and the ranks decided by construction
     chain_case        K29's fp32 chain across the look-ahead of sixteen list pieces, at N = 100 and N = 130
Nothing here has a tolerance."""
import numpy as np
import pytest
import torch

import _knn_oracle as O
from test_knn_cpu import (WIDE_ITEMS, band_case, band_oracle, chain_case, hand_case, hand_oracle, serve_case, serve_oracle,
                          wide_build_case, wide_build_oracle)

pytestmark = pytest.mark.gpu

NO_HEAVY = 1 << 40


def _dev(a):
    return torch.from_numpy(np.array(a, order='C')).cuda()


def _bits(a):
    return np.ascontiguousarray(a).view(np.int32)


def _same_table(got, want, what=''):
    np.testing.assert_array_equal(got[0], want[0], err_msg='ids ' + what)
    np.testing.assert_array_equal(_bits(got[1]), _bits(want[1]), err_msg='weights ' + what)


def _builder(c, similarity, workspace=None):
    """the operands of a case on the device, once -> build(N, **kw) -> (ids, w) as numpy"""
    import tkr_hip
    norm = O.norms(np.diff(c['ip']), similarity)
    args = tuple(_dev(c[name]) for name in ('up', 'uc', 'ip', 'ir')) + (_dev(norm),)

    def build(N, **kw):
        ids, w = tkr_hip.knn_build(*args, N, workspace=workspace, **kw)
        return ids.cpu().numpy(), w.cpu().numpy()
    return build


# ---- K28 ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('N', [16, 100, 512])
@pytest.mark.parametrize('similarity', ['cooc', 'cosine'])
def test_build_700_by_600(similarity, N):
    """case 1.  heavy_from = 700 splits every row (the heaviest to the cap of 64 parts); 256 and 257 columns a slab: three slabs"""
    build = _builder(wide_build_case(), similarity)
    want = wide_build_oracle(similarity, N)[:2]
    _same_table(build(N, heavy_from=NO_HEAVY), want, 'unsplit')
    _same_table(build(N, heavy_from=700), want, 'split')
    _same_table(build(N, heavy_from=NO_HEAVY, slab_cols=256), want, 'in slabs')
    _same_table(build(N, heavy_from=700, slab_cols=257), want, 'split and in slabs')


@pytest.fixture(scope='module')
def wide_workspace():
    import tkr_hip
    need = tkr_hip.knn_build_workspace_bytes(WIDE_ITEMS)
    assert 500 << 20 < need < 600 << 20
    ws = torch.empty(need // 8 + 1, dtype=torch.int64, device='cuda')      # once for every call of the case
    yield ws
    del ws
    torch.cuda.empty_cache()


@pytest.mark.parametrize('similarity', ['cooc', 'cosine'])
def test_build_66000_items(similarity, wide_workspace):
    """case 2, N = 100: the natural slabs (36,864 + 29,136 columns, 147 KB of LDS), the liked rows split, slabs of 20,000"""
    import tkr_hip
    assert tkr_hip.KNN_MAX_SLAB == 36864 < WIDE_ITEMS
    c = band_case()
    build = _builder(c, similarity, wide_workspace)
    want = band_oracle(similarity)
    _same_table(build(100, heavy_from=NO_HEAVY), want, 'natural slabs')
    _same_table(build(100, heavy_from=c['heavy_from']), want, 'split')
    _same_table(build(100, heavy_from=NO_HEAVY, slab_cols=20000), want, 'slabs of 20,000')


# ---- K29 ----------------------------------------------------------------------------------------------------------------------------------
def _server(hist, ids, w, n_cols, col_of_item, rated, likes):
    """the operands of a K29 case on the device, once -> score(K, lines=None, **kw) -> (ids, scores, ranks) as numpy"""
    import tkr_hip
    table = (_dev(ids), _dev(w))
    col_of_item = None if col_of_item is None else _dev(col_of_item)

    def score(K, lines=None, **kw):
        lo, hi = lines or (0, len(hist[0]) - 1)
        cut = lambda ptr, cols: (_dev(ptr[lo:hi + 1] - ptr[lo]), _dev(cols[ptr[lo]:ptr[hi]]))
        mask, pitch = tkr_hip.build_rated_mask(*cut(*rated), hi - lo, n_cols)
        lp, lc = cut(*likes)
        out = tkr_hip.knn_score(*cut(*hist), *table, K, col_of_item=col_of_item, n_cols=n_cols, mask=mask, mask_pitch=pitch, want_scores=True,
                                like_ptr=lp, like_cols=lc, **kw)
        return tuple(x.cpu().numpy() for x in out)
    return score


def _same_lists(got, top, top_s, ranks, K, what=''):
    """top / top_s: the oracle's lists at K or more columns; a list of K is their prefix"""
    np.testing.assert_array_equal(got[0], top[:, :K], err_msg='ids ' + what)
    np.testing.assert_array_equal(_bits(got[1]), _bits(top_s[:, :K]), err_msg='scores ' + what)
    np.testing.assert_array_equal(got[2], ranks, err_msg='ranks ' + what)


def _serve(columns, N):
    c = serve_case(columns)
    ids, w, s, ranks = serve_oracle(columns, N)
    return c, s, ranks, _server(c['hist'], ids, w, c['n_cols'], c['col_of_item'], c['rated'], c['likes'])


@pytest.mark.parametrize('N', [64, 65, 100, 130, 512])
@pytest.mark.parametrize('columns', ['identity', 'subset'])
def test_score_from_the_table_of_700_by_600(columns, N):
    """case 3: 1, 2, 2, 3 and 8 pieces per history item; K = 40 is above what one launch lists; slabs of 256 and 100 columns"""
    c, s, ranks, score = _serve(columns, N)
    for K in (5, 32, 40):
        top, top_s = O.topk(s, c['masked'], K)
        for slab_cols in (None, 256, 100):
            _same_lists(score(K, slab_cols=slab_cols), top, top_s, ranks, K, 'K = %d, slab_cols = %r' % (K, slab_cols))


def test_score_a_block_of_wide_lines_alone_is_the_block_inside_the_call():
    c, s, ranks, score = _serve('subset', 130)
    whole, block = score(32), score(32, lines=(30, 70))
    lp = c['likes'][0]
    assert block[0].tobytes() == whole[0][30:70].tobytes() and block[1].tobytes() == whole[1][30:70].tobytes()
    assert block[2].tobytes() == whole[2][lp[30]:lp[70]].tobytes()


def _hand(c):
    return _server(c['hist'], c['ids'], c['w'], WIDE_ITEMS, None, c['rated'], c['likes'])


def test_score_hand_made_table_over_66000_columns():
    """case 4, N = 512: lists of 32 and the ranks of every line with the natural slabs and with slabs of 30,000; the two lines with an
    empty history at K = 1 and at K = 70"""
    c = hand_case()
    s, masked, ranks, top, top_s = hand_oracle('hand')
    score = _hand(c)
    _same_lists(score(32), top, top_s, ranks, 32, 'natural slabs')
    _same_lists(score(32, slab_cols=30000), top, top_s, ranks, 32, 'slabs of 30,000')
    two = ranks[:c['likes'][0][2]]
    for K in (1, 70):
        _same_lists(score(K, lines=(0, 2)), top[:2], top_s[:2], two, K, 'K = %d' % K)


@pytest.mark.parametrize('N', [100, 130])
def test_score_chains_across_the_look_ahead(N):
    """case 4, the chains: every column's sum is the one of the history order, whichever batch of sixteen pieces a term falls in"""
    c = chain_case(N)
    s, masked, ranks, top, top_s = hand_oracle('chain', N)
    score = _hand(c)
    _same_lists(score(32), top, top_s, ranks, 32, 'natural slabs')
    _same_lists(score(5, slab_cols=30000), top, top_s, ranks, 5, 'slabs of 30,000')
