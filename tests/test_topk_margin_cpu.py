"""The inputs of tests/test_gpu_topk_margin.py do what they are built for: conditions on the INPUTS, checked with the CPU restatement of
K4's fp16 pass (tests/_margin_oracle.py) -- never on a kernel.  Runs without a GPU and prints the share of 2 * margin every case
reaches (pytest -s)."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _margin_oracle as M
from oracle import ref_np as R

ADVERSARIAL = M.CASES + M.SPLIT_CASES + M.FIRST_FORM_CASES + [M.WIDE_ID_CASE]


def _unique(cases):
    out, ids = [], set()
    for p in cases:
        if M.case_id(p) + str(p.get('victim_tile')) + str(p.get('n_rows')) not in ids:
            ids.add(M.case_id(p) + str(p.get('victim_tile')) + str(p.get('n_rows')))
            out.append(p)
    return out


@pytest.mark.parametrize('p', _unique(ADVERSARIAL), ids=M.case_id)
def test_adversarial_case_sits_near_the_margin(p):
    """The victim is in the exact top K (no exact tie at the cut) and at or behind position K by approximate score, at least
    share_floor (0.75; 0.7 for k = 8) of 2 * margin below the K-th best approximate score; no item's fp16 error exceeds the margin;
    the K-th best approximate score lies close above the lower edge of its 16-bit key (share - align > 0.6: an exact comparison
    with that edge - 1 * margin, as the first form and the second form's filter make, drops the victim); and a key edge lies between
    the victim and that edge - 1 * margin, but none between it and the edge - 2 * margin (key_drop_1m, key_keep_2m: the second form
    drops a list entry by its key alone, so a 1 * margin filter can lose the victim there only if this holds).  Necessary, not
    sufficient: on a build with m2 = margin the first form failed its cases and the second form passed all of them (it failed them
    all at 0.5 * margin) -- DESIGN.md section 4, K4."""
    case = M.adversarial_case(**p)
    got = M.case_conditions(case)
    print('%-40s share of 2*margin %.3f  largest |approx - exact| / margin %.3f  K-th above its key edge %.3f  key width / margin %.2f  '
          'approx rank %d' % (M.case_id(p), got['share'], got['used'], got['align'], got['key_width'], got['victim_approx_rank']))
    K = p['K']
    assert got['victim_exact_rank'] < K and not got['cut_tie']
    assert got['victim_approx_rank'] >= K
    assert got['share'] >= M.share_floor(p['k'])
    assert got['used'] <= 1.0
    assert got['share'] - got['align'] > 0.6
    assert got['key_drop_1m'] and got['key_keep_2m']
    # the special columns are spread over both half-lane groups of their tiles, and enough decoys stay unrated
    cols = np.array(case['decoys'] + [case['victim']])
    assert abs(int((cols % 8 < 4).sum()) - int((cols % 8 >= 4).sum())) <= 2
    assert all(len(set(case['decoys']) - set(r)) >= K for r in case['rated'])
    assert len({float(np.abs(u).max()) for u in case['U']}) >= (1 if p['bias'] else min(60, len(case['U']) - 1))      # every user its own scale


def test_exponents_cover_eighty_binades():
    case = M.adversarial_case(**M.CASES[0])
    e = np.log2(np.abs(case['U']).max(axis=1))
    assert e.min() <= -39 and e.max() >= 39


@pytest.mark.parametrize('n_rows,n_cols,k,bias,wide', M.GENERIC_SHAPES)
def test_documented_margin_covers_the_fp16_pass_on_generic_inputs(n_rows, n_cols, k, bias, wide):
    """|approx - exact| <= margin on the inputs of test_refine_is_the_fp32_arithmetic (a sample of the rows of the large shapes), and
    how little of it random factors use: what the adversarial cases are for."""
    U, V, b = M.generic_inputs(n_rows, n_cols, k, bias, wide)
    rows = np.arange(0, n_rows, max(1, n_rows * n_cols // 1_000_000))
    ap, scale = M.approx_scores(U[rows], V, b)
    chain = R.mfma_chain_scores(U[rows], V, b).astype(np.float64)
    m = M.margin(U, V, b, k)[rows]
    used = np.abs(ap - chain * scale[:, None]) / m[:, None]
    print('%dx%d k=%d%s: largest |approx - exact| / margin %.4f' % (n_rows, n_cols, k, ' wide' if wide else '', used.max()))
    assert used.max() <= 1.0


def test_restatement_is_the_documented_formula():
    """margin() and approx_scores() on a case small enough to do by hand: |u| = 5, max|v_i| = 2, max|bias| = 8; 4 and 2 scale to 2^13"""
    U = np.array([[3.0, 4.0]], np.float32)
    V = np.array([[0.0, 2.0], [1.0, 0.0]], np.float32)
    b = np.array([0.5, -8.0], np.float32)
    scale = 2.0 ** 11 * 2.0 ** 12
    assert M.margin(U, V, b, 2)[0] == scale * (1.05 * 2.0 ** -10 * 10.0 + 2.0 ** -18 * (10.0 + 8.0)) + 2.01 * 16
    ap, sc = M.approx_scores(U, V, b)
    assert sc[0] == scale and ap[0].tolist() == [(8.0 + 0.5) * scale, (3.0 - 8.0) * scale]
    assert M.key16_edge(1.0 + 2.0 ** -8) == 1.0 and M.key16_width(1.0) == 2.0 ** -7
