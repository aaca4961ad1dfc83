"""K4's bound-and-refine pass at its margin, on the GPU (the inputs: tests/_margin_oracle.py; what they promise is checked on the CPU
by tests/test_topk_margin_cpu.py).

Every test asserts that ids and score bits under 'refine' are those under 'fp32', that both are the chain oracle's ranking, and --
through tkr_hip.topk_last_report() -- which form of the pass ran and which user blocks it gave to the fp32 kernel: a flagged block is
ranked by the fp32 kernel, so without the report "refine == fp32" may compare that kernel with itself.

K = 30 ran unflagged at every width (k = 8, 15, 16, 32, 50, 64, 100, 119, 128), in both forms; no case had to fall back to a smaller K.

What these cases were seen to catch (a scratch build with m2 = margin instead of 2 * margin, once per form):
the first-form tests fail, the victim missing.  The second-form tests do NOT: all pass at m2 = margin, and all 44 of them fail at
m2 = 0.5 * margin.  They hold the second form to the fp32 kernel at inputs that use 0.88 of the margin, unflagged, and its filter
above half a margin -- not the factor 2."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _margin_oracle as M

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def hip():
    import tkr_hip
    assert torch.cuda.is_available()
    tkr_hip.lib()
    return tkr_hip


# ---- the second form (csrc/topk_refine.hip), the default -------------------------------------------------------------------------------
@pytest.mark.parametrize('p', M.CASES, ids=M.case_id)
def test_second_form_keeps_the_victim(hip, p):
    """k = 8 .. 128 (KS = 1, 2, 4, 8, both staging paths, odd k), K = 1, 8, 30, with and without bias and rated decoys"""
    M.run_case_on_gpu(hip, p, form=2)


def _first_case(**want):
    return next(p for p in M.CASES if all(bool(p[f]) == v if isinstance(v, bool) else p[f] == v for f, v in want.items()))


@pytest.mark.parametrize('p', [_first_case(k=8, bias=False, rated_decoys=False), _first_case(k=50, bias=True, rated_decoys=False),
                               _first_case(k=128, bias=True, rated_decoys=True), _first_case(k=119, bias=False, rated_decoys=True)],
                         ids=M.case_id)
def test_second_form_through_user_idx(hip, p):
    """rows gathered through user_idx from a larger table: one case without bias, one with, and one each with rated decoys"""
    M.run_case_on_gpu(hip, p, form=2, via_user_idx=True)


@pytest.mark.parametrize('p', M.SPLIT_CASES, ids=lambda p: M.case_id(p) + '-v%d' % p['victim_tile'])
def test_bounds_shared_across_item_ranges(hip, p):
    """One user block whose catalogue the plan cuts into item ranges: the decoys' range knows a bound of the K-th best score, the
    victim lives in another one.  What the ranges tell each other (share_bound: + margin on the way out, - margin on the way in) and
    the largest threshold the finish kernel takes over all pieces must leave the victim in."""
    report = M.run_case_on_gpu(hip, p, form=2, same_range=True)
    assert report['blocks'] == 1 and report['pieces'] > 1


# ---- the first form (csrc/topk.hip score_topk_bf16_kernel) -----------------------------------------------------------------------------
@pytest.mark.parametrize('image', [True, False], ids=['image', 'no-image'])
def test_first_form_in_a_fresh_process(image):
    """TKR_TOPK_V2=0 (and TKR_TOPK_IMAGE=0) are read once per process: tests/_margin_child.py runs the cases at k = 16 and 128 and one
    catalogue of 66,000 columns (32-bit ids) and asserts the report's form == 1, image field and id width"""
    env = dict(os.environ, TKR_TOPK_V2='0')
    env.pop('TKR_TOPK_IMAGE', None)
    if not image:
        env['TKR_TOPK_IMAGE'] = '0'
    child = os.path.join(os.path.dirname(os.path.abspath(__file__)), '_margin_child.py')
    done = subprocess.run([sys.executable, child, '1' if image else '0'], env=env, capture_output=True, text=True, timeout=180)
    assert done.returncode == 0 and 'first form ok' in done.stdout, done.stdout[-3000:] + done.stderr[-3000:]


# ---- the edges of `sane` (csrc/topk_parts.h refine_prologue) -----------------------------------------------------------------------------
def _row_with_exponent(rng, k, e):
    """a random row whose largest |element| is 1.5 * 2^e"""
    u = rng.standard_normal(k)
    return (u / np.abs(u).max() * 1.5 * 2.0 ** e).astype(np.float32)


def _run_plain(hip, U, V, b, K=30):
    rated = [[] for _ in range(len(U))]
    refine, fp32, report = M.topk_both_modes(hip, U, V, b, rated, K)
    M.assert_same_as_fp32_and_oracle(refine, fp32, U, V, b, rated, K)
    return report


@pytest.mark.parametrize('e,sane', [(-48, False), (-47, True), (59, True), (60, False)])
@pytest.mark.parametrize('k', [16, 50])
def test_row_exponent_at_the_edge_of_sane(hip, k, e, sane):
    """pow2_scale_exact: a row whose largest element has exponent in [-47, 60) keeps its block on the fast path, one outside flags it.
    The row sits in block 1 (rows 128, 129); block 0, which holds rows at BOTH inner edges and an all-zero row, is never flagged."""
    rng = np.random.Generator(np.random.PCG64(100 + k + e))
    U = (rng.standard_normal((130, k)) * 0.01).astype(np.float32)
    V = (rng.standard_normal((320, k)) * 0.01).astype(np.float32)
    b = (rng.standard_normal(320) * 0.002).astype(np.float32)
    U[5], U[70], U[100] = _row_with_exponent(rng, k, -47), _row_with_exponent(rng, k, 59), 0.0
    U[129] = _row_with_exponent(rng, k, e)
    report = _run_plain(hip, U, V, b)
    print(report)
    assert report['form'] == 2 and report['blocks'] == 2
    assert report['flags'] == [0, 0 if sane else 1] and report['flagged'] == (0 if sane else 1)


@pytest.mark.parametrize('q,bmax,sane', [(0.99e38, 0.0, True), (1.01e38, 0.0, False), (0.5e38, 0.48e38, True), (0.5e38, 0.52e38, False)])
def test_reach_near_the_range_of_fp32(hip, q, bmax, sane):
    """|u| * max|v_i| + max|bias| just below and just above 1e38, by the first term alone and by the sum with a bias as large as it
    (k = 128, every element of the table near 2^59.5 -- the only way there inside the exponent range; the kernel takes |u| 0.1 % high,
    the cases stay 1 % to 2 % off the edge): the row's block (1) is flagged on the far side only, block 0 never."""
    rng = np.random.Generator(np.random.PCG64(7))
    k = 128
    U = rng.standard_normal((130, k)).astype(np.float32)
    V = (rng.choice([-1.0, 1.0], (320, k)) * rng.uniform(0.92, 1.0, (320, k)) * 0.999 * 2.0 ** 60).astype(np.float32)
    vmax = np.sqrt((V.astype(np.float64) ** 2).sum(axis=1)).max()
    u = rng.choice([-1.0, 1.0], k) * rng.uniform(0.92, 1.0, k)
    U[128] = (u * (q / vmax / np.sqrt((u * u).sum()))).astype(np.float32)
    reach = np.sqrt((U[128].astype(np.float64) ** 2).sum()) * vmax
    assert abs(reach / q - 1) < 1e-6 and 2.0 ** 58 <= np.abs(U[128]).max() < 2.0 ** 60 and np.abs(V).max() < 2.0 ** 60
    b = None
    if bmax:
        b = rng.uniform(-bmax, bmax, 320).astype(np.float32)
        b[200] = bmax
    report = _run_plain(hip, U, V, b)
    print(report)
    assert report['form'] == 2 and report['flags'] == [0, 0 if sane else 1]


@pytest.mark.parametrize('bmax,sane', [(70.0, True), (80.0, False)])
def test_bias_in_scaled_units_near_the_range_of_fp32(hip, bmax, sane):
    """max|bias| * su * sv just below and just above 1e38: a row and a table at the small end of the exponent range (largest elements
    1.5 * 2^-47: su = sv = 2^60, and 1e38 / 2^120 = 75.2).  Only that row's scale is so large: block 1 is flagged on the far side,
    block 0 (ordinary rows, the same biases) never."""
    rng = np.random.Generator(np.random.PCG64(11))
    k = 16
    U = (rng.standard_normal((130, k)) * 0.01).astype(np.float32)
    V = rng.standard_normal((320, k))
    V = (V / np.abs(V).max() * 1.5 * 2.0 ** -47).astype(np.float32)
    U[129] = _row_with_exponent(rng, k, -47)
    b = rng.uniform(-bmax, bmax, 320).astype(np.float32)
    b[200] = bmax
    report = _run_plain(hip, U, V, b)
    print(report)
    assert report['form'] == 2 and report['flags'] == [0, 0 if sane else 1]


def test_bias_dominates(hip):
    """Every bias equal to 2^20 times the score scale, 60 columns: every score is within a few ulp of the bias, the margin (its
    2^-18 * max|bias| term) covers all of them, the lists hold the whole catalogue -- the canonical tie order, and no block flagged."""
    rng = np.random.Generator(np.random.PCG64(8))
    U = (rng.standard_normal((130, 16)) * 0.01).astype(np.float32)
    V = (rng.standard_normal((60, 16)) * 0.01).astype(np.float32)
    b = np.full(60, 2.0 ** 20 * 2.0 ** -11, dtype=np.float32)                # scores ~ 4e-4 ~ 2^-11
    report = _run_plain(hip, U, V, b)
    print(report)
    assert report['form'] == 2 and report['flagged'] == 0


def test_overflowing_lists_are_reported(hip):
    """The construction of test_gpu_topk.py test_refine_overflowing_lists_fall_back at a small shape: far more exact and near copies of
    every user's best item than a list has slots.  The blocks MUST be flagged -- this is what makes 'flagged == 0' elsewhere mean
    something -- and the lists are still the oracle's."""
    rng = np.random.Generator(np.random.PCG64(77))
    n_rows, n_cols, k, K = 130, 2048, 64, 30
    U = (np.abs(rng.standard_normal((n_rows, k))) * 0.01 + 0.001).astype(np.float32)
    V = (rng.standard_normal((n_cols, k)) * 0.002).astype(np.float32)
    best = np.full(k, 0.03, dtype=np.float32)
    dup = rng.choice(n_cols, 1400, replace=False)
    V[dup[:1000]] = best
    V[dup[1000:]] = best * (1.0 - rng.uniform(0, 2e-4, (400, 1)).astype(np.float32))
    rated = [rng.choice(n_cols, 20, replace=False).tolist() for _ in range(n_rows)]
    refine, fp32, report = M.topk_both_modes(hip, U, V, None, rated, K)
    print(report)
    M.assert_same_as_fp32_and_oracle(refine, fp32, U, V, None, rated, K)
    assert report['form'] == 2 and report['flagged'] == report['blocks'] == 2 and report['flags'] == [1, 1]
    assert all(set(row.tolist()) <= set(dup[:1000].tolist()) for row in refine[0])
