"""K19 (tkr_nearest_anchors) without a GPU: the oracle on a hand-worked example, the ABI and its argument checks, the arithmetic of
unexpectedness on CPU tensors, the text of the explain lines, and what the two command lines refuse."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _explain_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

V_, I32, I64 = C.c_void_p, C.c_int32, C.c_int64
ANCHOR_ARGTYPES = [V_, I32, I32, V_, I32, I32, V_, V_, I64, I32, V_, V_, V_, V_]
NINF = -np.inf


def test_oracle_on_a_hand_worked_example():
    """five items in two dimensions: 0 and 1 are (1, 0), 2 is (0, 1), 3 is (1/2, 1/2), 4 is (1/2, 0).  sim: s01 = 1, s02 = s12 = 0,
    s03 = s13 = s04 = s14 = s23 = 1/2, s24 = 0, s34 = 1/4.
      row 0: list 0, 3, -1, 2 (the 2 behind the -1 is not looked at), anchors 1, 0, 3, 1, 4 (item 1 twice), e = 3.
        entry 0 (item 0): position 1 is the item itself; positions 0 and 3 (item 1, sim 1) tie, the lower one first; then 2 and 4 (1/2)
                          tie and position 2 wins the last place: 0, 3, 2.  The best four are 1, 1, 1/2, 1/2: gap 0, ambiguous.
        entry 1 (item 3): position 2 is itself; 0, 1, 3 all 1/2, then 4 (1/4): 0, 1, 3; gaps 0, 0, 1/4.
      row 1: list 2, 4, 0, 1, anchors 2, 4: fewer than e.  Item 2 is left with position 1 (sim 0), item 4 with position 0; items 0 and 1
             see position 1 (1/2) before position 0 (0): gap 1/2.
      row 2: no anchors at all."""
    S = np.array([[1, 0], [1, 0], [0, 1], [0.5, 0.5], [0.5, 0]], dtype=np.float32)
    ids = np.array([[0, 3, -1, 2], [2, 4, 0, 1], [0, 1, 2, 3]], dtype=np.int32)
    ptr = np.array([0, 5, 7, 7], dtype=np.int64)
    cols = np.array([1, 0, 3, 1, 4, 2, 4], dtype=np.int32)
    pos, sim, amb = O.nearest(S, ids, ptr, cols, 3, 5)
    assert pos[0].tolist() == [[0, 3, 2], [0, 1, 3], [-1, -1, -1], [-1, -1, -1]]
    assert sim[0].tolist() == [[1, 1, .5], [.5, .5, .5], [NINF] * 3, [NINF] * 3]
    assert pos[1].tolist() == [[1, -1, -1], [0, -1, -1], [1, 0, -1], [1, 0, -1]]
    assert sim[1].tolist() == [[0, NINF, NINF], [0, NINF, NINF], [.5, 0, NINF], [.5, 0, NINF]]
    assert np.all(pos[2] == -1) and np.all(sim[2] == NINF)
    assert amb.tolist() == [[True, True, False, False], [False] * 4, [False] * 4]
    assert sim.dtype == np.float32 and pos.dtype == np.int32
    full = O.R.mfma_chain_scores(S, S)
    for a, b in zip(O.nearest(S, ids, ptr, cols, 3, 5, full=full), (pos, sim, amb)):
        np.testing.assert_array_equal(a, b)
    assert O.nearest(S, ids, ptr, cols, 1, 5)[0][:2, :, 0].tolist() == [[0, 0, -1, -1], [1, 0, 1, 1]]
    assert O.columns(pos, ptr, cols)[0].tolist() == [[1, 1, 3], [1, 0, 1], [-1] * 3, [-1] * 3]
    assert O.status_word(ids, ptr, cols, 5) == -1
    # untrusted input: an id >= n_items ends its row (kind 0), an anchor outside the table is skipped (kind 1) and keeps its position,
    # a descending anchor_ptr gives padding (kind 3); the smallest word is reported
    bad_ids = ids.copy()
    bad_ids[1, 2] = 5
    assert O.status_word(bad_ids, ptr, cols, 5) == 4 * 1 + 0
    assert O.nearest(S, bad_ids, ptr, cols, 3, 5)[0][1].tolist() == [[1, -1, -1], [0, -1, -1], [-1] * 3, [-1] * 3]
    bad_cols = cols.copy()
    bad_cols[0], bad_cols[5] = 7, -2
    assert O.status_word(ids, ptr, bad_cols, 5) == 4 * 0 + 1 and O.status_word(bad_ids, ptr, bad_cols, 5) == 1
    pos2, _, _ = O.nearest(S, ids, ptr, bad_cols, 3, 5)
    assert pos2[0].tolist()[:2] == [[3, 2, 4], [1, 3, 4]] and pos2[1].tolist() == [[1, -1, -1], [-1] * 3, [1, -1, -1], [1, -1, -1]]
    bad_ptr = np.array([0, 5, 4, 7], dtype=np.int64)
    assert O.status_word(ids, bad_ptr, cols, 5) == 4 * 1 + 3
    pos3, _, _ = O.nearest(S, ids, bad_ptr, cols, 3, 5)
    assert np.all(pos3[1] == -1) and pos3[0].tolist() == pos[0].tolist() and pos3[2].tolist()[0] == [0, 2, 1]            # row 2 now holds 4, 2, 4
    assert O.status_word(ids, np.array([1, 5, 7, 7]), cols, 5) == 3 and O.status_word(ids, np.array([0, 5, 7, 8]), cols, 5) == 4 * 2 + 3


def test_header_binding_and_library_agree_and_check_their_arguments():
    import tkr_hip
    header = open(os.path.join(ROOT, 'include', 'tkr.h')).read()
    declared = re.findall(r'^int(?:32_t|64_t)? (tkr_\w+)\(', header, flags=re.M)
    lib = C.CDLL(tkr_hip.LIB_PATH)
    assert 'tkr_nearest_anchors' in declared and 'tkr_nearest_anchors' in tkr_hip.EXPORTS and hasattr(lib, 'tkr_nearest_anchors')
    assert re.search(r'#define TKR_ANCHOR_MAX_E %d\b' % tkr_hip.ANCHOR_MAX_E, header) and tkr_hip.ANCHOR_MAX_E == 8
    assert re.search(r'#define TKR_ANCHOR_MAX_T %d\b' % tkr_hip.ANCHOR_MAX_T, header) and tkr_hip.ANCHOR_MAX_T == tkr_hip.MMR_MAX_POOL
    assert callable(tkr_hip.nearest_anchors)
    p = 4096                                                          # never dereferenced: every call below fails its checks
    fn = lib.tkr_nearest_anchors
    fn.restype, fn.argtypes = C.c_int, ANCHOR_ARGTYPES
    good = dict(S=p, n_items=600, k=8, ids=p, n_rows=3, t=30, ptr=p, cols=p, n_anchors=10, e=3, pos=p, sim=p, status=p, stream=None)
    assert len(good) == len(ANCHOR_ARGTYPES)
    for change in (dict(S=None), dict(ids=None), dict(ptr=None), dict(cols=None), dict(pos=None), dict(sim=None), dict(status=None),
                   dict(n_items=0), dict(k=0), dict(n_rows=0), dict(t=0), dict(e=0), dict(n_items=-1), dict(k=-5), dict(n_rows=-1), dict(t=-1),
                   dict(e=-1), dict(n_anchors=-1), dict(n_anchors=-1, cols=None)):
        assert fn(*dict(good, **change).values()) == -1, change
    assert fn(*dict(good, t=1025).values()) == -2                     # TKR_E_UNSUPPORTED
    assert fn(*dict(good, e=9).values()) == -2
    assert fn(*dict(good, t=1025, e=9).values()) == -2
    assert fn(*dict(good, t=1025, e=0).values()) == -1                # what is invalid is invalid at any size
    assert fn(*dict(good, e=9, S=None).values()) == -1


def test_wrappers_refuse_on_the_host():
    """tensor properties are looked at before the library is asked: CPU tensors never reach a kernel"""
    import explain
    import tkr_hip
    S, ids = torch.zeros((5, 4)), torch.zeros((2, 3), dtype=torch.int32)
    ptr, cols = torch.zeros(3, dtype=torch.int64), torch.zeros(0, dtype=torch.int32)
    with pytest.raises(tkr_hip.TkrError, match='GPU'):
        tkr_hip.nearest_anchors(S, ids, ptr, cols, 3)
    with pytest.raises(tkr_hip.TkrError, match='int32'):
        tkr_hip.nearest_anchors(S, ids.long(), ptr, cols, 3)
    with pytest.raises(tkr_hip.TkrError, match='GPU'):
        explain.explain(S, ids, ptr, cols, 3)
    assert explain.METRICS == ('unexp',)


def test_unexpectedness_arithmetic_against_a_loop():
    import explain
    rng = np.random.Generator(np.random.PCG64(19))
    n, t = 29, 12
    ids = rng.integers(0, 50, (n, t)).astype(np.int32)
    sims0 = (rng.random((n, t)) * 2 - 1).astype(np.float32)
    for r, cut in ((0, 0), (1, 1), (2, 5), (3, 11)):                  # an empty list, one entry, ...
        ids[r, cut:] = -1
    ids[4, 3] = -1                                                    # a -1 in the middle: everything behind it is ignored
    sims0[4, 7] = -1e9                                                # (behind the row's end: must not count)
    sims0[5, :] = NINF                                                # a line without any explained entry: not in the mean
    sims0[6, :4] = NINF                                               # ... and one that has none among its first four
    sims0[7, 2] = NINF
    grid = [1, 2, 4, 8, 12, 30]
    got = explain.unexpectedness(torch.from_numpy(sims0), torch.from_numpy(ids), grid)
    want = O.unexpectedness_loop(sims0, ids, grid)
    np.testing.assert_allclose(got, want, rtol=1e-12, atol=1e-15)
    assert got[-1] == got[-2] and all(0.0 < v < 2.0 for v in got)
    # by hand: two lines, sims (1/2, -inf, 0) and (-inf, -inf, 1): at K = 1 only the first line counts, 1 - 1/2; at K = 3 the first
    # line is (1/2 + 1) / 2 and the second 1 - 1 = 0
    i2 = np.array([[3, 4, 5], [6, 7, 8]], dtype=np.int32)
    s2 = np.array([[.5, NINF, 0], [NINF, NINF, 1]], dtype=np.float32)
    assert explain.unexpectedness(torch.from_numpy(s2), torch.from_numpy(i2), [1, 3]) == [0.5, 0.375] == O.unexpectedness_loop(s2, i2, [1, 3])
    none = np.full((2, 3), NINF, dtype=np.float32)
    assert explain.unexpectedness(torch.from_numpy(none), torch.from_numpy(i2), [1, 3]) == [0.0, 0.0] == O.unexpectedness_loop(none, i2, [1, 3])


def test_explain_lines_text():
    import explain
    tokens = ['a', 'bb', 'c', 'd', 'e']
    ids = np.array([[0, 3, -1], [2, -1, -1]], dtype=np.int32)
    cols = np.array([[[1, 4], [2, -1], [-1, -1]], [[-1, -1], [-1, -1], [-1, -1]]], dtype=np.int32)
    sims = np.array([[[1, .5], [-0.25, NINF], [NINF, NINF]], [[NINF] * 2] * 3], dtype=np.float32)
    want = ['u1,a:bb:1.000000:e:0.500000,d:c:-0.250000', 'u2,c']
    assert explain.format_lines(['u1', 'u2'], ids, cols, sims, tokens) == want
    lines, fields = O.explain_lines(['u1', 'u2'], ids, cols, sims, tokens)
    assert lines == want and fields[0] == [('a', [('bb', '1.000000'), ('e', '0.500000')]), ('d', [('c', '-0.250000')])] and fields[1] == [('c', [])]


def test_command_lines_refuse_bad_explain_arguments(golden_dir, tmp_path):
    """parser.error, before anything asks for a GPU or reads a file"""
    import evaluate
    import recommend
    d = os.path.join(golden_dir, 'g4')
    out, why = tmp_path / 'out.txt', tmp_path / 'why.txt'
    rec = ['-d', os.path.join(d, 'data'), '-m', os.path.join(d, 'model'), '-o', str(out), '-t', '30']
    bad = (['--explain', '3'], ['--explain-output', str(why)], ['--explain', '0', '--explain-output', str(why)],
           ['--explain', '9', '--explain-output', str(why)], ['--similarity', 'dot'], ['--similarity', 'cosine', '--explain-output', str(why)],
           ['--explain', '3', '--explain-output', str(why), '--similarity', 'jaccard'], ['--explain', '3', '--explain-output', str(why), '--pool', '50'])
    for extra in bad:
        with pytest.raises(SystemExit):
            recommend.main(rec + extra)
    assert not out.exists() and not why.exists()
    ev = ['-d', os.path.join(d, 'data'), '-m', os.path.join(d, 'model'), '-t', '30', '-sl', 'im']
    for extra in (['-M', 'unexp', '--bootstrap', '10'], ['-M', 'acc', 'unexp', '--bootstrap', '10'],
                  ['-M', 'acc', 'unexp', '--bootstrap', '10', '--compare', os.path.join(d, 'model')], ['-M', 'unexp', '--similarity', 'dot'],
                  ['-M', 'unexpected']):
        with pytest.raises(SystemExit):
            evaluate.main(ev + extra)
