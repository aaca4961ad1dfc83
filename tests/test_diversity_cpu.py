"""K17 (tkr_mmr_select, tkr_list_pair_sums) without a GPU: the oracle on a hand-worked example, the ABI and its argument checks, the
arithmetic of the list metrics on CPU tensors, and what the two command lines refuse."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _diversity_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

V_, I32, F64 = C.c_void_p, C.c_int32, C.c_double
MMR_ARGTYPES = [V_, I32, I32, V_, V_, I32, I32, F64, I32, V_, V_, V_]
PAIR_ARGTYPES = [V_, I32, I32, V_, I32, I32, V_, V_, V_]


def test_oracle_on_a_hand_worked_example():
    """four items in two dimensions: 0 and 1 point the same way, 2 is orthogonal to them, 3 lies between.  sim: s01 = 1, s02 = s12 = 0,
    s03 = s13 = s23 = 1/2.  rel = 1, 3/4, 1/2, 1/4 and lambda = 1/2 give a = 1/2, 3/8, 1/4, 1/8.
      pick 0: entry 0 (gap 1/8).
      pick 1: pen = (., 1, 0, 1/2), obj = (., -1/8, 1/4, -1/8): entry 2 (gap 3/8) -- the orthogonal item overtakes the duplicate.
      pick 2: pen = (., 1, ., 1/2), obj = (., -1/8, ., -1/8): a tie, the lower position 1 wins (gap 0: the row is ambiguous).
      pick 3: entry 3."""
    S = np.array([[1, 0], [1, 0], [0, 1], [0.5, 0.5]], dtype=np.float32)
    ids = np.array([[0, 1, 2, 3]], dtype=np.int32)
    rel = np.array([[1.0, 0.75, 0.5, 0.25]], dtype=np.float32)
    np.testing.assert_array_equal(O.sims(S, ids[0]), [[1, 1, 0, .5], [1, 1, 0, .5], [0, 0, 1, .5], [.5, .5, .5, .5]])
    sel, gap = O.mmr_row(S, ids[0], rel[0], 0.5, 4, 4)
    assert sel.tolist() == [0, 2, 1, 3] and gap == 0.0
    sel, gap = O.mmr_row(S, ids[0], rel[0], 0.5, 2, 4)
    assert sel.tolist() == [0, 2] and gap == 0.125
    assert O.mmr(S, ids, rel, 1.0, 3, 4)[0].tolist() == [[0, 1, 2]]                  # lambda = 1: the pool's own order
    assert O.mmr(S, ids, rel, 0.0, 4, 4)[0].tolist() == [[0, 2, 3, 1]]               # lambda = 0: a tie first, then similarity alone
    # the prefix rule: a negative id and an id >= n_items end the row; what follows is ignored
    cut = np.array([[0, 1, -1, 3], [0, 1, 2, 4], [-1, 0, 1, 2]], dtype=np.int32)
    sel, _ = O.mmr(S, cut, np.repeat(rel, 3, 0), 0.5, 3, 4)
    assert sel.tolist() == [[0, 1, -1], [0, 2, 1], [-1, -1, -1]]
    # the pair sums of the list 0, 2, 1, 3: 0;  1 - s02;  (1 - s01) + (1 - s12);  three halves
    np.testing.assert_array_equal(O.pair_sums(S, np.array([[0, 2, 1, 3], [0, 2, -1, 3]], dtype=np.int32), 4), [[0, 1, 1, 1.5], [0, 1, 0, 0]])


def test_header_binding_and_library_agree_and_check_their_arguments():
    import tkr_hip
    header = open(os.path.join(ROOT, 'include', 'tkr.h')).read()
    declared = re.findall(r'^int(?:32_t|64_t)? (tkr_\w+)\(', header, flags=re.M)
    lib = C.CDLL(tkr_hip.LIB_PATH)
    for name in ('tkr_mmr_select', 'tkr_list_pair_sums'):
        assert name in declared and name in tkr_hip.EXPORTS and hasattr(lib, name)
    assert re.search(r'#define TKR_VERSION 120\b', header) and tkr_hip.VERSION == 120 and lib.tkr_version() == 120
    assert re.search(r'#define TKR_MMR_MAX_POOL %d\b' % tkr_hip.MMR_MAX_POOL, header)
    assert callable(tkr_hip.mmr_select) and callable(tkr_hip.list_pair_sums)
    p = 4096                                                          # never dereferenced: every call below fails its checks
    fn = lib.tkr_mmr_select
    fn.restype, fn.argtypes = C.c_int, MMR_ARGTYPES
    good = dict(S=p, n_items=600, k=8, ids=p, rel=p, n_rows=3, N=100, lam=0.5, t=30, sel=p, status=p, stream=None)
    assert len(good) == len(MMR_ARGTYPES)
    for change in (dict(S=None), dict(ids=None), dict(rel=None), dict(sel=None), dict(status=None), dict(N=0), dict(N=-1), dict(t=0), dict(t=101),
                   dict(k=0), dict(n_items=0), dict(n_rows=0), dict(lam=float('nan')), dict(lam=float('inf')), dict(lam=-0.01), dict(lam=1.01)):
        assert fn(*dict(good, **change).values()) == -1, change
    assert fn(*dict(good, N=1025).values()) == -2                     # TKR_E_UNSUPPORTED
    assert fn(*dict(good, N=1025, t=1025).values()) == -2
    assert fn(*dict(good, N=1025, t=0).values()) == -1                # what is invalid is invalid at any size
    fn = lib.tkr_list_pair_sums
    fn.restype, fn.argtypes = C.c_int, PAIR_ARGTYPES
    good = dict(S=p, n_items=600, k=8, ids=p, n_rows=3, t=30, out=p, status=p, stream=None)
    assert len(good) == len(PAIR_ARGTYPES)
    for change in (dict(S=None), dict(ids=None), dict(out=None), dict(status=None), dict(t=0), dict(k=0), dict(n_items=0), dict(n_rows=0)):
        assert fn(*dict(good, **change).values()) == -1, change
    assert fn(*dict(good, t=1025).values()) == -2


def test_wrappers_refuse_on_the_host():
    """tensor properties are looked at before the library is asked: CPU tensors never reach a kernel"""
    import tkr_hip
    S, ids, rel = torch.zeros((5, 4)), torch.zeros((2, 3), dtype=torch.int32), torch.zeros((2, 3))
    with pytest.raises(tkr_hip.TkrError, match='GPU'):
        tkr_hip.mmr_select(S, ids, rel, 0.5, 2)
    with pytest.raises(tkr_hip.TkrError, match='int32'):
        tkr_hip.list_pair_sums(S, ids.long())


def test_list_metrics_arithmetic_against_a_loop():
    import diversity
    rng = np.random.Generator(np.random.PCG64(17))
    n, t, n_cols = 23, 12, 40
    ids = np.stack([rng.choice(n_cols, t, replace=False) for _ in range(n)]).astype(np.int32)
    for r, cut in ((0, 0), (1, 1), (2, 2), (3, 5), (4, 11)):          # empty, one entry, two, ...; and a -1 in the middle
        ids[r, cut:] = -1
    ids[5, 4] = -1                                                    # everything behind it is ignored
    pair = rng.random((n, t)) * np.arange(t)
    pair[5, 6] = 1e9                                                  # (behind the row's end: must not count)
    grid = [1, 2, 4, 8, 12]
    got = diversity.metrics_from_pair_sums(torch.from_numpy(pair), torch.from_numpy(ids), n_cols, grid)
    want = O.metrics_loop(pair, ids, n_cols, grid)
    assert sorted(got) == ['cov', 'gini', 'ild']
    for m in got:
        np.testing.assert_allclose(got[m], want[m], rtol=1e-12, atol=1e-15, err_msg=m)
    assert got['ild'][0] == 0.0 and 0 < got['cov'][0] < got['cov'][-1] <= 1.0
    # Gini by hand: equal exposure 0; one column takes everything (n - 1) / n; counts 1, 3: (-1 * 1 + 1 * 3) / (2 * 4) = 1/4
    assert diversity.gini(torch.tensor([3, 3, 3, 3])) == 0.0
    assert diversity.gini(torch.tensor([0, 0, 0, 7])) == pytest.approx(0.75, abs=1e-15)
    assert diversity.gini(torch.tensor([3, 1])) == pytest.approx(0.25, abs=1e-15)
    assert diversity.gini(torch.zeros(5)) == 0.0
    # relevance: min-max over the valid prefix, 0 in the padding, all 0 for a flat or single-entry row
    s = torch.tensor([[3.0, 2.0, 1.0, 9.0], [5.0, 5.0, 5.0, 5.0], [4.0, 0.0, 0.0, 0.0], [2.0, 1.0, 0.5, 0.0]])
    i = torch.tensor([[7, 8, 9, -1], [1, 2, 3, 4], [6, -1, 2, 3], [1, 2, 3, 4]], dtype=torch.int32)
    np.testing.assert_array_equal(diversity.relevance(i, s).numpy(), [[1, .5, 0, 0], [0, 0, 0, 0], [0, 0, 0, 0], [1, .5, .25, 0]])
    V = torch.tensor([[3.0, 4.0], [0.0, 0.0], [0.0, -2.0]])
    np.testing.assert_allclose(diversity.similarity_table(V, 'cosine').numpy(), [[.6, .8], [0, 0], [0, -1]], rtol=1e-7)
    assert diversity.similarity_table(V, 'dot') is V
    with pytest.raises(ValueError):
        diversity.similarity_table(V, 'jaccard')


def test_command_lines_refuse_bad_diversify_arguments(golden_dir, tmp_path, monkeypatch):
    """parser.error, before anything asks for a GPU or reads a file"""
    import evaluate
    import recommend
    d = os.path.join(golden_dir, 'g4')
    out = tmp_path / 'out.txt'
    rec = ['-d', os.path.join(d, 'data'), '-m', os.path.join(d, 'model'), '-o', str(out), '-t', '30']
    ev = ['-d', os.path.join(d, 'data'), '-m', os.path.join(d, 'model'), '-t', '30', '-sl', 'im']
    bad = (['--diversify', '0.5', '--pool', '29'], ['--diversify', '0.5', '--pool', '1025'], ['--diversify', '1.5'], ['--diversify', '-0.1'],
           ['--diversify', 'nan'], ['--pool', '50'], ['--similarity', 'dot'], ['--diversify', '0.5', '--similarity', 'jaccard'])
    for extra in bad:
        for main, base in ((recommend.main, rec), (evaluate.main, ev)):
            with pytest.raises(SystemExit):
                main(base + extra)
    assert not out.exists()
    monkeypatch.setenv('WORLD_SIZE', '2')                             # a multi-rank launcher: whole-list figures are not sharded
    for extra in (['-M', 'ild'], ['-M', 'acc', 'gini'], ['--diversify', '0.5']):
        with pytest.raises(SystemExit):
            evaluate.main(ev + extra)
