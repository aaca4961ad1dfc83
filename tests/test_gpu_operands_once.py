"""evaluate.py builds a scenario's operands once per entry of -sl, and recommend.py reads final-U.dat once: counted through shims around
tkr_hip.build_rated_mask and textio.read_matrix, with the output lines held to those of the same run without the shim."""
import os

import numpy as np
import pytest

import evaluate
import recommend
import synth
import textio
import tkr_hip

pytestmark = pytest.mark.gpu
N_USERS, N_IN, N_OUT, K = 300, 300, 100, 16


@pytest.fixture(scope='module')
def inputs(tmp_path_factory):
    """a synth dataset and two random models, B with a bias -> (data directory, model A, model B, the directory)"""
    d = str(tmp_path_factory.mktemp('once'))
    data = os.path.join(d, 'data')
    r = synth.make_ratings(n_users=N_USERS, n_in=N_IN, n_out=N_OUT, seed=5, mu=3.0, sigma=0.7)
    uid_names, _ = synth.write_dataset(data, r)
    rng = np.random.Generator(np.random.PCG64(7))
    models = []
    for name in ('A', 'B'):
        models.append(os.path.join(d, name))
        os.makedirs(models[-1])
        for file, rows in (('final-U.dat', N_USERS), ('final-V.dat', N_IN + N_OUT)):
            textio.write_matrix(os.path.join(models[-1], file), (rng.standard_normal((rows, K)) * 0.3).astype(np.float32), where='host')
    textio.write_matrix(os.path.join(models[1], 'final-B.dat'), (rng.standard_normal((N_IN + N_OUT, 1)) * 0.2).astype(np.float32), where='host')
    with open(os.path.join(d, 'new_vid'), 'w') as fh:
        fh.write(''.join('nv%d\n' % x for x in range(7)))
    with open(os.path.join(d, 'new_ratings'), 'w') as fh:
        for u in rng.choice(N_USERS, 90, replace=False):
            fh.write(uid_names[u] + ''.join(',nv%d:%d' % (x, rng.integers(0, 2)) for x in rng.choice(7, 3, replace=False)) + '\n')
    return data, models[0], models[1], d


def counted(monkeypatch, module, name, counts_it=lambda *a, **k: True):
    """module.name wrapped: -> a list that receives one entry per call `counts_it` accepts"""
    calls, real = [], getattr(module, name)

    def shim(*args, **kwargs):
        if counts_it(*args, **kwargs):
            calls.append(args)
        return real(*args, **kwargs)
    monkeypatch.setattr(module, name, shim)
    return calls


@pytest.mark.parametrize('flags,scenarios', [
    (['-M', 'acc', 'ndcg', 'ild', '--diversify', '0.5', '--bootstrap', '50', '--compare', 'B'], ['im', 'om']),
    (['-M', 'acc', 'ndcg', 'ild', 'unexp', '--diversify', '0.5'], ['im', 'om']),
    (['-M', 'acc', 'ndcg', '--negatives', '20'], ['im', 'im'])])
def test_one_rated_mask_per_scenario_entry(inputs, monkeypatch, capsys, flags, scenarios):
    """every consumer of the mask on one command line (unexp is refused together with --bootstrap, so it has a line of its own), and a
    scenario listed twice, whose second entry only ranks for the accuracy line.  Before the operands were shared these lines made 8, 6
    and 3 calls"""
    data, A, B, _ = inputs
    argv = ['-d', data, '-m', A, '-sl'] + scenarios + [B if f == 'B' else f for f in flags]
    want = evaluate.main(argv)
    printed = capsys.readouterr().out
    calls = counted(monkeypatch, tkr_hip, 'build_rated_mask')
    got = evaluate.main(argv)
    assert len(calls) == len(scenarios)
    assert got == want and capsys.readouterr().out == printed and len(want) > len(scenarios)


def test_recommend_reads_final_u_once(inputs, monkeypatch, tmp_path):
    data, _, B, d = inputs
    argv = ['-d', data, '-m', B, '-t', '10', '--new-vid', os.path.join(d, 'new_vid'), '--new-ratings', os.path.join(d, 'new_ratings'),
            '--fold-steps', '8']
    want = recommend.main(argv + ['-o', str(tmp_path / 'want.txt')])
    calls = counted(monkeypatch, textio, 'read_matrix', lambda path, *a, **k: os.path.basename(path) == 'final-U.dat')
    got = recommend.main(argv + ['-o', str(tmp_path / 'got.txt')])
    assert len(calls) == 1                                            # (the fold-in and the model users' ranking both need it)
    assert got == want and len(got) == N_USERS
