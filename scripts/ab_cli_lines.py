"""What evaluate.py, recommend.py and fuse.py print and write on a fixed, seeded dataset, one SHA-256 per command line: to be run on
two source trees (a git worktree of the parent commit and the branch, each with its own build of the library) whose printouts must be
identical.
  data    synth: 300 users, 300 in-matrix and 100 out-of-matrix items; two random models of k = 16, A without and B with final-B.dat
  evaluate   -sl im om; -sl im im; -M acc auc mrr ndcg map; the same with --negatives 20 -M hr ndcg mrr; -M ild cov gini unexp; the
             same with --diversify 0.5; --bootstrap 200 with and without --compare; all of them together; each on A and on B
  recommend  plain; -u; --candidates; --new-uid; --new-vid; --diversify with --explain; each on A and on B
  fuse       methods a, b, e and s over A and B: final-U.dat, final-V.dat, final-W.dat and the returned weights
python scripts/ab_cli_lines.py TREE [evaluate] [recommend] [fuse]        (TREE: the root whose top-k-rec_amd is imported; none: all three)"""
import contextlib
import hashlib
import io
import os
import sys
import tempfile

ROOT = os.path.abspath(sys.argv[1]) if len(sys.argv) > 1 else os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'top-k-rec_amd')]
os.environ.setdefault('TKR_NO_CACHE', '1')
import numpy as np
import torch

import evaluate
import fuse
import recommend
import synth
import textio

ALL = hashlib.sha256()
N_USERS, N_IN, N_OUT, K = 300, 300, 100, 16


def show(tag, *parts):
    """parts: lists of lines, arrays, or paths of files a command wrote"""
    h = hashlib.sha256()
    for part in parts:
        if isinstance(part, str):
            with open(part, 'rb') as fh:
                part = fh.read()
        elif isinstance(part, list):
            part = '\n'.join(part).encode()
        else:
            part = np.ascontiguousarray(part).tobytes()
        h.update(hashlib.sha256(part).digest())
    line = '%-92s %s' % (tag, h.hexdigest())
    ALL.update(line.encode())
    print(line, flush=True)


def quiet(main, argv):
    """main(argv) -> (what it returns, what it printed)"""
    with contextlib.redirect_stdout(io.StringIO()) as out:
        result = main(argv)
    return result, out.getvalue().splitlines()


def write_inputs(d):
    """-> (data directory, {name: model directory}, the extra input files of recommend.py)"""
    data = os.path.join(d, 'data')
    r = synth.make_ratings(n_users=N_USERS, n_in=N_IN, n_out=N_OUT, seed=5, mu=3.0, sigma=0.7)
    uid_names, vid_names = synth.write_dataset(data, r, vid_order=np.random.Generator(np.random.PCG64(6)).permutation(N_IN + N_OUT))
    rng = np.random.Generator(np.random.PCG64(7))
    models = {}
    for name in ('A', 'B'):
        models[name] = os.path.join(d, 'model' + name)
        os.makedirs(models[name])
        textio.write_matrix(os.path.join(models[name], 'final-U.dat'), (rng.standard_normal((N_USERS, K)) * 0.3).astype(np.float32), where='host')
        textio.write_matrix(os.path.join(models[name], 'final-V.dat'), (rng.standard_normal((N_IN + N_OUT, K)) * 0.3).astype(np.float32), where='host')
    textio.write_matrix(os.path.join(models['B'], 'final-B.dat'), (rng.standard_normal((N_IN + N_OUT, 1)) * 0.2).astype(np.float32), where='host')
    files = {key: os.path.join(d, key) for key in ('users', 'candidates', 'new_uid', 'new_history', 'new_vid', 'new_ratings')}

    def ratings(path, who, pool, n_fields):
        with open(path, 'w') as fh:
            for u in who:
                picks = rng.choice(len(pool), n_fields, replace=False)
                fh.write(u + ''.join(',%s:%d' % (pool[p], rng.integers(0, 2)) for p in picks) + '\n')

    with open(files['users'], 'w') as fh:
        fh.write(''.join(uid_names[u] + '\n' for u in (17, 3, 250, 3, 99)))           # a user asked for twice
    new_users, new_items = ['nu%d' % x for x in range(23)], ['nv%d' % x for x in range(11)]
    for key, names in (('new_uid', new_users), ('new_vid', new_items)):
        with open(files[key], 'w') as fh:
            fh.write(''.join(n + '\n' for n in names))
    ratings(files['new_history'], new_users, vid_names, 12)
    ratings(files['new_ratings'], [uid_names[u] for u in rng.choice(N_USERS, 120, replace=False)], new_items, 4)
    ratings(files['candidates'], [uid_names[u] for u in rng.integers(0, N_USERS, 70)], vid_names, 40)
    return data, models, files


def evaluate_cases(data, models):
    full = ['-M', 'acc', 'auc', 'mrr', 'ndcg', 'map']
    lists = ['-M', 'ild', 'cov', 'gini', 'unexp']
    for name, other in (('A', 'B'), ('B', 'A')):
        cases = [['-sl', 'im', 'om'], ['-sl', 'im', 'im'],
                 ['-sl', 'im', 'om'] + full,
                 ['-sl', 'im', 'om'] + full + ['hr', '--negatives', '20'],
                 ['-sl', 'im', 'om'] + lists,
                 ['-sl', 'im', 'om'] + lists + ['--diversify', '0.5'],
                 ['-sl', 'im', 'om'] + full + ['--bootstrap', '200'],
                 ['-sl', 'im', 'om'] + full + ['--bootstrap', '200', '--compare', models[other]],
                 ['-sl', 'im', 'om', 'im'] + full + ['hr', 'ild', 'cov', 'gini', '--negatives', '20', '--diversify', '0.5', '--bootstrap', '200',
                                                     '--compare', models[other]]]
        for argv in cases:
            lines, printed = quiet(evaluate.main, ['-d', data, '-m', models[name]] + argv)
            tag = 'evaluate %s %s' % (name, ' '.join(models[other] == a and other or a for a in argv))
            show(tag, lines, printed)


def recommend_cases(data, models, files, d):
    new_u = ['--new-uid', files['new_uid'], '--new-history', files['new_history'], '--fold-steps', '8']
    new_v = ['--new-vid', files['new_vid'], '--new-ratings', files['new_ratings'], '--fold-steps', '8']
    for name in ('A', 'B'):
        cases = [('plain', []), ('-u', ['-u', files['users']]), ('--candidates', ['--candidates', files['candidates']]), ('--new-uid', new_u),
                 ('--new-vid', new_v), ('--new-vid --new-uid', new_v + new_u[:4]),
                 ('--diversify --explain', ['--diversify', '0.6', '--explain', '3', '--explain-output', os.path.join(d, 'why.txt')])]
        for tag, argv in cases:
            out = os.path.join(d, 'lists.txt')
            lines, _ = quiet(recommend.main, ['-d', data, '-m', models[name], '-t', '10', '-o', out] + argv)
            show('recommend %s %s' % (name, tag), lines, out, *([argv[-1]] if '--explain-output' in argv else []))


def fuse_cases(data, models, d):
    learned = {'a': [], 'b': ['--samples', '40000', '--batch', '1000'], 'e': [], 's': ['--samples', '20000']}
    for method, argv in learned.items():
        out = os.path.join(d, 'fused_' + method)
        w, printed = quiet(fuse.main, ['-d', data, '-m', models['A'], models['B'], '-o', out, '--method', method, '--seed', '3'] + argv)
        written = [os.path.join(out, f) for f in ('final-U.dat', 'final-V.dat', 'final-W.dat') if os.path.exists(os.path.join(out, f))]
        show('fuse --method %s (%d files)' % (method, len(written)), np.asarray(w), printed[-1:], *written)       # (the line of weights: b and s
                                                                                                                  # also log a time and a path)


def main():
    if not torch.cuda.is_available():
        raise SystemExit('ab_cli_lines.py runs the command lines on the GPU; none is visible')
    parts = sys.argv[2:] or ['evaluate', 'recommend', 'fuse']
    with tempfile.TemporaryDirectory() as d:
        data, models, files = write_inputs(d)
        for part in parts:
            {'evaluate': lambda: evaluate_cases(data, models), 'recommend': lambda: recommend_cases(data, models, files, d),
             'fuse': lambda: fuse_cases(data, models, d)}[part]()
    torch.cuda.synchronize()
    print('all of the above: %s' % ALL.hexdigest(), flush=True)


if __name__ == '__main__':
    main()
