"""K15 against the host grouping: evaluate.load_scenario on already parsed arrays (the parse itself is K11's and is not timed: both
paths are handed the same host arrays), where='host' and where='device' alternated in one process, the seven arrays asserted equal.
The device leg is also split into its phases: upload (the parsed arrays of both files), kernels (count, scan, emit of the three CSRs,
last_line_of_user, scenario_lines, with their read-backs of a few words) and download (the seven arrays to numpy).
Shapes: ML-10M (69,878 lines, 10,677 columns, 9 M + 1 M entries), the Netflix shape (480,189 lines, 17,770 columns, 90 M + 10 M
entries) and a sweep of entry counts for the crossover (the smallest swept size at which the device, upload and download included,
wins the median).
    python scripts/time_group.py [scale] [rounds]      scale 1.0 = the shapes above; 0.1 for a quick run"""
import os, sys, time, tempfile, shutil
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'top-k-rec_amd')]
os.environ['TKR_NO_CACHE'] = '1'
import numpy as np
import torch
import evaluate
import textio
scale = float(sys.argv[1]) if len(sys.argv) > 1 else 1.0
rounds = int(sys.argv[2]) if len(sys.argv) > 2 else 3
if not torch.cuda.is_available():
    print('no GPU visible: K15 cannot be timed here')
    sys.exit(0)
sync = torch.cuda.synchronize
d = tempfile.mkdtemp(prefix='tkr_k15_')
if len(sys.argv) > 3 and sys.argv[3] == 'cli':
    # what a user sees: evaluate.py -sl im om from text (no stamped copies) on a Netflix-shaped data set, TKR_GROUP=host and =device alternated
    import contextlib, io
    import synth, utils
    shape = dict(synth.NETFLIX, n_users=max(int(synth.NETFLIX['n_users'] * scale), 64))
    data, model = os.path.join(d, 'data'), os.path.join(d, 'model')
    t0 = time.perf_counter(); r = synth.make_ratings(seed=42, **shape); synth.write_dataset(data, r)
    print('data set written in %.1f s (%.0f MB train file)' % (time.perf_counter() - t0, os.path.getsize(os.path.join(data, 'f0tr.txt')) / 1e6), flush=True)
    rng = np.random.Generator(np.random.PCG64(1))
    os.makedirs(model)
    utils.export_embed_to_file(os.path.join(model, 'final-U.dat'), (rng.standard_normal((r['n_users'], 32)) * 0.1).astype(np.float32))
    utils.export_embed_to_file(os.path.join(model, 'final-V.dat'), (rng.standard_normal((r['n_in'] + r['n_out'], 32)) * 0.1).astype(np.float32))
    ts, said = {'host': [], 'device': []}, {}
    for k in range(rounds + 1):                                      # the first pair warms up
        for where in ('host', 'device'):
            os.environ['TKR_GROUP'] = where
            before = dict(textio.group_counts)
            with contextlib.redirect_stdout(io.StringIO()) as out:
                t0 = time.perf_counter(); evaluate.main(['-d', data, '-m', model, '-sl', 'im', 'om']); t1 = time.perf_counter()
            assert textio.group_counts[where] == before[where] + 2
            said[where] = out.getvalue()
            if k:
                ts[where].append(t1 - t0)
        assert said['host'] == said['device']
    print('evaluate.py -sl im om from text, k = 32, medians of %d alternated runs, stdout equal: TKR_GROUP=host %.2f s, TKR_GROUP=device %.2f s   %s'
          % (rounds, np.median(ts['host']), np.median(ts['device']), said['host'].strip().replace('\n', ' | ')[:70]), flush=True)
    shutil.rmtree(d)
    sys.exit(0)
rng = np.random.Generator(np.random.PCG64(15))
NAMES = ('users', 'like_ptr', 'like_cols', 'rated_ptr', 'rated_cols', 'seen_ptr', 'seen_cols')
parsed = {}                                                        # path -> Ratings: what both paths are handed instead of a parse
textio.parse_ratings = lambda path, users, items, where=None: parsed[path]
textio.parse_ratings_for_group = lambda path, users, items, where: parsed[path]


def ratings(n_lines, n_entries, n_cols, line_user):
    """a parsed file: line lengths spread like a long-tailed catalogue's, items uniform (a few repeat on a line), likes 0 / 1"""
    w = rng.lognormal(0.0, 1.0, n_lines)
    lengths = np.maximum((w * (n_entries / w.sum())).astype(np.int64), 1)
    line_ptr = np.zeros(n_lines + 1, dtype=np.int64)
    np.cumsum(lengths, out=line_ptr[1:])
    n = int(line_ptr[-1])
    return textio.Ratings(line_user.astype(np.int32), line_ptr, rng.integers(0, n_cols, n, dtype=np.int32), rng.integers(0, 2, n, dtype=np.int32))


def leg(name, n_lines, n_cols, n_train, n_test, rounds):
    uids = {'u%d' % k: k for k in range(n_lines)}
    umap = textio.IdMap({})                                          # (not looked at: nothing is parsed)
    with open(os.path.join(d, 'f0te.tm.idl'), 'w') as fh:
        fh.write(''.join('i%d\n' % k for k in range(n_cols)))
    H = ratings(n_lines, n_train, n_cols, rng.permutation(n_lines))
    T = ratings(n_lines, n_test, n_cols, rng.permutation(n_lines))
    parsed[os.path.join(d, 'f0tr.txt')], parsed[os.path.join(d, 'f0te.tm.txt')] = H, T
    entries = len(H.item) + len(T.item)
    evaluate.load_scenario(d, 0, 'tm', uids, umap, where='device')    # warm-up: code objects, allocator
    ts = {'host': [], 'device': []}
    for _ in range(rounds):
        got = {}
        for where in ('host', 'device'):
            before = dict(textio.group_counts)
            sync(); t0 = time.perf_counter(); got[where] = evaluate.load_scenario(d, 0, 'tm', uids, umap, where=where); sync()
            ts[where].append(time.perf_counter() - t0)
            assert textio.group_counts[where] == before[where] + 1
        for n in NAMES:
            a, b = getattr(got['host'], n), getattr(got['device'], n)
            assert a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a, b), n
        del got
    up, total, down = [], [], []
    dev = torch.device('cuda', torch.cuda.current_device())
    for _ in range(rounds):
        sync(); t0 = time.perf_counter(); Td, Hd = textio.ratings_to_device(T, dev), textio.ratings_to_device(H, dev); sync()
        up.append(time.perf_counter() - t0)
        teids = evaluate.read_ids(os.path.join(d, 'f0te.tm.idl'))
        t0 = time.perf_counter()
        phase = {}
        sc = evaluate._load_scenario_device(Td, Hd, 'te', 'tr', teids, None, n_cols, uids, umap, 'device', timing=phase)
        sync(); total.append(time.perf_counter() - t0 - phase['download'])
        down.append(phase['download'])
        del sc, Td, Hd
    host, devt = float(np.median(ts['host'])), float(np.median(ts['device']))
    up, down = float(np.median(up)), float(np.median(down))
    print('%-10s %7d lines %6d cols %10d entries  host %8.4f s (%5.1f ns/entry)  device %8.4f s  %6.1fx   upload %.4f kernels %.4f download %.4f'
          % (name, n_lines, n_cols, entries, host, host / entries * 1e9, devt, host / devt, up, float(np.median(total)), down), flush=True)
    return entries, host, devt


print('load_scenario on parsed arrays, medians of %d alternated calls, the seven arrays equal; phases: medians of %d more device runs'
      % (rounds, rounds), flush=True)
leg('ML-10M', max(int(69878 * scale), 4), 10677, int(9e6 * scale), int(1e6 * scale), rounds)
leg('Netflix', max(int(480189 * scale), 4), 17770, int(9e7 * scale), int(1e7 * scale), rounds)
cross = None
for entries in (1 << 10, 1 << 12, 1 << 14, 1 << 16, 1 << 18, 1 << 20, 1 << 22):
    n, host, dev = leg('sweep', max(entries // 64, 4), 10000, entries * 9 // 10, entries // 10, rounds)
    if cross is None and dev < host:
        cross = n
print('crossover: the device is first ahead at %s entries; GROUP_DEVICE_FROM is %d' % (cross, textio.GROUP_DEVICE_FROM))
shutil.rmtree(d)
