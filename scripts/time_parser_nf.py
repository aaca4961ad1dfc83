"""n1/n2 at Netflix scale: write a ~10^8-rating train file in the reference's text format (uid,iid:like,...), then time
BPR.load_training_data's native one-pass parser on it, cold and from the stamped binary copy.  The host leg needs no GPU.  With
one, a device leg follows on the same file in the same process: K11 (csrc/parse_dev.hip) after one warm-up parse, its arrays
asserted equal to the host parser's, then upload / kernels (device events around the launches) / download on their own, the
kernels at several chunk sizes, and whole textio.parse_ratings calls from text (no stamped copy) with where='host' and
where='device' alternated.
    python scripts/time_parser_nf.py [scale] [rounds]      scale 1.0 = 480,189 users, ~1e8 ratings; 0.1 for a quick run"""
import os, sys, time, tempfile
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'top-k-rec_amd')]
import numpy as np
import synth, textio
scale = float(sys.argv[1]) if len(sys.argv) > 1 else 1.0
spec = dict(synth.NETFLIX, n_users=int(synth.NETFLIX['n_users'] * scale))
t0 = time.time()
r = synth.make_ratings(seed=42, **spec)
n_items = r['n_in'] + r['n_out']
print('generated %d train ratings for %d users in %.1f s' % (len(r['tr_u']), spec['n_users'], time.time() - t0), flush=True)
d = tempfile.mkdtemp(prefix='tkr_nf_')
uid_names = [str(x + 1) for x in range(spec['n_users'])]
vid_names = [str(1000 + 3 * x) for x in range(n_items)]
tok = [',%s:%d' % (v, l) for v in vid_names for l in (0, 1)]          # token of (item, like) = tok[2 * item + like]
path = os.path.join(d, 'f0tr.txt')
t0 = time.time()
idx = (2 * r['tr_i'] + r['tr_l']).tolist()
cuts = np.flatnonzero(np.r_[True, r['tr_u'][1:] != r['tr_u'][:-1], True]).tolist()
users = r['tr_u'][cuts[:-1]].tolist()
with open(path, 'w') as fh:
    get = tok.__getitem__
    for q, u in enumerate(users):
        fh.write(uid_names[u] + ''.join(map(get, idx[cuts[q]:cuts[q + 1]])) + '\n')
print('wrote %s (%.2f GB) in %.1f s' % (path, os.path.getsize(path) / 1e9, time.time() - t0), flush=True)
uids = {n: i for i, n in enumerate(uid_names)}
vids = {n: i for i, n in enumerate(vid_names)}
os.environ['TKR_NO_CACHE'] = '0'
t0 = time.time(); um, vm = textio.IdMap(uids), textio.IdMap(vids); t_maps = time.time() - t0
t0 = time.time(); R = textio.parse_ratings(path, um, vm, where='host'); t_cold = time.time() - t0
t0 = time.time(); R2 = textio.parse_ratings(path, um, vm); t_warm = time.time() - t0
assert np.array_equal(R.item, R2.item) and len(R.item) == len(r['tr_u'])
print('id tables %.2f s; parse_ratings: %.2f s from text (%.0f M ratings/s, %.2f GB/s), %.2f s from the stamped copy (%s.csr.npz, %.2f GB)'
      % (t_maps, t_cold, len(R.item) / t_cold / 1e6, os.path.getsize(path) / t_cold / 1e9, t_warm, os.path.basename(path),
         os.path.getsize(path + '.csr.npz') / 1e9), flush=True)
import shutil, torch, tkr_hip
if not torch.cuda.is_available():
    print('no GPU visible: host leg only')
    shutil.rmtree(d)
    sys.exit(0)
rounds = int(sys.argv[2]) if len(sys.argv) > 2 else 3
os.environ['TKR_NO_CACHE'] = '1'
os.remove(path + '.csr.npz')
dev = torch.device('cuda', 0)
sync = torch.cuda.synchronize
t0 = time.time(); D = textio.parse_ratings_device(path, um, vm).host(); sync(); t_first = time.time() - t0        # warm-up: code objects, id tables
for name in ('line_user', 'line_ptr', 'item', 'like'):
    a, b = getattr(D, name), getattr(R, name)
    assert a.dtype == b.dtype and np.array_equal(a, b), name
print('device == host on all four arrays (%d lines, %d entries); first device parse, id tables included, %.2f s' % (len(D.line_user), len(D.item), t_first), flush=True)
del D


def split(chunk):
    """-> seconds of (upload, count kernels, emit kernels, download) of one device parse"""
    t0 = time.time(); text = torch.from_numpy(np.memmap(path, dtype=np.uint8, mode='c')).to(dev); sync(); t_up = time.time() - t0
    ws = torch.empty(tkr_hip.parse_dev_workspace_bytes(text.numel(), chunk), dtype=torch.uint8, device=dev)
    totals, status = torch.empty(2, dtype=torch.int64, device=dev), torch.empty(1, dtype=torch.int64, device=dev)
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
    ev[0].record(); tkr_hip.ratings_count_dev(text, chunk, ws, totals); ev[1].record()
    n_lines, n_entries = totals.tolist()
    tables = um.device_table(dev), vm.device_table(dev)
    torch.empty(20 * n_lines + 12 * n_entries + 64, dtype=torch.uint8, device=dev)          # the allocator has the outputs' blocks before the timed launches
    ev[2].record(); out = textio.RatingsDevice(*tkr_hip.ratings_emit_dev(text, chunk, ws, n_lines, n_entries, tables[0], tables[1], status)); ev[3].record()
    sync()
    assert int(status.item()) == -1
    t0 = time.time(); out.host(); t_down = time.time() - t0
    return t_up, ev[0].elapsed_time(ev[1]) / 1e3, ev[2].elapsed_time(ev[3]) / 1e3, t_down


split(textio.PARSE_CHUNK_BYTES)
for chunk in (1024, 4096, 16384, 65536, 262144):
    t_up, t_count, t_emit, t_down = split(chunk)
    print('chunk_bytes %7d: upload %.3f s, kernels %.4f s (count + scan %.4f, positions + fields + lines %.4f), download %.3f s'
          % (chunk, t_up, t_count + t_emit, t_count, t_emit, t_down), flush=True)
legs = {'host': [], 'device': []}
for _ in range(rounds):
    for where in ('host', 'device'):
        t0 = time.time(); textio.parse_ratings(path, um, vm, where=where); sync(); legs[where].append(time.time() - t0)
for where, ts in legs.items():
    print('parse_ratings(where=%r) from text, %d alternated calls: min %.3f median %.3f max %.3f s   %s'
          % (where, rounds, min(ts), float(np.median(ts)), max(ts), ' '.join('%.3f' % t for t in ts)), flush=True)
print('device over host: %.1fx on the medians; file %.3f GB' % (np.median(legs['host']) / np.median(legs['device']), os.path.getsize(path) / 1e9))
shutil.rmtree(d)
