"""K13 at the shapes recommend.py and the model writer meet: the parent commit's path (recommend.format_lines and its write loop;
tkr_matrix_write) against textio.write_lists / write_matrix with where='device', in one process, the two legs alternated, the files
asserted byte-equal.  Medians and spreads (max - min) of `rounds` runs; the device leg split into kernels (device events), download
and file write.  Needs a GPU.
    python scripts/time_write_lists.py [scale] [rounds] [parts]
        scale 1.0 = 480,189 users; parts: any of lists,matrix,sweep,phases (default: all)
    lists   ML-10M 69,878 x 30 and Netflix 480,189 x 30: ids and scores from K4 on random rank-128 factors, decimal tokens as synth.py's
    matrix  480,189 x 128 through write_matrix
    sweep   list sizes from 2^12 to 2^24 fields in powers of 4 -> the smallest size at which the device's median beats the host's by
            more than both spreads (TKR_FORMAT_DEVICE_FROM)
    phases  a whole recommend.py run at the Netflix shape, phase by phase: read model, parse, rated_csr, K4, format, write"""
import os, shutil, sys, tempfile, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'top-k-rec_amd')]
import numpy as np
import torch
import recommend, synth, textio, tkr_hip
from evaluate import read_ids, read_matrix

scale = float(sys.argv[1]) if len(sys.argv) > 1 else 1.0
rounds = int(sys.argv[2]) if len(sys.argv) > 2 else 3
parts = (sys.argv[3] if len(sys.argv) > 3 else 'lists,matrix,sweep,phases').split(',')
assert torch.cuda.is_available(), 'a measurement without a GPU says nothing'
os.environ['TKR_NO_CACHE'] = '1'
dev = torch.device('cuda', 0)
sync = torch.cuda.synchronize
d = tempfile.mkdtemp(prefix='tkr_fmt_')
K, k = 30, 128
med = lambda ts: float(np.median(ts))
spread = lambda ts: max(ts) - min(ts)
show = lambda ts: 'median %.3f spread %.3f s (%s)' % (med(ts), spread(ts), ' '.join('%.3f' % t for t in ts))


def topk(n_users, n_items, seed):
    """-> (ids, scores) [n_users, K] on the device: K4 on random factors"""
    g = torch.Generator(device='cpu').manual_seed(seed)
    U = (0.1 * torch.randn(n_users, k, generator=g)).to(dev)
    V = (0.1 * torch.randn(n_items, k, generator=g)).to(dev)
    return tkr_hip.score_topk(U, V, K, want_scores=True)


def parent_write(path, users, ids, scores, items):
    """the parent commit's recommend.py: download, format_lines, the write loop -> seconds of (download, format, write)"""
    t0 = time.perf_counter(); ids, scores = ids.cpu().numpy(), scores.cpu().numpy(); t1 = time.perf_counter()
    lines = recommend.format_lines(users, ids, scores, items); t2 = time.perf_counter()
    with open(path, 'w') as fh:
        for ln in lines:
            fh.write(ln + '\n')
    return t1 - t0, t2 - t1, time.perf_counter() - t2


def lists_legs(name, ids, scores, uid_names, vid_names, quiet=False):
    """alternated runs of both writers on one shape -> (host totals, device totals)"""
    n = int(ids.shape[0])
    users, items = uid_names[:n], dict(enumerate(vid_names))
    umap, vmap = textio.IdMap({t: i for i, t in enumerate(users)}), textio.IdMap({t: i for i, t in enumerate(vid_names)})
    rows = np.arange(n, dtype=np.int32)
    hp, dp = os.path.join(d, 'host.txt'), os.path.join(d, 'dev.txt')
    textio.write_lists(dp, umap, ids, scores, rows, vmap, where='device'); sync()          # warm-up: code objects, token tables
    host, device, split, hsplit = [], [], [], []
    for _ in range(rounds):
        t0 = time.perf_counter(); hsplit.append(parent_write(hp, users, ids, scores, items)); host.append(time.perf_counter() - t0)
        timing = {}
        t0 = time.perf_counter(); textio.write_lists(dp, umap, ids, scores, rows, vmap, where='device', timing=timing); sync()
        device.append(time.perf_counter() - t0)
        split.append(timing)
        assert open(hp, 'rb').read() == open(dp, 'rb').read()
    if not quiet:
        print('%s lists %d x %d (%d fields, %.1f MB of text), %d alternated runs, files byte-equal' % (name, n, K, n * K, os.path.getsize(dp) / 1e6, rounds))
        print('  host   (download + format_lines + write loop)  %s' % show(host))
        print('         of that: download %.3f, format_lines %.3f, write loop %.3f s (medians)' % tuple(med([h[i] for h in hsplit]) for i in range(3)))
        print('  device (write_lists where=device)              %s' % show(device))
        print('         of that: kernels %.4f (device events), download %.3f, file write %.3f s (medians); the rest is host code and allocation'
              % tuple(med([s.get(key, 0.0) for s in split]) for key in ('kernels', 'download', 'write')))
        print('  host over device: %.1fx on the medians' % (med(host) / med(device)), flush=True)
    return host, device


uid_all = [str(x + 1) for x in range(max(int(480189 * scale), 1 << 10))]
vid_nf = [str(1000 + 3 * x) for x in range(17770)]
ids_nf = scores_nf = None
if 'lists' in parts or 'sweep' in parts:
    ids_nf, scores_nf = topk(int(480189 * scale), 17770, 1)
if 'lists' in parts:
    n_ml = int(69878 * scale)
    ids_ml, scores_ml = topk(n_ml, 10380, 2)
    lists_legs('ML-10M', ids_ml, scores_ml, uid_all, [str(1000 + 3 * x) for x in range(10380)])
    del ids_ml, scores_ml
    lists_legs('Netflix', ids_nf, scores_nf, uid_all, vid_nf)

if 'matrix' in parts:
    n = int(480189 * scale)
    g = torch.Generator(device='cpu').manual_seed(3)
    M = (0.1 * torch.randn(n, k, generator=g))
    M_host, M_dev = M.numpy(), M.to(dev)
    hp, dp = os.path.join(d, 'host.dat'), os.path.join(d, 'dev.dat')
    textio.write_matrix(dp, M_dev[:1000], where='device'); sync()
    host, device, split, upload = [], [], [], []
    for _ in range(rounds):
        t0 = time.perf_counter(); textio.write_matrix(hp, M_host, where='host'); host.append(time.perf_counter() - t0)
        timing = {}
        t0 = time.perf_counter(); textio.write_matrix(dp, M_dev, where='device', timing=timing); sync(); device.append(time.perf_counter() - t0)
        split.append(timing)
        t0 = time.perf_counter(); torch.from_numpy(M_host).to(dev); sync(); upload.append(time.perf_counter() - t0)
        assert open(hp, 'rb').read() == open(dp, 'rb').read()
    print('matrix %d x %d (%d elements, %.1f MB of text), %d alternated runs, files byte-equal' % (n, k, n * k, os.path.getsize(dp) / 1e6, rounds))
    print('  host   (tkr_matrix_write)                       %s' % show(host))
    print('  device (write_matrix where=device, tensor on the GPU) %s' % show(device))
    print('         of that: kernels %.4f (device events), download %.3f, file write %.3f s (medians); a host array adds its upload, %.3f s'
          % (tuple(med([s.get(key, 0.0) for s in split]) for key in ('kernels', 'download', 'write')) + (med(upload),)))
    print('  host over device: %.1fx on the medians' % (med(host) / med(device)), flush=True)
    del M, M_host, M_dev

if 'sweep' in parts:
    print('sweep of list sizes (K = %d), %d alternated runs each' % (K, rounds))
    chosen = None
    top = 24 if scale >= 1.0 else 20
    for e in range(12, top + 1, 2):
        n = max((1 << e) // K, 1)
        pick = torch.arange(n, device=dev) % ids_nf.shape[0]
        names = uid_all if n <= len(uid_all) else [str(x + 1) for x in range(n)]
        host, device = lists_legs('', ids_nf[pick].contiguous(), scores_nf[pick].contiguous(), names, vid_nf, quiet=True)
        wins = med(device) + spread(device) + spread(host) < med(host)
        if wins and chosen is None:
            chosen = n * K
        if not wins:
            chosen = None                                             # the threshold is where the device wins from there upward
        print('  2^%d fields (%d rows): host %s | device %s | device %s' % (e, n, show(host), show(device), 'wins' if wins else 'does not win'), flush=True)
    print('smallest measured size from which the device wins by more than both spreads: %s fields (TKR_FORMAT_DEVICE_FROM is never below 65536)'
          % (chosen,), flush=True)

if 'phases' in parts:
    spec = dict(synth.NETFLIX, n_users=int(synth.NETFLIX['n_users'] * scale))
    t0 = time.perf_counter()
    r = synth.make_ratings(seed=42, **spec)
    n_users, n_items = spec['n_users'], r['n_in'] + r['n_out']
    data, model = os.path.join(d, 'data'), os.path.join(d, 'model')
    os.makedirs(data); os.makedirs(model)
    uid_names, vid_names = uid_all[:n_users], [str(1000 + 3 * x) for x in range(n_items)]
    open(os.path.join(data, 'uid'), 'w').write(''.join(t + '\n' for t in uid_names))
    open(os.path.join(data, 'vid'), 'w').write(''.join(t + '\n' for t in vid_names))
    tok = [',%s:%d' % (v, l) for v in vid_names for l in (0, 1)]
    idx = (2 * r['tr_i'] + r['tr_l']).tolist()
    cuts = np.flatnonzero(np.r_[True, r['tr_u'][1:] != r['tr_u'][:-1], True]).tolist()
    with open(os.path.join(data, 'f0tr.txt'), 'w') as fh:
        for q, u in enumerate(r['tr_u'][cuts[:-1]].tolist()):
            fh.write(uid_names[u] + ''.join(map(tok.__getitem__, idx[cuts[q]:cuts[q + 1]])) + '\n')
    g = torch.Generator(device='cpu').manual_seed(4)
    textio.write_matrix(os.path.join(model, 'final-U.dat'), (0.1 * torch.randn(n_users, k, generator=g)).to(dev), where='device')
    textio.write_matrix(os.path.join(model, 'final-V.dat'), (0.1 * torch.randn(n_items, k, generator=g)).to(dev), where='device')
    print('phases: wrote the data and model directories (%d users, %d items, %d ratings, train file %.2f GB) in %.0f s'
          % (n_users, n_items, len(idx), os.path.getsize(os.path.join(data, 'f0tr.txt')) / 1e9, time.perf_counter() - t0), flush=True)
    del r, idx, tok
    ph = {}

    def phase(name, t0):
        sync()
        ph[name] = ph.get(name, 0.0) + time.perf_counter() - t0

    # the statements of recommend.main, in its order, timed one by one
    t0 = time.perf_counter(); uids, vids = read_ids(os.path.join(data, 'uid')), read_ids(os.path.join(data, 'vid')); users = list(uids); phase('read ids', t0)
    t0 = time.perf_counter(); vmat = read_matrix(os.path.join(model, 'final-V.dat'), vids); umat = read_matrix(os.path.join(model, 'final-U.dat'), uids); phase('read model', t0)
    t0 = time.perf_counter(); V_dev, U_dev = torch.from_numpy(vmat).to(dev), torch.from_numpy(umat).to(dev); phase('upload model', t0)
    t0 = time.perf_counter(); umap, vmap = textio.IdMap(uids), textio.IdMap(vids); phase('id tables', t0)
    t0 = time.perf_counter(); R = textio.parse_ratings(os.path.join(data, 'f0tr.txt'), umap, vmap); phase('parse (%s)' % ('device' if textio.parse_counts['device'] else 'host'), t0)
    t0 = time.perf_counter()
    user_rows = [uids[u] for u in users]
    rows_of_user = {}
    for row, user in enumerate(user_rows):
        rows_of_user.setdefault(int(user), []).append(row)
    ptr, cols = recommend.rated_csr(R, rows_of_user, len(user_rows), n_items)
    phase('rated_csr', t0)
    t0 = time.perf_counter()
    mask, pitch = tkr_hip.build_rated_mask(torch.from_numpy(ptr).to(dev), torch.from_numpy(cols).to(dev), len(user_rows), n_items)
    idx_dev = torch.from_numpy(np.asarray(user_rows, dtype=np.int32)).to(dev)
    phase('mask upload + build', t0)
    tkr_hip.score_topk(U_dev, V_dev, K, user_idx=idx_dev, mask=mask, mask_pitch=pitch, want_scores=True); sync()      # warm-up
    t0 = time.perf_counter(); ids, scores = tkr_hip.score_topk(U_dev, V_dev, K, user_idx=idx_dev, mask=mask, mask_pitch=pitch, want_scores=True); phase('K4', t0)
    out = os.path.join(d, 'rec.txt')
    t0 = time.perf_counter(); tokens, rows = recommend.row_tokens(users); phase('row tokens', t0)
    textio.write_lists(out, tokens, ids, scores, rows, vmap, where='device'); sync()                                    # warm-up
    timing = {}
    t0 = time.perf_counter(); textio.write_lists(out, tokens, ids, scores, rows, vmap, where='device', timing=timing); phase('format + write (device)', t0)
    t0 = time.perf_counter(); lines = open(out, 'rb').read().decode().split('\n')[:-1]; phase('lines for the caller', t0)
    th = parent_write(os.path.join(d, 'rec_host.txt'), users, ids, scores, {i: t for t, i in vids.items()})
    assert open(out, 'rb').read() == open(os.path.join(d, 'rec_host.txt'), 'rb').read() and len(lines) == n_users
    print('phases of recommend.py at %d users x %d items, -t %d (one run, seconds):' % (n_users, n_items, K))
    for name, t in ph.items():
        print('  %-28s %8.3f' % (name, t))
    print('  of format + write (device): kernels %.4f, download %.3f, file write %.3f' % tuple(timing.get(key, 0.0) for key in ('kernels', 'download', 'write')))
    print('  the parent commit in place of it: download %.3f + format_lines %.3f + write loop %.3f = %.3f' % (th + (sum(th),)), flush=True)
shutil.rmtree(d)
