"""K14 against the host reader: '%f ' matrices written with textio.write_matrix, read back from text (TKR_NO_CACHE=1) by
textio.read_matrix with where='host' and where='device' alternated in one process, the arrays asserted byte-equal.  The device
leg is also split into its phases: upload (memmap -> one copy), kernels (count, scan, positions, convert, with the two read-backs of
a few words), patch (the hard tokens through the host's strtod) and download of the finished array.
Shapes: 10,380 x 128, 69,878 x 128 and 480,189 x 128 model-like values, one file of random fp32 bit patterns (about a third of its
tokens have more than 19 digits and go through the host), and a sweep of small sizes around the crossover.
    python scripts/time_read_matrix.py [scale] [rounds]      scale 1.0 = the shapes above; 0.1 for a quick run"""
import os, sys, time, tempfile, shutil
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'top-k-rec_amd')]
os.environ['TKR_NO_CACHE'] = '1'
import numpy as np
import torch
import textio
scale = float(sys.argv[1]) if len(sys.argv) > 1 else 1.0
rounds = int(sys.argv[2]) if len(sys.argv) > 2 else 3
if not torch.cuda.is_available():
    print('no GPU visible: K14 cannot be timed here')
    sys.exit(0)
sync = torch.cuda.synchronize
d = tempfile.mkdtemp(prefix='tkr_k14_')
rng = np.random.Generator(np.random.PCG64(14))


def model_like(rows, cols=128):
    return (0.1 * rng.standard_normal((rows, cols))).astype(np.float32)


def bit_patterns(rows, cols=128):
    bits = rng.integers(0, 1 << 32, (rows, cols), dtype=np.uint64).astype(np.uint32)
    return bits.view(np.float32)


def leg(name, m, rounds):
    """-> (median host seconds, median device seconds) of read_matrix on the text of m"""
    path = os.path.join(d, name + '.dat')
    textio.write_matrix(path, m)
    size = os.path.getsize(path)
    first = textio.read_matrix_device(path)                        # warm-up: code objects, allocator
    del first
    ts = {'host': [], 'device': []}
    for _ in range(rounds):
        got = {}
        for where in ('host', 'device'):
            before = dict(textio.scan_counts)
            t0 = time.perf_counter(); got[where] = textio.read_matrix(path, where=where); sync(); ts[where].append(time.perf_counter() - t0)
            assert textio.scan_counts[where] == before[where] + 1
        assert got['host'].shape == got['device'].shape == m.shape and got['host'].tobytes() == got['device'].tobytes()
    phases = {}
    t = textio.read_matrix_device(path, timing=phases)
    sync(); t0 = time.perf_counter(); t.cpu().numpy(); phases['download'] = time.perf_counter() - t0
    host, dev = float(np.median(ts['host'])), float(np.median(ts['device']))
    print('%-22s %7d x %3d  %9.3f MB  host %8.4f s (%6.1f MB/s)  device %8.4f s  %5.1fx   upload %.4f kernels %.4f patch %.4f download %.4f'
          % (name, m.shape[0], m.shape[1], size / 1e6, host, size / host / 1e6, dev, host / dev, phases.get('upload', 0.0), phases.get('kernels', 0.0),
             phases.get('patch', 0.0), phases['download']), flush=True)
    os.remove(path)
    return size, host, dev


print('read_matrix from text, medians of %d alternated calls, arrays byte-equal; phases of one more device read' % rounds, flush=True)
for rows in (10380, 69878, 480189):
    leg('model-like', model_like(max(int(rows * scale), 1)), rounds)
leg('random bit patterns', bit_patterns(max(int(69878 * scale), 1)), rounds)
cross = None
for rows in (16, 64, 256, 1024, 4096, 16384, 65536):
    size, host, dev = leg('sweep', model_like(rows), max(rounds, 5))
    if cross is None and dev < host:
        cross = size
print('crossover: the device is first ahead at %s bytes of text; MATRIX_DEVICE_FROM is %d' % (cross, textio.MATRIX_DEVICE_FROM))
shutil.rmtree(d)
