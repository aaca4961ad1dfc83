"""Bulk readers/writers of the reference's text formats on top of the native parsers of libtkr_hip.so
(csrc/textio.hip on the host; csrc/parse_dev.hip, csrc/scan_dev.hip and csrc/format_dev.hip on the GPU).

    IdMap(dict)                       the reference's token -> index dict, handed to the parser
    parse_ratings(path, users, items, where=None)
                                      "uid,iid:like,..." lines -> flat arrays (Ratings)   (+ stamped .csr.npz copy)
    parse_ratings_device(path, users, items, device=None, chunk_bytes=None)
                                      the same arrays parsed by HIP kernels, left on the device (RatingsDevice)
    read_matrix(path, where=None)     '%f ' text matrix -> fp32 [lines, cols]   (+ stamped .npy copy)
    read_matrix_device(path, device=None, chunk_bytes=None)
                                      the same array read by HIP kernels, left on the device
    parse_ratings_for_group(path, users, items, where)
                                      the arrays of parse_ratings where the grouping (K15) wants them: host or device
    write_matrix(path, array, where=None)
                                      fp32 array -> '%f ' text, byte-identical to utils.py:47-55
    write_lists(path, users, ids, scores, row_user, items, where=None, block_bytes=None, append=False)
                                      top-k lists -> "uid,iid:%f,iid:%f,..." lines, the bytes of format_lines
    format_lists_device(ids, scores, row_user, users, items)
                                      the same text formatted by HIP kernels, left on the device with its line offsets

The text files stay authoritative.  ``read_matrix`` keeps a binary copy ``<path>.npy`` of what
it parsed and ``parse_ratings`` a copy ``<path>.csr.npz`` of its flat arrays (n1).  A copy is used
only when TKR_NO_CACHE is unset and the STAMP stored inside it -- byte size and mtime_ns of the
text file it was made from (ratings: also a digest of the two id tables) -- equals the text file's
current one; anything else (an older or newer text, a copy made with ``cp -p``, a coarse-mtime file
system, other id lists) is a miss and the text is parsed again.  ``write_matrix`` refreshes the copy
by parsing back the text it just wrote, so a cached read returns exactly what a fresh parse would.

Which parser reads a ratings file (``where`` / TKR_PARSE): 'host' -- one thread over the mapped file, needs no GPU; 'device' --
the file's bytes are copied to the GPU and parsed there (K11), the four arrays come back in one copy; 'auto' (the default) -- the
device for files of at least TKR_PARSE_DEVICE_FROM bytes when a GPU is visible and the text fits beside its outputs, else the host.
Both produce the same arrays bit for bit and raise for the same files.

Which reader reads a matrix (``where`` / TKR_MATRIX): 'host' -- tkr_matrix_read, one thread over the mapped file, needs no GPU;
'device' -- the file's bytes are copied to the GPU (K14, csrc/scan_dev.hip), which checks that the text has the canonical layout
("%f %f ... %f \\n" lines: no \\t \\r \\v \\f, no empty token, no blank line, equal token counts) and converts every plain decimal
token exactly; the tokens it cannot (exponent forms, inf, nan, more than 19 digits) are parsed by the host reader's own strtod
check from the mapped file and patched in.  A file in any other layout is read by the host reader as a whole, so both readers
return the same array bit for bit and raise TextFormatError for the same files.  'auto' (the default) -- the device for files of
at least TKR_MATRIX_DEVICE_FROM bytes when a GPU is visible and the text fits beside its outputs, else the host.

Which code groups parsed arrays into CSR rows (``where`` / TKR_GROUP; evaluate.load_scenario, recommend.rank, recommend.candidate_lines):
'host' -- numpy (evaluate._group), needs no GPU; 'device' -- K15 (csrc/group_dev.hip, tkr_hip.group_segments): the arrays K11 left on
the GPU, or the uploaded arrays of a stamped copy, are grouped there and the CSRs go to the kernels that read them without a download;
'auto' (the default) -- the device from TKR_GROUP_DEVICE_FROM parsed entries upward when a GPU is visible, the arrays fit and a row's
bitmap of columns fits LDS (tkr_hip.GROUP_MAX_COLS), else the host.  Both build the same arrays and raise the same errors;
``group_counts`` tells which ran.

Which writer formats a matrix or the lists (``where`` / TKR_FORMAT): 'host' -- tkr_matrix_write / format_lines, needs no GPU; 'device'
-- the text is formatted on the GPU (K13, csrc/format_dev.hip) in blocks of at most ``block_bytes``, each downloaded and appended to
the file; 'auto' (the default) -- the device from TKR_FORMAT_DEVICE_FROM fields (list entries, matrix elements) upward when a GPU is
visible, else the host.  Both write the same bytes.
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np
import torch

import tkr_hip


class TextFormatError(ValueError):
    """a line the reference itself would raise on (field without ':', non-integer like, ragged matrix row)"""


def _check(rc, what, path=None):
    if rc == 0:
        return
    if rc == -3:
        raise OSError('%s: cannot open %s' % (what, path))
    if rc == -4:
        raise TextFormatError('%s: malformed line in %s' % (what, path))
    raise tkr_hip.TkrError('%s failed: %d' % (what, rc))


class IdMap:
    """native token -> index table built from a reference-style dict (keys: str without newline)"""

    def __init__(self, table: dict):
        keys = list(table.keys())
        if any((not isinstance(t, str)) or ('\n' in t) for t in keys):
            raise TextFormatError('id tokens must be strings without newlines')
        blob = '\n'.join(keys).encode()
        index = np.fromiter(table.values(), dtype=np.int32, count=len(keys))
        import zlib
        self.digest = '%08x%08x%d' % (zlib.crc32(blob), zlib.crc32(index.tobytes()), len(keys))     # of tokens AND indices
        self._h = C.c_void_p()
        _check(tkr_hip.lib().tkr_idmap_create(blob, C.c_int64(len(blob)), index.ctypes.data_as(C.c_void_p),
                                              C.c_int64(len(keys)), C.byref(self._h)), 'tkr_idmap_create')
        self.size = len(keys)
        self._blob, self._index, self._dev, self._dev_tokens, self._by_index = blob, index, {}, {}, None

    def device_table(self, device):
        """-> (slots int32 [n_slots, 4], blob uint8, blob_len) on `device`: the open-addressing table K11 probes, laid out on the host
        once (tkr_idtable_build) and kept per device"""
        device = torch.device(device)
        if device not in self._dev:
            slots = torch.from_numpy(tkr_hip.idtable_build(self._blob, self._index)).to(device)
            blob = np.zeros(max(len(self._blob), 4), dtype=np.uint8)          # never an empty allocation: the only token may be ''
            blob[:len(self._blob)] = np.frombuffer(self._blob, dtype=np.uint8)
            self._dev[device] = (slots, torch.from_numpy(blob).to(device), len(self._blob))
        return self._dev[device]

    def tokens_by_index(self):
        """-> {index: token}, the later token where two share an index (the reference's own inversion of its dict)"""
        if self._by_index is None:
            self._by_index = {int(i): t for t, i in zip(self._blob.decode().split('\n'), self._index)}
        return self._by_index

    def device_tokens(self, device):
        """-> (blob uint8, blob_len, start int64 [n], length int32 [n]) on `device`, n = the largest index + 1: token i is
        blob[start[i], start[i] + length[i]), length[i] = -1 where no token has index i (a negative index is left out; of two tokens
        with one index the later wins).  What K13 writes ids with; laid out on the host once and kept per device"""
        device = torch.device(device)
        if device not in self._dev_tokens:
            n = len(self._index)
            raw = np.frombuffer(self._blob, dtype=np.uint8)
            ends = np.append(np.flatnonzero(raw == 10), len(raw))[:n].astype(np.int64)      # n tokens, n - 1 separators
            starts = np.append(0, ends[:-1] + 1)[:n].astype(np.int64)
            keep = self._index >= 0
            size = int(self._index[keep].max()) + 1 if keep.any() else 0
            start, length = np.zeros(size, dtype=np.int64), np.full(size, -1, dtype=np.int32)
            start[self._index[keep]] = starts[keep]
            length[self._index[keep]] = (ends - starts)[keep]
            blob = np.zeros(max(len(raw), 4), dtype=np.uint8)
            blob[:len(raw)] = raw
            self._dev_tokens[device] = (torch.from_numpy(blob).to(device), len(raw), torch.from_numpy(start).to(device),
                                        torch.from_numpy(length).to(device))
        return self._dev_tokens[device]

    def __del__(self):
        if getattr(self, '_h', None) and getattr(tkr_hip, 'lib', None) is not None:      # (module globals are gone at interpreter shutdown)
            tkr_hip.lib().tkr_idmap_destroy(self._h)
            self._h = None


class Ratings:
    """one record per line of a ratings file: ``line_user`` [n_lines] (index or -1), ``line_ptr`` [n_lines+1],
    per entry ``item`` (index or -1) and ``like`` (int)"""

    def __init__(self, line_user, line_ptr, item, like):
        self.line_user, self.line_ptr, self.item, self.like = line_user, line_ptr, item, like

    @property
    def entry_line(self):
        return np.repeat(np.arange(len(self.line_user), dtype=np.int64), np.diff(self.line_ptr))

    @property
    def entry_user(self):
        return np.repeat(self.line_user, np.diff(self.line_ptr))


def _stamp(path, extra=''):
    st = os.stat(path)
    return '%d:%d:%s' % (st.st_size, st.st_mtime_ns, extra)


class RatingsDevice:
    """``Ratings`` with its four arrays as torch tensors on the device that parsed them"""

    def __init__(self, line_user, line_ptr, item, like):
        self.line_user, self.line_ptr, self.item, self.like = line_user, line_ptr, item, like

    def host(self) -> Ratings:
        return Ratings(*(t.cpu().numpy() for t in (self.line_user, self.line_ptr, self.item, self.like)))


class DeviceParseTooLarge(tkr_hip.TkrError):
    """the text, its outputs and the scratch of K11 do not fit the free memory of the device ('auto' then parses on the host)"""


PARSE_WHERE = ('host', 'device', 'auto')
PARSE_DEFAULT = 'auto'
PARSE_DEVICE_FROM = 64 << 20         # bytes: 'auto' parses smaller files on the host (TKR_PARSE_DEVICE_FROM; DESIGN.md §7 has the crossover)
PARSE_CHUNK_BYTES = 16384            # the piece of text one wave counts and walks (any power of two 64 ... 2^20 gives the same arrays)
parse_counts = {'host': 0, 'device': 0}      # parses from text per parser in this process (what 'auto' chose is read off here)


def _parse_where(where):
    where = os.environ.get('TKR_PARSE', '') or PARSE_DEFAULT if where is None else where
    if where not in PARSE_WHERE:
        raise ValueError('where / TKR_PARSE must be one of %s, got %r' % (', '.join(PARSE_WHERE), where))
    return where


def _device_from():
    return int(os.environ.get('TKR_PARSE_DEVICE_FROM', '') or PARSE_DEVICE_FROM)


def _cached_ratings(path, users, items):
    """-> (the stamp the text carries now, or None when copies are off; the arrays of its valid stamped copy, or None)"""
    cache = path + '.csr.npz'
    stamp = _stamp(path, users.digest + '/' + items.digest) if _cache_enabled() else None
    if stamp is not None and os.path.isfile(cache):
        try:
            with np.load(cache, allow_pickle=False) as z:
                if str(z['stamp']) == stamp:
                    return stamp, Ratings(z['line_user'], z['line_ptr'], z['item'], z['like'])
        except (OSError, ValueError, KeyError):
            pass
    return stamp, None


def parse_ratings(path: str, users, items, where=None) -> Ratings:
    where = _parse_where(where)
    users = users if isinstance(users, IdMap) else IdMap(users)
    items = items if isinstance(items, IdMap) else IdMap(items)
    cache = path + '.csr.npz'
    stamp, cached = _cached_ratings(path, users, items)
    if cached is not None:
        return cached
    out = None
    if where == 'device' or (where == 'auto' and torch.cuda.is_available() and os.path.getsize(path) >= _device_from()):
        try:
            out = _parse_ratings_device(path, users, items).host()
        except DeviceParseTooLarge:
            if where == 'device':
                raise
    if out is None:
        out = _parse_ratings(path, users, items)
    # the copy is stored under the stamp taken BEFORE the parse, and only if the file still carries it afterwards (a text rewritten
    # in between would otherwise get a copy of the old contents under the new stamp: ADVICE r2); one writer per launch
    if stamp is not None and _cache_writer() and _stamp(path, users.digest + '/' + items.digest) == stamp:
        try:
            tmp = cache + '.tmp.%d.npz' % os.getpid()
            np.savez(tmp, stamp=np.array(stamp), line_user=out.line_user, line_ptr=out.line_ptr, item=out.item, like=out.like)
            os.replace(tmp, cache)
        except OSError:
            pass                               # read-only data directory: the text stays the only copy
    return out


def parse_ratings_device(path: str, users, items, device=None, chunk_bytes=None) -> RatingsDevice:
    """the arrays of parse_ratings, parsed on `device` (default: the current GPU) and left there; no stamped copy is read or written"""
    users = users if isinstance(users, IdMap) else IdMap(users)
    items = items if isinstance(items, IdMap) else IdMap(items)
    return _parse_ratings_device(path, users, items, device, chunk_bytes)


def _fits(need, device, what, path):
    """K11 keeps the text beside everything it writes: raise unless `need` more bytes fit the device's free memory"""
    free = torch.cuda.mem_get_info(device)[0]
    if need > free:
        raise DeviceParseTooLarge('%s: %s needs %d bytes of device memory, %d are free' % (path, what, need, free))


def _parse_ratings_device(path, users, items, device=None, chunk_bytes=None) -> RatingsDevice:
    if not torch.cuda.is_available():
        raise tkr_hip.TkrError('parse_ratings on the device runs through libtkr_hip.so; no MI355X is visible')
    chunk_bytes = PARSE_CHUNK_BYTES if chunk_bytes is None else chunk_bytes
    # a missing file is an OSError before anything is uploaded; an empty one cannot be mapped
    host = np.memmap(path, dtype=np.uint8, mode='c') if os.stat(path).st_size else np.empty(0, dtype=np.uint8)
    n_bytes = int(host.size)
    need_ws = tkr_hip.parse_dev_workspace_bytes(n_bytes, chunk_bytes)
    device = torch.device('cuda', torch.cuda.current_device()) if device is None else torch.device(device)
    # the limit: text + workspace, then 12 bytes per entry and 20 per line beside them, must fit the free device memory
    _fits(n_bytes + need_ws, device, 'the text', path)
    text = torch.from_numpy(host).to(device)                       # mapped, copied once
    del host
    ws = torch.empty(need_ws, dtype=torch.uint8, device=device)
    totals = torch.empty(2, dtype=torch.int64, device=device)
    tkr_hip.ratings_count_dev(text, chunk_bytes, ws, totals)
    n_lines, n_entries = totals.tolist()                           # the one round trip: the outputs are sized by it
    _fits(12 * n_entries + 20 * n_lines + 64, device, 'the parsed arrays', path)
    status = torch.empty(1, dtype=torch.int64, device=device)
    out = tkr_hip.ratings_emit_dev(text, chunk_bytes, ws, n_lines, n_entries, users.device_table(device), items.device_table(device), status)
    if int(status.item()) != -1:
        _check(-4, 'tkr_ratings_emit_dev', path)
    parse_counts['device'] += 1
    return RatingsDevice(*out)


def _parse_ratings(path, users, items) -> Ratings:
    parse_counts['host'] += 1
    lib = tkr_hip.lib()
    h = C.c_void_p()
    _check(lib.tkr_ratings_parse(os.fsencode(path), users._h, items._h, C.byref(h)), 'tkr_ratings_parse', path)
    try:
        n_lines, n_entries = C.c_int64(), C.c_int64()
        _check(lib.tkr_ratings_sizes(h, C.byref(n_lines), C.byref(n_entries)), 'tkr_ratings_sizes')
        line_user = np.empty(n_lines.value, dtype=np.int32)
        line_ptr = np.empty(n_lines.value + 1, dtype=np.int64)
        item = np.empty(n_entries.value, dtype=np.int32)
        like = np.empty(n_entries.value, dtype=np.int32)
        _check(lib.tkr_ratings_copy(h, *(a.ctypes.data_as(C.c_void_p) for a in (line_user, line_ptr, item, like))),
               'tkr_ratings_copy')
    finally:
        lib.tkr_ratings_destroy(h)
    return Ratings(line_user, line_ptr, item, like)


# ---- K15: where the parsed arrays are grouped into CSRs (evaluate.load_scenario, recommend.rank / candidate_lines) --------------------
DeviceGroupTooLarge = tkr_hip.DeviceGroupTooLarge
GROUP_WHERE = ('host', 'device', 'auto')
GROUP_DEFAULT = 'auto'
GROUP_DEVICE_FROM = 262144           # entries: 'auto' groups fewer on the host (TKR_GROUP_DEVICE_FROM; DESIGN.md §4 K15 has the sweep)
group_counts = {'host': 0, 'device': 0}      # scenarios / rated sets / candidate files grouped per path in this process (what 'auto' chose)


def _group_where(where):
    where = os.environ.get('TKR_GROUP', '') or GROUP_DEFAULT if where is None else where
    if where not in GROUP_WHERE:
        raise ValueError('where / TKR_GROUP must be one of %s, got %r' % (', '.join(GROUP_WHERE), where))
    return where


def _group_device_from():
    return int(os.environ.get('TKR_GROUP_DEVICE_FROM', '') or GROUP_DEVICE_FROM)


def group_on_device(where, n_entries, n_cols):
    """whether K15 groups `n_entries` parsed entries over `n_cols` columns: 'device' -- yes, and without a GPU that raises; 'auto' -- with
    a GPU, from TKR_GROUP_DEVICE_FROM entries upward, while a row's bitmap fits (tkr_hip.GROUP_MAX_COLS); 'host' -- no"""
    if where == 'device' and not torch.cuda.is_available():
        raise tkr_hip.TkrError('grouping on the device runs through libtkr_hip.so; no MI355X is visible')
    return where == 'device' or (where == 'auto' and torch.cuda.is_available() and n_entries >= _group_device_from()
                                 and n_cols <= tkr_hip.GROUP_MAX_COLS)


def group_fits(need, device, what):
    """K15 keeps the parsed arrays beside the CSRs it writes: raise DeviceGroupTooLarge unless `need` more bytes fit"""
    free = torch.cuda.mem_get_info(device)[0]
    if need > free:
        raise DeviceGroupTooLarge('%s needs %d bytes of device memory, %d are free' % (what, need, free))


def n_entries_of(R):
    return int(R.item.numel()) if isinstance(R, RatingsDevice) else int(len(R.item))


def ratings_to_device(R, device=None) -> RatingsDevice:
    """a Ratings uploaded (a RatingsDevice is returned as it is)"""
    if isinstance(R, RatingsDevice):
        return R
    device = torch.device('cuda', torch.cuda.current_device()) if device is None else torch.device(device)
    group_fits(12 * len(R.item) + 20 * len(R.line_user) + 64, device, 'the parsed arrays')
    return RatingsDevice(*(torch.from_numpy(np.ascontiguousarray(a)).to(device) for a in (R.line_user, R.line_ptr, R.item, R.like)))


def ratings_to_host(R) -> Ratings:
    return R.host() if isinstance(R, RatingsDevice) else R


def parse_ratings_for_group(path: str, users, items, where):
    """the arrays of parse_ratings where the grouping wants them -> Ratings or RatingsDevice.  A valid stamped copy is answered from the
    host as always; otherwise, when K11 parses the file (TKR_PARSE 'device', or 'auto' and a file of TKR_PARSE_DEVICE_FROM bytes -- under
    where='device' any file), its arrays stay on the device and no copy is written; everything else is parse_ratings itself"""
    users = users if isinstance(users, IdMap) else IdMap(users)
    items = items if isinstance(items, IdMap) else IdMap(items)
    if where != 'host' and torch.cuda.is_available() and _cached_ratings(path, users, items)[1] is None:
        parser = _parse_where(None)
        if parser == 'device' or (parser == 'auto' and (where == 'device' or os.path.getsize(path) >= _device_from())):
            try:
                return _parse_ratings_device(path, users, items)
            except DeviceParseTooLarge:
                if parser == 'device':
                    raise
    return parse_ratings(path, users, items)


def _parse_matrix(path):
    lib = tkr_hip.lib()
    h = C.c_void_p()
    _check(lib.tkr_matrix_read(os.fsencode(path), C.byref(h)), 'tkr_matrix_read', path)
    try:
        rows, cols = C.c_int64(), C.c_int64()
        _check(lib.tkr_matrix_sizes(h, C.byref(rows), C.byref(cols)), 'tkr_matrix_sizes')
        out = np.empty((rows.value, cols.value), dtype=np.float32)
        _check(lib.tkr_matrix_copy(h, out.ctypes.data_as(C.c_void_p)), 'tkr_matrix_copy')
    finally:
        lib.tkr_matrix_destroy(h)
    return out


def _cache_path(path):
    return path + '.npy'


def _cache_enabled():
    return os.environ.get('TKR_NO_CACHE', '') in ('', '0')


def _cache_writer():
    """under a torch.distributed launcher every rank parses the same files: rank 0 alone writes the copies"""
    return os.environ.get('RANK', '0') == '0'


class MatrixNotCanonical(TextFormatError):
    """the text does not have the layout K14 reads on the device (read_matrix then hands the whole file to the host reader, which
    returns the array or raises its own TextFormatError); ``offset`` is the first byte that breaks a rule"""

    def __init__(self, path, offset):
        super().__init__('%s: not the canonical layout of a \'%%f \' matrix at byte %d' % (path, offset))
        self.offset = offset


MATRIX_WHERE = ('host', 'device', 'auto')
MATRIX_DEFAULT = 'auto'
MATRIX_DEVICE_FROM = 1 << 20         # bytes of text: 'auto' reads smaller files on the host (TKR_MATRIX_DEVICE_FROM; DESIGN.md §4 K14 has the sweep)
MATRIX_CHUNK_BYTES = 16384           # the piece of text one wave counts and walks (any power of two 64 ... 2^20 gives the same array)
scan_counts = {'host': 0, 'device': 0}       # matrices read from text per reader in this process (what 'auto' chose is read off here)


def _matrix_where(where):
    where = os.environ.get('TKR_MATRIX', '') or MATRIX_DEFAULT if where is None else where
    if where not in MATRIX_WHERE:
        raise ValueError('where / TKR_MATRIX must be one of %s, got %r' % (', '.join(MATRIX_WHERE), where))
    return where


def _matrix_device_from():
    return int(os.environ.get('TKR_MATRIX_DEVICE_FROM', '') or MATRIX_DEVICE_FROM)


def _first_line_cols(host):
    """the token count of the first line of the mapped text, as the host reader counts it"""
    end, step = 0, 1 << 16
    while True:
        hit = np.flatnonzero(host[end:end + step] == 10)
        if hit.size:
            end += int(hit[0])
            break
        end += step
        if end >= host.size:
            end = int(host.size)
            break
    line = bytes(host[:end]).strip(b' \t\n\r\v\f')
    return len(line.split(b' ')) if line else 0


def _read_matrix_device(path, device=None, chunk_bytes=None, timing=None):
    """K14 -> fp32 [rows, cols] on the device.  timing: a dict that receives the seconds of 'upload', 'kernels' (with the two
    read-backs of a few words), 'patch' (the hard tokens: their offsets down, the host's strtod, their values up)"""
    if not torch.cuda.is_available():
        raise tkr_hip.TkrError('read_matrix on the device runs through libtkr_hip.so; no MI355X is visible')
    import time
    chunk_bytes = MATRIX_CHUNK_BYTES if chunk_bytes is None else chunk_bytes
    host = np.memmap(path, dtype=np.uint8, mode='c') if os.stat(path).st_size else np.empty(0, dtype=np.uint8)
    n_bytes = int(host.size)
    need_ws = tkr_hip.scan_dev_workspace_bytes(n_bytes, chunk_bytes)
    device = torch.device('cuda', torch.cuda.current_device()) if device is None else torch.device(device)

    def lap(name, since):
        if timing is not None:
            torch.cuda.synchronize(device)
            timing[name] = timing.get(name, 0.0) + time.perf_counter() - since
        return time.perf_counter()

    # the limit: text + workspace, then 12 bytes and a bit per token beside them, must fit the free device memory
    _fits(n_bytes + need_ws, device, 'the text', path)
    t0 = time.perf_counter()
    text = torch.from_numpy(host).to(device)                       # mapped, copied once
    t0 = lap('upload', t0)
    ws = torch.empty(need_ws, dtype=torch.uint8, device=device)
    totals = torch.empty(3, dtype=torch.int64, device=device)
    tkr_hip.matrix_count_dev(text, chunk_bytes, ws, totals)
    n_lines, n_tokens, status = totals.tolist()                    # the one round trip: the outputs are sized by it
    if status != -1:
        raise MatrixNotCanonical(path, status)
    cols = _first_line_cols(host)
    _fits(12 * n_tokens + n_tokens // 8 + 64, device, 'the parsed array', path)
    tok_start, data, hard, counts = tkr_hip.matrix_emit_dev(text, chunk_bytes, ws, n_lines, n_tokens, cols)
    status, n_hard = counts.tolist()
    if status != -1:
        raise MatrixNotCanonical(path, status)
    t0 = lap('kernels', t0)
    if n_hard:
        bits = np.unpackbits(hard.cpu().numpy().view(np.uint8), bitorder='little')[:n_tokens]
        index = torch.from_numpy(np.flatnonzero(bits)).to(device)
        rc, values = tkr_hip.matrix_tokens_host(host, tok_start[index].cpu().numpy())
        _check(rc, 'tkr_matrix_tokens_host', path)
        data[index] = torch.from_numpy(values).to(device)
        lap('patch', t0)
    return data.view(n_lines, cols)


def read_matrix_device(path: str, device=None, chunk_bytes=None, timing=None) -> torch.Tensor:
    """the array of read_matrix, read on `device` (default: the current GPU) by K14 and left there, the tokens the device leaves to
    the host's strtod already patched in; no stamped copy is read or written.  A text that is not in the canonical layout raises
    MatrixNotCanonical, a token that is no number TextFormatError"""
    out = _read_matrix_device(path, device, chunk_bytes, timing)
    scan_counts['device'] += 1
    return out


def read_matrix(path: str, where=None) -> np.ndarray:
    """every line of a '%f ' text matrix -> fp32 [n_lines, n_cols]; see the module text for `where`"""
    where = _matrix_where(where)
    cache = _cache_path(path)
    if _cache_enabled() and os.path.isfile(cache) and os.path.isfile(cache + '.stamp'):
        try:
            if open(cache + '.stamp').read() == _stamp(path):
                got = np.load(cache)
                if got.dtype == np.float32 and got.ndim == 2:
                    return got
        except (OSError, ValueError):
            pass
    stamp = _stamp(path) if _cache_enabled() else None
    out = None
    if where == 'device' or (where == 'auto' and torch.cuda.is_available() and os.path.getsize(path) >= _matrix_device_from()):
        try:
            out = _read_matrix_device(path).cpu().numpy()
            scan_counts['device'] += 1
        except (MatrixNotCanonical, DeviceParseTooLarge):
            pass                               # the host reader takes the whole file: it returns the array or raises as it always did
    if out is None:
        out = _parse_matrix(path)
        scan_counts['host'] += 1
    _store_cache(path, out, stamp)
    return out


def _store_cache(path, parsed, stamp):
    """binary copy + the stamp (size, mtime_ns) the text carried BEFORE it was parsed -- stored only if it still carries it;
    the stamp file goes last, so a torn pair is a miss"""
    if not _cache_enabled() or not _cache_writer():
        return
    try:
        if stamp is None or _stamp(path) != stamp:
            return
        if os.path.exists(_cache_path(path) + '.stamp'):
            os.remove(_cache_path(path) + '.stamp')
        tmp = _cache_path(path) + '.tmp.%d' % os.getpid()
        with open(tmp, 'wb') as fh:
            np.save(fh, parsed)
        os.replace(tmp, _cache_path(path))
        with open(tmp, 'w') as fh:
            fh.write(stamp)
        os.replace(tmp, _cache_path(path) + '.stamp')
    except OSError:
        pass                                   # read-only data directory: the text stays the only copy


FORMAT_WHERE = ('host', 'device', 'auto')
FORMAT_DEFAULT = 'auto'
FORMAT_DEVICE_FROM = 65536           # fields: 'auto' formats fewer on the host (TKR_FORMAT_DEVICE_FROM; DESIGN.md §4 K13 has the crossover)
FORMAT_BLOCK_BYTES = 256 << 20       # text formatted, downloaded and written at a time (any value from the longest line up gives the same file)
format_counts = {'host': 0, 'device': 0}     # files (or appended parts) written per writer in this process


def _format_where(where):
    where = os.environ.get('TKR_FORMAT', '') or FORMAT_DEFAULT if where is None else where
    if where not in FORMAT_WHERE:
        raise ValueError('where / TKR_FORMAT must be one of %s, got %r' % (', '.join(FORMAT_WHERE), where))
    return where


def _format_on_device(where, n_fields):
    """'device', or 'auto' with a GPU and enough fields; 'device' without a GPU raises"""
    if where == 'device' and not torch.cuda.is_available():
        raise tkr_hip.TkrError('formatting on the device runs through libtkr_hip.so; no MI355X is visible')
    from_fields = int(os.environ.get('TKR_FORMAT_DEVICE_FROM', '') or FORMAT_DEVICE_FROM)
    return where == 'device' or (where == 'auto' and torch.cuda.is_available() and n_fields >= from_fields)


def format_lines(users, ids, scores, items):
    """users: n tokens; ids int [n, K] catalogue indices, -1 = no item; scores float [n, K]; items: index -> token
    -> n lines 'uid,iid:%f,iid:%f,...'"""
    out = []
    for u, row_i, row_s in zip(users, np.asarray(ids), np.asarray(scores)):
        out.append(','.join([u] + ['%s:%f' % (items[int(c)], float(s)) for c, s in zip(row_i, row_s) if c >= 0]))
    return out


def _host_array(x, dtype):
    return np.ascontiguousarray(x.detach().cpu().numpy() if isinstance(x, torch.Tensor) else x, dtype=dtype)


def _device_array(x, dtype, device):
    if isinstance(x, torch.Tensor):
        return x.detach().to(device=device, dtype=dtype).contiguous()
    return torch.from_numpy(np.ascontiguousarray(x, dtype={torch.int32: np.int32, torch.float32: np.float32}[dtype])).to(device)


def _format_device_of(*arrays):
    for x in arrays:
        if isinstance(x, torch.Tensor) and x.is_cuda:
            return x.device
    return torch.device('cuda', torch.cuda.current_device())


class _Timer:
    """device time of the kernels between start() and stop() (events, read at the end), host time of the download and the file
    write, summed into the caller's dict"""

    def __init__(self, into):
        self.into, self.pairs = into, []

    def kernels(self):
        if self.into is None:
            return None
        pair = (torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
        self.pairs.append(pair)
        pair[0].record()
        return pair[1]

    def host(self, name, since):
        if self.into is not None:
            import time
            self.into[name] = self.into.get(name, 0.0) + time.perf_counter() - since

    def close(self):
        if self.into is not None:
            torch.cuda.synchronize()
            self.into['kernels'] = self.into.get('kernels', 0.0) + sum(a.elapsed_time(b) for a, b in self.pairs) * 1e-3


def _emit_blocks(path, append, line_ptr, totals, emit, block_bytes, what, timing=None):
    """the second half of K13 for a whole file: read back the line offsets (the one round trip between the two calls), cut the rows into
    blocks of at most block_bytes of text, format each into one device buffer, download it and append it to the file -> bytes written"""
    import time
    timer = _Timer(timing)
    t0 = time.perf_counter()
    host = torch.cat([line_ptr, totals]).cpu().numpy()
    timer.host('download', t0)
    lp = host[:-2]
    total = tkr_hip.format_totals(host[-2:], what)
    n = len(lp) - 1
    longest = int(np.diff(lp).max()) if n else 0
    device = line_ptr.device
    if block_bytes is None:
        block_bytes = max(min(FORMAT_BLOCK_BYTES, torch.cuda.mem_get_info(device)[0] // 2), longest)
    if block_bytes < longest:
        raise ValueError('%s: block_bytes must be at least %d, the longest line (got %d)' % (path, longest, block_bytes))
    _fits(min(block_bytes, total) + 64, device, 'a block of the text', path)
    buf = torch.empty(min(block_bytes, total), dtype=torch.uint8, device=device)
    with open(path, 'ab' if append else 'wb') as fh:
        first = 0
        while first < n:
            last = int(np.searchsorted(lp, lp[first] + block_bytes, side='right')) - 1      # the rows [first, last) fit
            size = int(lp[last] - lp[first])
            done = timer.kernels()
            status = emit(first, last - first, buf)
            if done is not None:
                done.record()
            t0 = time.perf_counter()
            text = buf[:size].cpu().numpy()
            tkr_hip.format_emit_check(status, what)
            timer.host('download', t0)
            t0 = time.perf_counter()
            fh.write(memoryview(text))
            timer.host('write', t0)
            first = last
    timer.close()
    return total


def format_lists_device(ids, scores, row_user, users: IdMap, items: IdMap):
    """-> (text uint8 [bytes], line_ptr int64 [n + 1]) on the device: the lines of format_lines for the rows of ids / scores [n, K]
    (negative id = no entry), row r under token row_user[r] of `users`, the items under their tokens of `items`, each with its '\n';
    line r is text[line_ptr[r] : line_ptr[r + 1]].  An index that names no token raises TkrError"""
    if not torch.cuda.is_available():
        raise tkr_hip.TkrError('formatting on the device runs through libtkr_hip.so; no MI355X is visible')
    device = _format_device_of(ids, scores, row_user)
    ids, scores, row_user = _device_array(ids, torch.int32, device), _device_array(scores, torch.float32, device), _device_array(row_user, torch.int32, device)
    if ids.dim() != 2 or ids.shape != scores.shape or row_user.numel() != ids.shape[0]:
        raise ValueError('ids and scores [n, K] and row_user [n] required')
    args = (ids, scores, row_user.reshape(-1), users.device_tokens(device), items.device_tokens(device))
    line_ptr, totals = tkr_hip.lists_format_sizes(*args)
    total = tkr_hip.format_totals(totals.tolist(), 'tkr_lists_format_sizes_dev')       # the one round trip: the text is sized by it
    _fits(total + 64, device, 'the text', 'format_lists_device')
    text = torch.empty(total, dtype=torch.uint8, device=device)
    tkr_hip.format_emit_check(tkr_hip.lists_format_emit(*args, line_ptr, 0, ids.shape[0], text), 'tkr_lists_format_emit_dev')
    return text, line_ptr


def write_lists(path, users: IdMap, ids, scores, row_user, items: IdMap, where=None, block_bytes=None, append=False, timing=None):
    """write (or append) the top-k lines of ids / scores [n, K] -> bytes written; row r is the list of user index row_user[r].
    The bytes are '\n'.join(format_lines(...)) + '\n' whichever writer runs; see the module text for `where`.  On the device the text is
    formatted in blocks of at most block_bytes (at least the longest line, else ValueError before anything is written)"""
    where = _format_where(where)
    shape = tuple(ids.shape)
    if len(shape) != 2 or shape != tuple(scores.shape) or len(row_user) != shape[0]:
        raise ValueError('ids and scores [n, K] and row_user [n] required')
    if _format_on_device(where, shape[0] * shape[1]):
        device = _format_device_of(ids, scores, row_user)
        try:
            args = (_device_array(ids, torch.int32, device), _device_array(scores, torch.float32, device),
                    _device_array(row_user, torch.int32, device).reshape(-1), users.device_tokens(device), items.device_tokens(device))
            timer = _Timer(timing)
            done = timer.kernels()
            line_ptr, totals = tkr_hip.lists_format_sizes(*args)
            if done is not None:
                done.record()
            timer.close()
            size = _emit_blocks(path, append, line_ptr, totals, lambda first, count, out: tkr_hip.lists_format_emit(*args, line_ptr, first, count, out),
                                block_bytes, 'tkr_lists_format', timing)
            format_counts['device'] += 1
            return size
        except DeviceParseTooLarge:
            if where == 'device':
                raise
    utok, itok = users.tokens_by_index(), items.tokens_by_index()
    lines = format_lines([utok[int(u)] for u in _host_array(row_user, np.int64).reshape(-1)], _host_array(ids, np.int64), _host_array(scores, np.float32), itok)
    text = ('\n'.join(lines) + '\n').encode() if lines else b''
    with open(path, 'ab' if append else 'wb') as fh:
        fh.write(text)
    format_counts['host'] += 1
    return len(text)


def _write_matrix_device(path, array, block_bytes, timing):
    device = _format_device_of(array)
    data = _device_array(array, torch.float32, device)
    timer = _Timer(timing)
    done = timer.kernels()
    line_ptr, totals = tkr_hip.matrix_format_sizes(data)
    if done is not None:
        done.record()
    timer.close()
    return _emit_blocks(path, False, line_ptr, totals, lambda first, count, out: tkr_hip.matrix_format_emit(data, line_ptr, first, count, out),
                        block_bytes, 'tkr_matrix_format', timing)


def write_matrix(path: str, array, where=None, block_bytes=None, timing=None) -> None:
    where = _format_where(where)
    shape = tuple(array.shape) if hasattr(array, 'shape') else np.shape(array)
    if len(shape) != 2:
        raise ValueError('2-D array required')
    rows, cols = (int(v) for v in shape)
    written = False
    if _format_on_device(where, rows * cols):
        try:
            _write_matrix_device(path, array, block_bytes, timing)
            format_counts['device'] += 1
            written = True
        except DeviceParseTooLarge:
            if where == 'device':
                raise
    if not written:
        array = _host_array(array, np.float32)
        _check(tkr_hip.lib().tkr_matrix_write(os.fsencode(path), array.ctypes.data_as(C.c_void_p),
                                              C.c_int64(array.shape[0]), C.c_int64(array.shape[1])), 'tkr_matrix_write', path)
        format_counts['host'] += 1
    if _cache_enabled():
        stamp = _stamp(path)
        _store_cache(path, _parse_matrix(path), stamp)      # the 6-decimal text is authoritative: cache what IT says
