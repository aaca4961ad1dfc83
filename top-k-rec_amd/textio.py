"""Bulk readers/writers of the reference's text formats on top of the native parsers of libtkr_hip.so
(csrc/textio.hip on the host, csrc/parse_dev.hip on the GPU).

    IdMap(dict)                       the reference's token -> index dict, handed to the parser
    parse_ratings(path, users, items, where=None)
                                      "uid,iid:like,..." lines -> flat arrays (Ratings)   (+ stamped .csr.npz copy)
    parse_ratings_device(path, users, items, device=None, chunk_bytes=None)
                                      the same arrays parsed by HIP kernels, left on the device (RatingsDevice)
    read_matrix(path)                 '%f ' text matrix -> fp32 [lines, cols]   (+ stamped .npy copy)
    write_matrix(path, array)         fp32 array -> '%f ' text, byte-identical to utils.py:47-55

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
        self._blob, self._index, self._dev = blob, index, {}

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

    def __del__(self):
        if getattr(self, '_h', None) and tkr_hip is not None:      # (module globals are gone at interpreter shutdown)
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


def parse_ratings(path: str, users, items, where=None) -> Ratings:
    where = _parse_where(where)
    users = users if isinstance(users, IdMap) else IdMap(users)
    items = items if isinstance(items, IdMap) else IdMap(items)
    cache = path + '.csr.npz'
    stamp = _stamp(path, users.digest + '/' + items.digest) if _cache_enabled() else None
    if stamp is not None and os.path.isfile(cache):
        try:
            with np.load(cache, allow_pickle=False) as z:
                if str(z['stamp']) == stamp:
                    return Ratings(z['line_user'], z['line_ptr'], z['item'], z['like'])
        except (OSError, ValueError, KeyError):
            pass
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


def read_matrix(path: str) -> np.ndarray:
    """every line of a '%f ' text matrix -> fp32 [n_lines, n_cols]"""
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
    out = _parse_matrix(path)
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


def write_matrix(path: str, array) -> None:
    array = np.ascontiguousarray(array, dtype=np.float32)
    if array.ndim != 2:
        raise ValueError('2-D array required')
    _check(tkr_hip.lib().tkr_matrix_write(os.fsencode(path), array.ctypes.data_as(C.c_void_p),
                                          C.c_int64(array.shape[0]), C.c_int64(array.shape[1])), 'tkr_matrix_write', path)
    if _cache_enabled():
        stamp = _stamp(path)
        _store_cache(path, _parse_matrix(path), stamp)      # the 6-decimal text is authoritative: cache what IT says
