// K13: the text writers on the device -- the top-k lists of recommend.py ("uid,iid:%f,iid:%f,...") and the '%f ' matrices of
// tkr_matrix_write (csrc/textio.hip), byte for byte what glibc printf / Python's '%f' % float(x) give, from arrays in device memory.
//
//   sizes   one wave per row: every lane takes the length of one piece (a list entry, a matrix element) per round of 64, the wave
//           sums them -> line_ptr[row] = bytes of the row
//   scan    one workgroup: exclusive 64-bit prefix of the row lengths in place, line_ptr[n] = totals[0] = the bytes of the whole text
//                                                                                                              -> the host allocates
//   emit    one wave per row: a wave-wide prefix of the piece lengths gives every piece its offset; the lanes format into a window of
//           the row's text in LDS (kWindow bytes, its start a multiple of 16 in the output) and the wave copies every full window out
//           with 16-byte stores.  Only the two ends of a row, which share a 16-byte chunk with the neighbouring rows, go out as bytes.
//
// '%f' of an fp32 value with integers only (tests/_format_oracle.py is the same recipe in Python): x = +-m * 2^ex, m < 2^24.
//   ex >= 0          the integer m << ex, fraction 000000.  Up to ex = 40 it fits 64 bits; above (|x| >= 2^64) it is held in four
//                    32-bit limbs and divided by 10^9 five times: five chunks of nine decimal digits, 39 digits at most.
//   ex < 0, sh = -ex integer part m >> sh, fraction ((m mod 2^sh) * 10^6) >> sh (below 2^44), rounded half to even on the remainder;
//                    a fraction that reaches 10^6 carries into the integer part.  sh >= 64: 0.000000, never a tie.
//   a set sign bit prints '-' (also -0.000000 and what rounds to it), +-inf prints inf / -inf, every NaN prints nan.
// The longest text is 47 bytes: sign, 39 digits, '.', 6 digits.
//
// A list entry with a negative id is skipped wherever it stands.  A row_user or an id outside its token table, or one whose slot holds
// no token (length -1), or a token outside its blob, writes the row number to the status word (atomic min: the first row wins) and
// counts as empty in both passes, so the two passes agree and nothing is read or written out of bounds.  emit stores only inside
// [line_ptr[row], line_ptr[row + 1]) of the block it was handed, whatever the arrays hold.
#include "tkr_common.h"
#include "../../include/tkr.h"

namespace tkr {
namespace {

constexpr int kFmtBlock = 256;                                     // 4 waves = 4 rows per workgroup
constexpr int kFmtWaves = kFmtBlock / 64;
constexpr int kWindow = 2048;                                      // bytes of a row's text a wave stages at a time (a multiple of 1024)
constexpr int kFmtScanThreads = 1024;
constexpr int64_t kMaxBlob = (int64_t)1 << 29;                     // bytes of a token table: a piece's offsets stay 32-bit
constexpr unsigned kFmtMaxGrid = 1u << 16;                         // rows beyond 2^18 are taken by a grid-stride loop

// ---- '%f' ------------------------------------------------------------------------------------------------------------------------
enum : uint32_t { kSmall = 0, kBig = 1, kInf = 2, kNan = 3 };

struct Dec {                                                        // a decoded fp32
    uint64_t ip;                                                    // kSmall: the integer part after rounding; kBig: m
    uint32_t frac;                                                  // kSmall: the six fraction digits as a number; kBig: ex
    uint32_t kind, neg;
};

__host__ __device__ __forceinline__ Dec decode(uint32_t bits) {
    Dec d;
    const uint32_t e = (bits >> 23) & 0xffu, f = bits & 0x7fffffu;
    d.neg = bits >> 31;
    d.ip = 0;
    d.frac = 0;
    if (e == 255u) {
        d.kind = f ? kNan : kInf;
        return d;
    }
    const uint64_t m = e ? (f | 0x800000u) : f;
    const int ex = e ? (int)e - 150 : -149;
    d.kind = kSmall;
    if (ex >= 0) {
        if (ex <= 40) {
            d.ip = m << ex;
        } else {
            d.kind = kBig;
            d.ip = m;
            d.frac = (uint32_t)ex;
        }
        return d;
    }
    const int sh = -ex;
    if (sh >= 64) return d;                                         // below 2^-40: 0.000000
    const uint64_t mask = ((uint64_t)1 << sh) - 1;
    const uint64_t p = (m & mask) * 1000000u;                       // < 2^44
    const uint64_t r = p & mask, half = (uint64_t)1 << (sh - 1);
    uint32_t frac = (uint32_t)(p >> sh);
    uint64_t ip = m >> sh;
    if (r > half || (r == half && (frac & 1u))) ++frac;
    if (frac == 1000000u) {
        frac = 0;
        ++ip;
    }
    d.ip = ip;
    d.frac = frac;
    return d;
}

// the five 9-digit chunks of m << ex (41 <= ex <= 104), least significant first
struct Chunks { uint32_t c0, c1, c2, c3, c4; };

__host__ __device__ __forceinline__ uint32_t div1e9(uint32_t& limb, uint32_t rem) {
    const uint64_t cur = (uint64_t)rem << 32 | limb;
    const uint64_t q = cur / 1000000000u;                           // rem < 10^9: q < 2^32
    limb = (uint32_t)q;
    return (uint32_t)(cur - q * 1000000000u);
}

__host__ __device__ inline Chunks big_chunks(uint32_t m, uint32_t ex) {
    const uint32_t ws = ex >> 5, bs = ex & 31u;                     // ws = 1, 2, 3
    const uint64_t t = (uint64_t)m << bs;                           // < 2^55; ws == 3 has bs <= 8: t < 2^32
    const uint32_t lo = (uint32_t)t, hi = (uint32_t)(t >> 32);
    uint32_t l0 = 0, l1 = ws == 1 ? lo : 0u, l2 = ws == 1 ? hi : (ws == 2 ? lo : 0u), l3 = ws == 2 ? hi : (ws == 3 ? lo : 0u);
    auto step = [&]() { return div1e9(l0, div1e9(l1, div1e9(l2, div1e9(l3, 0u)))); };      // the limbs / 10^9 -> the remainder
    Chunks c;
    c.c0 = step();
    c.c1 = step();
    c.c2 = step();
    c.c3 = step();
    c.c4 = step();
    return c;
}

__host__ __device__ __forceinline__ int digits32(uint32_t v) {
    int n = 1;
    while (v >= 10u) {
        v /= 10u;
        ++n;
    }
    return n;
}

__host__ __device__ __forceinline__ int digits64(uint64_t v) {
    int n = 0;
    while (v >> 32) {                                               // at most twice
        v /= 100000u;
        n += 5;
    }
    return n + digits32((uint32_t)v);
}

__host__ __device__ __forceinline__ int big_digits(const Chunks& c) {        // m << ex >= 2^64: at least 20 digits
    if (c.c4) return 36 + digits32(c.c4);
    if (c.c3) return 27 + digits32(c.c3);
    return 18 + digits32(c.c2);
}

__host__ __device__ __forceinline__ int fmt_len(const Dec& d) {
    if (d.kind == kSmall) return (int)d.neg + digits64(d.ip) + 7;
    if (d.kind == kNan) return 3;
    if (d.kind == kInf) return 3 + (int)d.neg;
    return (int)d.neg + big_digits(big_chunks((uint32_t)d.ip, d.frac)) + 7;
}

// a wave's window of the output: lds[i] is the byte at offset base + i, base a multiple of 16.  The pieces are placed by their 32-bit
// offset from `base` (negative: the piece began in an earlier window); a piece is shorter than 2^30 + 64 bytes (tokens_ok)
struct Window {
    uint8_t* lds;
    int64_t base;
    __host__ __device__ __forceinline__ void put(int at, uint32_t byte) const {
        if ((uint32_t)at < (uint32_t)kWindow) lds[at] = (uint8_t)byte;
    }
};

// the last `n` decimal digits of v in front of `end` (leading zeros included) -> the position of the first one
__host__ __device__ __forceinline__ int put_digits(const Window& w, int end, uint32_t v, int n) {
#pragma unroll 1
    for (int k = 0; k < n; ++k) {
        const uint32_t q = v / 10u;
        w.put(--end, '0' + (v - q * 10u));
        v = q;
    }
    return end;
}

// the fmt_len(d) = len bytes of '%f' at [pos, pos + len), written from the back
__host__ __device__ __forceinline__ void fmt_put(const Dec& d, int len, const Window& w, int pos) {
    if (d.kind == kNan) {
        w.put(pos, 'n');
        w.put(pos + 1, 'a');
        w.put(pos + 2, 'n');
        return;
    }
    if (d.neg) w.put(pos, '-');
    int end = pos + len;
    if (d.kind == kInf) {
        w.put(end - 3, 'i');
        w.put(end - 2, 'n');
        w.put(end - 1, 'f');
        return;
    }
    if (d.kind == kSmall) {
        end = put_digits(w, end, d.frac, 6);
        w.put(--end, '.');
        uint64_t v = d.ip;
        while (v >> 32) {                                           // nine digits at a time: at most twice
            const uint64_t q = v / 1000000000u;
            end = put_digits(w, end, (uint32_t)(v - q * 1000000000u), 9);
            v = q;
        }
        put_digits(w, end, (uint32_t)v, end - pos - (int)d.neg);
        return;
    }
    const Chunks c = big_chunks((uint32_t)d.ip, d.frac);
    end = put_digits(w, end, 0u, 6);
    w.put(--end, '.');
    end = put_digits(w, end, c.c0, 9);
    end = put_digits(w, end, c.c1, 9);
    if (c.c3 || c.c4) {
        end = put_digits(w, end, c.c2, 9);
        if (c.c4) {
            end = put_digits(w, end, c.c3, 9);
            put_digits(w, end, c.c4, end - pos - (int)d.neg);
        } else {
            put_digits(w, end, c.c3, end - pos - (int)d.neg);
        }
    } else {
        put_digits(w, end, c.c2, end - pos - (int)d.neg);
    }
}

// ---- the pieces of a row -----------------------------------------------------------------------------------------------------------
// a token table addressed by index: token i = blob[start[i], start[i] + len[i]), len[i] = -1: no token has this index
struct Tokens {
    const uint8_t* blob;
    int64_t blob_len;
    const int64_t* start;
    const int32_t* len;
    int64_t n;
    // -> false for an index outside the table, an empty slot or a token outside the blob
    __device__ __forceinline__ bool find(int64_t i, int64_t& s, int32_t& l) const {
        s = 0;
        l = 0;
        if (i < 0 || i >= n) return false;
        const int32_t tl = len[i];
        const int64_t ts = start[i];
        if (tl < 0 || ts < 0 || ts > blob_len || (int64_t)tl > blob_len - ts) return false;
        s = ts;
        l = tl;
        return true;
    }
    __device__ __forceinline__ void put(const Window& w, int pos, int64_t s, int32_t l) const {
        const int lo = pos < 0 ? -pos : 0, hi = l < kWindow - pos ? l : kWindow - pos;      // the part inside the window
#pragma unroll 1
        for (int i = lo; i < hi; ++i) w.lds[pos + i] = blob[s + i];
    }
};

// "uid,iid:%f,iid:%f,...\n": piece j of a row is ",iid:%f" of entry j; the first one carries the uid in front, the last one of the
// row's last round the '\n' behind
struct ListRows {
    const int32_t* ids;
    const float* scores;
    const int32_t* row_user;
    int64_t n;
    int32_t K;
    Tokens users, items;

    struct Piece {
        Dec d;
        int64_t us, is;
        int32_t ul, il, fl;
        bool uid, entry, nl, bad;
        int64_t len;
    };
    __device__ __forceinline__ int64_t cols() const { return K; }
    __device__ __forceinline__ Piece piece(int64_t row, int64_t j, bool last) const {
        Piece p;
        p.uid = j == 0;
        p.nl = last;
        p.bad = false;
        p.entry = false;
        p.us = p.is = 0;
        p.ul = p.il = p.fl = 0;
        if (p.uid) p.bad = !users.find(row_user[row], p.us, p.ul);
        if (j < K) {
            const int32_t c = ids[row * K + j];
            if (c >= 0) {
                p.entry = items.find(c, p.is, p.il);
                p.bad = p.bad || !p.entry;
            }
        }
        if (p.entry) {
            p.d = decode(__float_as_uint(scores[row * K + j]));
            p.fl = fmt_len(p.d);
        }
        p.len = (int64_t)p.ul + (p.entry ? (int64_t)p.il + p.fl + 2 : 0) + (p.nl ? 1 : 0);
        return p;
    }
    __device__ __forceinline__ void put(const Piece& p, const Window& w, int pos) const {
        if (p.uid) users.put(w, pos, p.us, p.ul);
        pos += p.ul;
        if (p.entry) {
            w.put(pos, ',');
            items.put(w, pos + 1, p.is, p.il);
            pos += p.il + 1;
            w.put(pos, ':');
            fmt_put(p.d, p.fl, w, pos + 1);
            pos += p.fl + 1;
        }
        if (p.nl) w.put(pos, '\n');
    }
};

// "%f " per element and '\n' per row
struct MatrixRows {
    const float* data;
    int64_t n, n_cols;

    struct Piece {
        Dec d;
        int32_t fl;
        bool entry, nl, bad;
        int64_t len;
    };
    __device__ __forceinline__ int64_t cols() const { return n_cols; }
    __device__ __forceinline__ Piece piece(int64_t row, int64_t j, bool last) const {
        Piece p;
        p.entry = j < n_cols;
        p.nl = last;
        p.bad = false;
        p.fl = 0;
        if (p.entry) {
            p.d = decode(__float_as_uint(data[row * n_cols + j]));
            p.fl = fmt_len(p.d);
        }
        p.len = (p.entry ? p.fl + 1 : 0) + (p.nl ? 1 : 0);
        return p;
    }
    __device__ __forceinline__ void put(const Piece& p, const Window& w, int pos) const {
        if (p.entry) {
            fmt_put(p.d, p.fl, w, pos);
            pos += p.fl;
            w.put(pos++, ' ');
        }
        if (p.nl) w.put(pos, '\n');
    }
};

__device__ __forceinline__ int64_t rounds_of(int64_t cols) { return cols > 0 ? (cols + 63) / 64 : 1; }      // a row without columns still ends

template <class Rows>
__global__ __launch_bounds__(kFmtBlock) void format_sizes_kernel(Rows rows, int64_t* __restrict__ line_ptr,
                                                                unsigned long long* __restrict__ status) {
    const int lane = threadIdx.x & 63;
    const int64_t stride = (int64_t)gridDim.x * kFmtWaves;
    for (int64_t row = (int64_t)blockIdx.x * kFmtWaves + (threadIdx.x >> 6); row < rows.n; row += stride) {      // wave-uniform
        const int64_t rounds = rounds_of(rows.cols());
        int64_t sum = 0;
        bool bad = false;
        for (int64_t k = 0; k < rounds; ++k) {
            const typename Rows::Piece p = rows.piece(row, k * 64 + lane, k == rounds - 1 && lane == 63);
            sum += p.len;
            bad = bad || p.bad;
        }
        for (int off = 32; off > 0; off >>= 1) sum += __shfl_down(sum, off);
        if (bad) atomicMin(status, (unsigned long long)row);
        if (lane == 0) line_ptr[row] = sum;
    }
}

// v[0 .. n) -> its exclusive prefix in place, v[n] = totals[0] = the sum; thread x takes a contiguous run of rows (parse_scan_kernel)
__global__ __launch_bounds__(kFmtScanThreads) void format_scan_kernel(int64_t* __restrict__ v, int64_t n, int64_t* __restrict__ totals) {
    __shared__ int64_t s[2][kFmtScanThreads];
    const int x = threadIdx.x;
    const int64_t per = (n + kFmtScanThreads - 1) / kFmtScanThreads;
    const int64_t lo = x * per < n ? x * per : n;
    const int64_t hi = lo + per < n ? lo + per : n;
    int64_t own = 0;
    for (int64_t r = lo; r < hi; ++r) own += v[r];
    int cur = 0;
    s[0][x] = own;
    __syncthreads();
    for (int d = 1; d < kFmtScanThreads; d <<= 1) {                // inclusive, double-buffered
        s[cur ^ 1][x] = s[cur][x] + (x >= d ? s[cur][x - d] : 0);
        cur ^= 1;
        __syncthreads();
    }
    int64_t run = s[cur][x] - own;
    for (int64_t r = lo; r < hi; ++r) {
        const int64_t len = v[r];
        v[r] = run;
        run += len;
    }
    if (x == kFmtScanThreads - 1) {
        v[n] = s[cur][x];
        totals[0] = s[cur][x];
    }
}

// the wave's LDS traffic is its own: what its lanes wrote is read by other lanes of the same wave, in program order
__device__ __forceinline__ void wave_lds_fence() {
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
    __builtin_amdgcn_wave_barrier();
}

// bytes [lo, hi) of the window -> out: whole 16-byte chunks as one store, the chunks the row shares with a neighbour bytewise
__device__ __forceinline__ void flush(const Window& w, int64_t lo, int64_t hi, uint8_t* __restrict__ out, int lane) {
    wave_lds_fence();
#pragma unroll
    for (int o = lane * 16; o < kWindow; o += 1024) {
        const int64_t c0 = w.base + o, c1 = c0 + 16;
        if (c1 <= lo || c0 >= hi) continue;
        if (c0 >= lo && c1 <= hi) {
            *reinterpret_cast<uint4*>(out + c0) = *reinterpret_cast<const uint4*>(w.lds + o);
        } else {
#pragma unroll 1
            for (int j = 0; j < 16; ++j)
                if (c0 + j >= lo && c0 + j < hi) out[c0 + j] = w.lds[o + j];
        }
    }
    wave_lds_fence();
}

// rows [first, first + count) of the text into out[0, out_bytes): the byte at offset q of the whole text goes to out[q - line_ptr[first]]
template <class Rows>
__global__ __launch_bounds__(kFmtBlock) void format_emit_kernel(Rows rows, const int64_t* __restrict__ line_ptr, int64_t first, int64_t count,
                                                               uint8_t* __restrict__ out, int64_t out_bytes,
                                                               unsigned long long* __restrict__ status) {
    __shared__ __attribute__((aligned(16))) uint8_t s_win[kFmtWaves][kWindow];
    const int lane = threadIdx.x & 63;
    const int64_t stride = (int64_t)gridDim.x * kFmtWaves;
    const int64_t origin = line_ptr[first];
    for (int64_t at = (int64_t)blockIdx.x * kFmtWaves + (threadIdx.x >> 6); at < count; at += stride) {      // wave-uniform
        const int64_t row = first + at;
        const int64_t rs = line_ptr[row] - origin, re = line_ptr[row + 1] - origin;
        if (rs < 0 || re < rs || re > out_bytes) {                  // not the line_ptr of this block: nothing is stored
            if (lane == 0) atomicMin(status, (unsigned long long)row);
            continue;
        }
        Window w{s_win[threadIdx.x >> 6], rs & ~(int64_t)15};
        const int64_t rounds = rounds_of(rows.cols());
        int64_t a = rs;                                             // the text of the rounds so far ends here
        for (int64_t k = 0; k < rounds; ++k) {
            const typename Rows::Piece p = rows.piece(row, k * 64 + lane, k == rounds - 1 && lane == 63);
            int64_t incl = p.len;
            for (int d = 1; d < 64; d <<= 1) {
                const int64_t up = __shfl_up(incl, d);
                if (lane >= d) incl += up;
            }
            const int64_t pos = a + incl - p.len, b = a + __shfl(incl, 63);
            for (;;) {                                              // wave-uniform: a, b and the window are
                if (p.len > 0 && pos < w.base + kWindow && pos + p.len > w.base) rows.put(p, w, (int)(pos - w.base));
                if (b < w.base + kWindow) break;                    // the window is not full yet: the next round goes on in it
                flush(w, rs > w.base ? rs : w.base, re < w.base + kWindow ? re : w.base + kWindow, out, lane);
                w.base += kWindow;
                if (b <= w.base) break;
            }
            a = b;
        }
        if (a != re && lane == 0) atomicMin(status, (unsigned long long)row);      // the lengths of another input
        if (re > w.base) flush(w, rs > w.base ? rs : w.base, re < w.base + kWindow ? re : w.base + kWindow, out, lane);
    }
}

inline unsigned rows_grid(int64_t n) {
    const int64_t blocks = (n + kFmtWaves - 1) / kFmtWaves;
    return (unsigned)(blocks < (int64_t)kFmtMaxGrid ? blocks : (int64_t)kFmtMaxGrid);
}

inline bool tokens_ok(const void* blob, int64_t blob_len, const int64_t* start, const int32_t* len, int64_t n) {
    return n >= 0 && blob_len >= 0 && blob_len <= kMaxBlob && (blob_len == 0 || blob) && (n == 0 || (start && len));
}

inline bool lists_ok(const int32_t* ids, const float* scores, const int32_t* row_user, int64_t n, int32_t K) {
    return n >= 0 && K >= 0 && (n == 0 || row_user) && (n == 0 || K == 0 || (ids && scores));
}

inline bool block_ok(int64_t n, int64_t first, int64_t count, const void* out, int64_t out_bytes) {
    return first >= 0 && count >= 0 && first <= n && count <= n - first && out_bytes >= 0 && (out_bytes == 0 || out) && ((uintptr_t)out & 15) == 0;
}

template <class Rows>
int sizes(const Rows& rows, int64_t* line_ptr, int64_t* totals, hipStream_t s) {
    TKR_CHECK(hipMemsetAsync(totals, 0, sizeof(int64_t), s));
    TKR_CHECK(hipMemsetAsync(totals + 1, 0xff, sizeof(int64_t), s));      // -1: every index names a token
    if (rows.n > 0) {
        hipLaunchKernelGGL(format_sizes_kernel<Rows>, dim3(rows_grid(rows.n)), dim3(kFmtBlock), 0, s, rows, line_ptr,
                           reinterpret_cast<unsigned long long*>(totals + 1));
        TKR_LAUNCH_CHECK();
    }
    hipLaunchKernelGGL(format_scan_kernel, dim3(1), dim3(kFmtScanThreads), 0, s, line_ptr, rows.n, totals);
    TKR_LAUNCH_CHECK();
    return TKR_OK;
}

template <class Rows>
int emit(const Rows& rows, const int64_t* line_ptr, int64_t first, int64_t count, void* out, int64_t out_bytes, int64_t* status, hipStream_t s) {
    TKR_CHECK(hipMemsetAsync(status, 0xff, sizeof(int64_t), s));
    if (count > 0) {
        hipLaunchKernelGGL(format_emit_kernel<Rows>, dim3(rows_grid(count)), dim3(kFmtBlock), 0, s, rows, line_ptr, first, count,
                           static_cast<uint8_t*>(out), out_bytes, reinterpret_cast<unsigned long long*>(status));
        TKR_LAUNCH_CHECK();
    }
    return TKR_OK;
}

}  // namespace
}  // namespace tkr

extern "C" int tkr_lists_format_sizes_dev(const int32_t* ids, const float* scores, const int32_t* row_user, int64_t n, int32_t K,
                                          const void* user_blob, int64_t user_blob_len, const int64_t* user_start, const int32_t* user_len,
                                          int64_t n_users, const void* item_blob, int64_t item_blob_len, const int64_t* item_start,
                                          const int32_t* item_len, int64_t n_items, int64_t* line_ptr, int64_t* totals, void* stream) {
    if (!tkr::lists_ok(ids, scores, row_user, n, K) || !tkr::tokens_ok(user_blob, user_blob_len, user_start, user_len, n_users) ||
        !tkr::tokens_ok(item_blob, item_blob_len, item_start, item_len, n_items) || !line_ptr || !totals)
        return TKR_E_INVAL;
    const tkr::ListRows rows{ids, scores, row_user, n, K,
                             {static_cast<const uint8_t*>(user_blob), user_blob_len, user_start, user_len, n_users},
                             {static_cast<const uint8_t*>(item_blob), item_blob_len, item_start, item_len, n_items}};
    return tkr::sizes(rows, line_ptr, totals, (hipStream_t)stream);
}

extern "C" int tkr_lists_format_emit_dev(const int32_t* ids, const float* scores, const int32_t* row_user, int64_t n, int32_t K,
                                         const void* user_blob, int64_t user_blob_len, const int64_t* user_start, const int32_t* user_len,
                                         int64_t n_users, const void* item_blob, int64_t item_blob_len, const int64_t* item_start,
                                         const int32_t* item_len, int64_t n_items, const int64_t* line_ptr, int64_t first_row,
                                         int64_t n_rows, void* out, int64_t out_bytes, int64_t* status, void* stream) {
    if (!tkr::lists_ok(ids, scores, row_user, n, K) || !tkr::tokens_ok(user_blob, user_blob_len, user_start, user_len, n_users) ||
        !tkr::tokens_ok(item_blob, item_blob_len, item_start, item_len, n_items) || !line_ptr || !status ||
        !tkr::block_ok(n, first_row, n_rows, out, out_bytes))
        return TKR_E_INVAL;
    const tkr::ListRows rows{ids, scores, row_user, n, K,
                             {static_cast<const uint8_t*>(user_blob), user_blob_len, user_start, user_len, n_users},
                             {static_cast<const uint8_t*>(item_blob), item_blob_len, item_start, item_len, n_items}};
    return tkr::emit(rows, line_ptr, first_row, n_rows, out, out_bytes, status, (hipStream_t)stream);
}

extern "C" int tkr_matrix_format_sizes_dev(const float* data, int64_t rows, int64_t cols, int64_t* line_ptr, int64_t* totals, void* stream) {
    if (rows < 0 || cols < 0 || (rows > 0 && cols > 0 && !data) || !line_ptr || !totals) return TKR_E_INVAL;
    return tkr::sizes(tkr::MatrixRows{data, rows, cols}, line_ptr, totals, (hipStream_t)stream);
}

extern "C" int tkr_matrix_format_emit_dev(const float* data, int64_t rows, int64_t cols, const int64_t* line_ptr, int64_t first_row,
                                          int64_t n_rows, void* out, int64_t out_bytes, int64_t* status, void* stream) {
    if (rows < 0 || cols < 0 || (rows > 0 && cols > 0 && !data) || !line_ptr || !status || !tkr::block_ok(rows, first_row, n_rows, out, out_bytes))
        return TKR_E_INVAL;
    return tkr::emit(tkr::MatrixRows{data, rows, cols}, line_ptr, first_row, n_rows, out, out_bytes, status, (hipStream_t)stream);
}
