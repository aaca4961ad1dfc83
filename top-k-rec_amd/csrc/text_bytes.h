// Byte helpers shared by the device-side text readers: K11 (csrc/parse_dev.hip, ratings files) and K14 (csrc/scan_dev.hip, '%f '
// matrices).  Both cut the text into chunks of chunk_bytes (a power of two), give one wave a chunk, count two kinds of marks per
// chunk, and turn the chunk pairs into 64-bit exclusive prefixes with one workgroup (no library scan).
#pragma once
#include "tkr_common.h"

namespace tkr {
namespace {

constexpr int kParseBlock = 256;                                  // 4 waves = 4 chunks per workgroup
constexpr int64_t kMinChunk = 64, kMaxChunk = 1 << 20;
constexpr int64_t kWaveBytes = 64 * 16;                            // one step of a wave
constexpr int64_t kMaxChunks = (int64_t)1 << 30;
constexpr int kScanThreads = 1024;
constexpr unsigned kMaxLaneGrid = 1u << 20;                        // entries / lines beyond 2^28 are taken by a grid-stride loop

// n bytes at a 4-byte aligned p.  word(w) = bytes [4w, 4w + 4) as a little-endian word; bytes at or past n are never touched and read as 0
struct Bytes {
    const uint8_t* p;
    int64_t n;
    __device__ __forceinline__ uint32_t word(int64_t w) const {
        const int64_t o = w * 4;
        if (o + 4 <= n) return *reinterpret_cast<const uint32_t*>(p + o);
        uint32_t v = 0;
        for (int j = 0; j < 4; ++j)
            if (o + j < n) v |= (uint32_t)p[o + j] << (8 * j);
        return v;
    }
};

// a lane's reader: at(i), 0 <= i < n, keeps the word it last loaded
struct Cursor {
    Bytes t;
    int64_t w = -1;
    uint32_t v = 0;
    __device__ __forceinline__ uint32_t at(int64_t i) {
        if ((i >> 2) != w) {
            w = i >> 2;
            v = t.word(w);
        }
        return (v >> ((i & 3) * 8)) & 0xffu;
    }
};

// bytes [g, g + 16) of t, g a multiple of 16 below t.n
__device__ __forceinline__ void load16(const Bytes& t, int64_t g, uint32_t (&w)[4]) {
    if (g + 16 <= t.n) {
        const uint4 q = *reinterpret_cast<const uint4*>(t.p + g);
        w[0] = q.x; w[1] = q.y; w[2] = q.z; w[3] = q.w;
    } else {
#pragma unroll
        for (int k = 0; k < 4; ++k) w[k] = g + 4 * k < t.n ? t.word((g >> 2) + k) : 0u;
    }
}

// bit 7 of every byte of w that equals c, nothing else (exact: no borrow runs between the bytes)
__device__ __forceinline__ uint32_t mark_eq(uint32_t w, uint32_t c) {
    const uint32_t x = w ^ (c * 0x01010101u);
    return ~(((x & 0x7f7f7f7fu) + 0x7f7f7f7fu) | x) & 0x80808080u;
}

// number of bytes of w equal to c
__device__ __forceinline__ uint32_t count_eq(uint32_t w, uint32_t c) { return __popc(mark_eq(w, c)); }

// exclusive prefixes of the chunk pairs and the totals; thread x takes a contiguous run of chunks.  totals[0] counts a last line
// without a terminator
__global__ __launch_bounds__(kScanThreads) void chunk_scan_kernel(Bytes t, const uint2* __restrict__ counts, int64_t n_chunks,
                                                                 int64_t* __restrict__ off_x, int64_t* __restrict__ off_y,
                                                                 int64_t* __restrict__ totals) {
    __shared__ int64_t s_x[2][kScanThreads], s_y[2][kScanThreads];
    const int x = threadIdx.x;
    const int64_t per = (n_chunks + kScanThreads - 1) / kScanThreads;
    const int64_t lo = x * per < n_chunks ? x * per : n_chunks;
    const int64_t hi = lo + per < n_chunks ? lo + per : n_chunks;
    int64_t nx = 0, ny = 0;
    for (int64_t c = lo; c < hi; ++c) {
        const uint2 v = counts[c];
        nx += v.x;
        ny += v.y;
    }
    int cur = 0;
    s_x[0][x] = nx;
    s_y[0][x] = ny;
    __syncthreads();
    for (int d = 1; d < kScanThreads; d <<= 1) {                   // inclusive, double-buffered
        s_x[cur ^ 1][x] = s_x[cur][x] + (x >= d ? s_x[cur][x - d] : 0);
        s_y[cur ^ 1][x] = s_y[cur][x] + (x >= d ? s_y[cur][x - d] : 0);
        cur ^= 1;
        __syncthreads();
    }
    int64_t run_x = s_x[cur][x] - nx, run_y = s_y[cur][x] - ny;
    for (int64_t c = lo; c < hi; ++c) {
        const uint2 v = counts[c];
        off_x[c] = run_x;
        off_y[c] = run_y;
        run_x += v.x;
        run_y += v.y;
    }
    if (x == kScanThreads - 1) {
        totals[0] = s_x[cur][x] + ((t.n > 0 && t.p[t.n - 1] != '\n') ? 1 : 0);      // a last line without a terminator counts
        totals[1] = s_y[cur][x];
    }
}

inline bool chunk_ok(int64_t chunk) { return chunk >= kMinChunk && chunk <= kMaxChunk && (chunk & (chunk - 1)) == 0; }
inline int64_t chunks_of(int64_t n_bytes, int64_t chunk) { return (n_bytes + chunk - 1) / chunk; }
inline unsigned lane_grid(int64_t n) {
    const int64_t blocks = (n + kParseBlock - 1) / kParseBlock;
    return (unsigned)(blocks < (int64_t)kMaxLaneGrid ? blocks : (int64_t)kMaxLaneGrid);
}

// the three arrays in front of the workspace, each 256-byte aligned, and 256 spare bytes behind them (K14 keeps its status word there)
struct Workspace {
    uint2* counts;
    int64_t *off_x, *off_y;
    unsigned long long* spare;
    static int64_t part(int64_t n_chunks) { return (n_chunks * 8 + 255) / 256 * 256; }
    static int64_t bytes(int64_t n_chunks) { return 3 * part(n_chunks) + 256; }
    Workspace(void* ws, int64_t n_chunks) {
        char* p = static_cast<char*>(ws);
        counts = reinterpret_cast<uint2*>(p);
        off_x = reinterpret_cast<int64_t*>(p + part(n_chunks));
        off_y = reinterpret_cast<int64_t*>(p + 2 * part(n_chunks));
        spare = reinterpret_cast<unsigned long long*>(p + 3 * part(n_chunks));
    }
};

}  // namespace
}  // namespace tkr
