// K15: the grouping of evaluate._group on the device -- parsed ratings (K11's flat arrays) or rows of a CSR in, a CSR with ascending,
// duplicate-free columns out, for rows that arrive grouped: row r is the union of the counted items of one segment of each source.
// A segment is a line of a parsed file (seg_ptr = line_ptr) or a row of a CSR; an entry counts when item >= 0 (with like_only: and
// like == 1).  The entries of a segment are adjacent, so nothing is sorted:
//
//   count   the row's set is a bitmap of n_cols bits in LDS: zeroed, the segments read coalesced and their bits set with LDS OR atomics,
//           the popcounts summed over the team; one size per row.  No compare network, the cost does not depend on duplicates
//   scan    one workgroup: 64-bit exclusive prefix of the sizes, in place -> ptr[n_rows + 1], totals[0] = ptr[n_rows]  -> the host allocates
//   emit    the bitmap is built again; every lane owns a contiguous run of its words, a team prefix of the popcounts gives the lane
//           its place, and it writes the column numbers of its set bits from ptr[r] + prefix on: ascending by construction
//
// One body, two teams: a wave per row, four rows per workgroup, while n_cols <= TKR_GROUP_WAVE_COLS (4 KB of bitmap per wave: the 32
// waves a CU holds keep 128 of its 160 KB); above that one workgroup of 1024 lanes per row, up to TKR_GROUP_MAX_COLS, what one
// workgroup's LDS holds.  A row of any length runs: its length only sets how many loads it makes.
//
// Nothing of the input is trusted: seg_of_row must lie in [-1, n_seg), a segment in [0, n_entries) with seg_ptr never decreasing, a
// counted item below n_cols; whatever is not is never used as an index, and the smallest 4 * (row or segment) + kind of what was
// refused goes to the status word (-1: nothing).  emit checks ptr against what it counts before it writes.  The only global atomics are
// the status word's min and last_line's max: order-independent, so every output is deterministic.
//
// tkr_last_line_of_user_dev: last[u] = the largest line whose line_user is u, -1 where none is (fill, then a 64-bit atomic max).
// tkr_compact_rows_*_dev: the rows of a CSR with at least one element, ascending, and the ptr of the CSR that keeps only them.
#include "tkr_common.h"
#include "../../include/tkr.h"

namespace tkr {
namespace {

constexpr int kGroupWaveBlock = 256;                              // 4 waves = 4 rows per workgroup
constexpr int kGroupWgBlock = 1024;                               // 16 waves on one row
constexpr int kGroupScratchWords = 16;                            // in front of the bitmaps: the wave totals of the wide team
constexpr unsigned kGroupMaxGrid = 1u << 20;
constexpr int kGroupScanThreads = 1024;
constexpr int kGroupLaneBlock = 256;

enum { kBadSegOfRow = 0, kBadSegPtr = 1, kBadItem = 2, kBadPtr = 3 };

struct GroupArgs {
    tkr_group_source src[2];
    int32_t n_src, n_cols, like_only;
    int64_t n_rows;
};

// T lanes work on one row: T = 64, a wave of a kGroupWaveBlock workgroup, or T = kGroupWgBlock, the workgroup
template <int T>
struct Team {
    static constexpr int rows = T == 64 ? kGroupWaveBlock / 64 : 1;    // rows per workgroup
    static constexpr int block = T == 64 ? kGroupWaveBlock : kGroupWgBlock;
    __device__ static __forceinline__ int lane() { return T == 64 ? (int)(threadIdx.x & 63) : (int)threadIdx.x; }
    __device__ static __forceinline__ int row() { return T == 64 ? (int)(threadIdx.x >> 6) : 0; }
};

__device__ __forceinline__ uint32_t wave_incl(uint32_t v) {
    const int lane = threadIdx.x & 63;
    for (int d = 1; d < 64; d <<= 1) {
        const uint32_t up = __shfl_up(v, d);
        if (lane >= d) v += up;
    }
    return v;
}

// exclusive prefix of v over the team and the team's total.  The wide team goes through `scratch`; the caller's next barrier
// separates this use from the next
template <int T>
__device__ __forceinline__ uint32_t team_prefix(uint32_t v, uint32_t* scratch, uint32_t* total) {
    const uint32_t incl = wave_incl(v);
    if (T == 64) {
        *total = __shfl(incl, 63);
        return incl - v;
    }
    const int wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 63) scratch[wave] = incl;
    __syncthreads();
    uint32_t before = 0, all = 0;
    for (int k = 0; k < kGroupWgBlock / 64; ++k) {
        const uint32_t t = scratch[k];
        all += t;
        if (k < wave) before += t;
    }
    *total = all;
    return before + incl - v;
}

// the set of row r as bits of bm[0, W).  Every lane of the workgroup arrives, `active` or not (uniform over the team)
template <int T>
__device__ __forceinline__ void build_bitmap(const GroupArgs& a, int64_t r, bool active, uint32_t* bm, int W, unsigned long long* status) {
    const int tl = Team<T>::lane();
    for (int w = tl; w < W; w += T) bm[w] = 0u;
    __syncthreads();
    if (active) {
        for (int s = 0; s < a.n_src; ++s) {
            const tkr_group_source& src = a.src[s];
            const int64_t seg = src.seg_of_row ? src.seg_of_row[r] : r;
            if (seg == -1) continue;
            if (seg < -1 || seg >= src.n_seg) {
                if (tl == 0) status_refuse(status, r, kBadSegOfRow);
                continue;
            }
            const int64_t lo = src.seg_ptr[seg], hi = src.seg_ptr[seg + 1];
            if (lo < 0 || hi < lo || hi > src.n_entries) {
                if (tl == 0) status_refuse(status, r, kBadSegPtr);
                continue;
            }
            bool bad = false;
            for (int64_t e = lo + tl; e < hi; e += T) {
                const int32_t it = src.item[e];
                if (it < 0 || (a.like_only && src.like[e] != 1)) continue;
                if (it >= a.n_cols) {
                    bad = true;                                        // never a bit index
                    continue;
                }
                atomicOr(&bm[it >> 5], 1u << (it & 31));
            }
            if (bad) status_refuse(status, r, kBadItem);
        }
    }
    __syncthreads();
}

template <int T>
__global__ __launch_bounds__(Team<T>::block) void group_count_kernel(GroupArgs a, int64_t* __restrict__ sizes, unsigned long long* __restrict__ status) {
    extern __shared__ __attribute__((aligned(16))) uint32_t group_lds[];
    const int W = (a.n_cols + 31) >> 5;
    uint32_t* scratch = group_lds;
    uint32_t* bm = group_lds + kGroupScratchWords + (size_t)Team<T>::row() * W;
    const int tl = Team<T>::lane();
    // every seg_ptr is checked once, used by a row or not
    for (int s = 0; s < a.n_src; ++s) {
        const tkr_group_source& src = a.src[s];
        for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < src.n_seg; i += (int64_t)gridDim.x * blockDim.x) {
            const int64_t lo = src.seg_ptr[i], hi = src.seg_ptr[i + 1];
            if (lo < 0 || hi < lo || hi > src.n_entries) status_refuse(status, i, kBadSegPtr);
        }
    }
    for (int64_t base = (int64_t)blockIdx.x * Team<T>::rows; base < a.n_rows; base += (int64_t)gridDim.x * Team<T>::rows) {      // uniform over the workgroup
        const int64_t r = base + Team<T>::row();
        const bool active = r < a.n_rows;
        build_bitmap<T>(a, r, active, bm, W, status);
        uint32_t n = 0;
        for (int w = tl; w < W; w += T) n += __popc(bm[w]);
        uint32_t total;
        team_prefix<T>(n, scratch, &total);
        if (active && tl == 0) sizes[r] = (int64_t)total;
        __syncthreads();                                               // the bitmap and the scratch are free again
    }
}

template <int T>
__global__ __launch_bounds__(Team<T>::block) void group_emit_kernel(GroupArgs a, const int64_t* __restrict__ ptr, int32_t* __restrict__ cols, int64_t n_out,
                                                                   unsigned long long* __restrict__ status) {
    extern __shared__ __attribute__((aligned(16))) uint32_t group_lds[];
    const int W = (a.n_cols + 31) >> 5;
    uint32_t* scratch = group_lds;
    uint32_t* bm = group_lds + kGroupScratchWords + (size_t)Team<T>::row() * W;
    const int tl = Team<T>::lane();
    const int per = (W + T - 1) / T;                                   // a lane's run of words
    const int w0 = tl * per < W ? tl * per : W, w1 = w0 + per < W ? w0 + per : W;
    for (int64_t base = (int64_t)blockIdx.x * Team<T>::rows; base < a.n_rows; base += (int64_t)gridDim.x * Team<T>::rows) {
        const int64_t r = base + Team<T>::row();
        const bool active = r < a.n_rows;
        build_bitmap<T>(a, r, active, bm, W, status);
        uint32_t n = 0;
        for (int w = w0; w < w1; ++w) n += __popc(bm[w]);
        uint32_t total;
        const uint32_t before = team_prefix<T>(n, scratch, &total);
        if (active) {
            const int64_t p0 = ptr[r], p1 = ptr[r + 1];
            if (p0 < 0 || p1 < p0 || p1 > n_out || p1 - p0 != (int64_t)total) {      // not the ptr of these sources: nothing is written
                if (tl == 0) status_refuse(status, r, kBadPtr);
            } else {
                int64_t o = p0 + before;                               // o + n <= p1 <= n_out
                for (int w = w0; w < w1; ++w) {
                    uint32_t bits = bm[w];
                    while (bits) {
                        cols[o++] = w * 32 + (__ffs(bits) - 1);
                        bits &= bits - 1;
                    }
                }
            }
        }
        __syncthreads();
    }
}

// out[c] = sum of v(c') over c' < c, out[n] = the total (also to *total when given); v(c) = in[c], or with FLAG in[c + 1] > in[c].
// Thread x takes a contiguous run; in == out is allowed without FLAG (a thread reads an element before it alone writes it)
template <bool FLAG>
__global__ __launch_bounds__(kGroupScanThreads) void group_scan_kernel(const int64_t* in, int64_t n, int64_t* out, int64_t* total) {
    __shared__ int64_t s[2][kGroupScanThreads];
    const int x = threadIdx.x;
    const int64_t per = (n + kGroupScanThreads - 1) / kGroupScanThreads;
    const int64_t lo = x * per < n ? x * per : n;
    const int64_t hi = lo + per < n ? lo + per : n;
    int64_t own = 0;
    for (int64_t c = lo; c < hi; ++c) own += FLAG ? (int64_t)(in[c + 1] > in[c]) : in[c];
    int cur = 0;
    s[0][x] = own;
    __syncthreads();
    for (int d = 1; d < kGroupScanThreads; d <<= 1) {              // inclusive, double-buffered
        s[cur ^ 1][x] = s[cur][x] + (x >= d ? s[cur][x - d] : 0);
        cur ^= 1;
        __syncthreads();
    }
    int64_t run = s[cur][x] - own;
    for (int64_t c = lo; c < hi; ++c) {
        const int64_t v = FLAG ? (int64_t)(in[c + 1] > in[c]) : in[c];
        out[c] = run;
        run += v;
    }
    if (x == kGroupScanThreads - 1) {
        out[n] = s[cur][x];
        if (total) *total = s[cur][x];
    }
}

__global__ __launch_bounds__(kGroupLaneBlock) void last_line_kernel(const int32_t* __restrict__ line_user, int64_t n_lines, int64_t n_users,
                                                                   long long* __restrict__ last) {
    for (int64_t i = (int64_t)blockIdx.x * kGroupLaneBlock + threadIdx.x; i < n_lines; i += (int64_t)gridDim.x * kGroupLaneBlock) {
        const int64_t u = line_user[i];
        if (u >= 0 && u < n_users) atomicMax(&last[u], (long long)i);
    }
}

__global__ __launch_bounds__(kGroupLaneBlock) void compact_emit_kernel(const int64_t* __restrict__ ptr, const int64_t* __restrict__ pos, int64_t n_rows,
                                                                      int64_t n_kept, int64_t* __restrict__ rows, int64_t* __restrict__ out_ptr,
                                                                      unsigned long long* __restrict__ status) {
    for (int64_t r = (int64_t)blockIdx.x * kGroupLaneBlock + threadIdx.x; r < n_rows; r += (int64_t)gridDim.x * kGroupLaneBlock) {
        if (ptr[r + 1] <= ptr[r]) continue;
        const int64_t k = pos[r];
        if (k < 0 || k >= n_kept) {                                    // not the pos of this ptr
            status_refuse(status, r, kBadPtr);
            continue;
        }
        rows[k] = r;
        out_ptr[k] = ptr[r];                                           // the rows left out are empty: the offsets stay
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) out_ptr[n_kept] = ptr[n_rows];
}

inline unsigned lane_blocks(int64_t n) {
    const int64_t blocks = (n + kGroupLaneBlock - 1) / kGroupLaneBlock;
    return (unsigned)(blocks < 1 ? 1 : blocks < (int64_t)kGroupMaxGrid ? blocks : (int64_t)kGroupMaxGrid);
}

// TKR_OK, or why the arguments cannot be taken; no device access
int group_args(const tkr_group_source* src, int32_t n_src, int64_t n_rows, int32_t n_cols, int32_t like_only, GroupArgs* out) {
    if (!src || n_src < 1 || n_src > 2 || n_rows <= 0 || n_cols <= 0) return TKR_E_INVAL;
    for (int s = 0; s < n_src; ++s) {
        const tkr_group_source& q = src[s];
        if (!q.seg_ptr || q.n_seg < 0 || q.n_entries < 0 || (q.n_entries > 0 && !q.item) || (like_only && q.n_entries > 0 && !q.like) ||
            (!q.seg_of_row && q.n_seg < n_rows) || ((uintptr_t)q.seg_ptr & 7) || ((uintptr_t)q.seg_of_row & 7) || ((uintptr_t)q.item & 3) ||
            ((uintptr_t)q.like & 3))
            return TKR_E_INVAL;
        out->src[s] = q;
    }
    if (n_src == 1) out->src[1] = tkr_group_source{nullptr, nullptr, nullptr, nullptr, 0, 0};
    out->n_src = n_src;
    out->n_cols = n_cols;
    out->like_only = like_only ? 1 : 0;
    out->n_rows = n_rows;
    return n_cols > TKR_GROUP_MAX_COLS ? TKR_E_UNSUPPORTED : TKR_OK;
}

template <int T>
size_t group_lds_bytes(int32_t n_cols) {
    return ((size_t)kGroupScratchWords + (size_t)Team<T>::rows * ((n_cols + 31) >> 5)) * 4;
}

static_assert(((size_t)kGroupScratchWords + ((TKR_GROUP_MAX_COLS + 31) >> 5)) * 4 <= 160 * 1024, "one workgroup's LDS");
static_assert(((size_t)kGroupScratchWords + (kGroupWaveBlock / 64) * ((TKR_GROUP_WAVE_COLS + 31) >> 5)) * 4 * (32 / (kGroupWaveBlock / 64)) <= 160 * 1024,
              "the bitmaps of the 32 waves a CU holds");

template <int T>
unsigned group_grid(int64_t n_rows) {
    const int64_t blocks = (n_rows + Team<T>::rows - 1) / Team<T>::rows;
    const int64_t cap = T == 64 ? (int64_t)kGroupMaxGrid : 1 << 14;
    return (unsigned)(blocks < cap ? blocks : cap);
}

template <int T>
int launch_count(const GroupArgs& a, int64_t* sizes, unsigned long long* status, hipStream_t s) {
    auto kern = group_count_kernel<T>;
    if (T != 64) TKR_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
    hipLaunchKernelGGL(kern, dim3(group_grid<T>(a.n_rows)), dim3(Team<T>::block), group_lds_bytes<T>(a.n_cols), s, a, sizes, status);
    return (int)hipGetLastError();
}

template <int T>
int launch_emit(const GroupArgs& a, const int64_t* ptr, int32_t* cols, int64_t n_out, unsigned long long* status, hipStream_t s) {
    auto kern = group_emit_kernel<T>;
    if (T != 64) TKR_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
    hipLaunchKernelGGL(kern, dim3(group_grid<T>(a.n_rows)), dim3(Team<T>::block), group_lds_bytes<T>(a.n_cols), s, a, ptr, cols, n_out, status);
    return (int)hipGetLastError();
}

}  // namespace
}  // namespace tkr

extern "C" int tkr_group_count_dev(const tkr_group_source* src, int32_t n_src, int64_t n_rows, int32_t n_cols, int32_t like_only,
                                   int64_t* ptr, int64_t* totals, void* stream) {
    tkr::GroupArgs a;
    if (!ptr || !totals || ((uintptr_t)ptr & 7) || ((uintptr_t)totals & 7)) return TKR_E_INVAL;
    TKR_CHECK_RC(tkr::group_args(src, n_src, n_rows, n_cols, like_only, &a));
    hipStream_t s = (hipStream_t)stream;
    unsigned long long* status = reinterpret_cast<unsigned long long*>(totals) + 1;
    TKR_CHECK(hipMemsetAsync(status, 0xff, sizeof(unsigned long long), s));          // -1: nothing refused
    if (n_cols <= TKR_GROUP_WAVE_COLS) {
        TKR_CHECK_RC(tkr::launch_count<64>(a, ptr, status, s));
    } else {
        TKR_CHECK_RC(tkr::launch_count<tkr::kGroupWgBlock>(a, ptr, status, s));
    }
    hipLaunchKernelGGL(tkr::group_scan_kernel<false>, dim3(1), dim3(tkr::kGroupScanThreads), 0, s, ptr, n_rows, ptr, totals);
    TKR_LAUNCH_CHECK();
    return TKR_OK;
}

extern "C" int tkr_group_emit_dev(const tkr_group_source* src, int32_t n_src, int64_t n_rows, int32_t n_cols, int32_t like_only,
                                  const int64_t* ptr, int32_t* cols, int64_t n_out, int64_t* status, void* stream) {
    tkr::GroupArgs a;
    if (!ptr || !status || n_out < 0 || (n_out > 0 && !cols) || ((uintptr_t)ptr & 7) || ((uintptr_t)status & 7) || ((uintptr_t)cols & 3))
        return TKR_E_INVAL;
    TKR_CHECK_RC(tkr::group_args(src, n_src, n_rows, n_cols, like_only, &a));
    hipStream_t s = (hipStream_t)stream;
    unsigned long long* st = reinterpret_cast<unsigned long long*>(status);
    TKR_CHECK(hipMemsetAsync(st, 0xff, sizeof(unsigned long long), s));
    if (n_cols <= TKR_GROUP_WAVE_COLS) return tkr::launch_emit<64>(a, ptr, cols, n_out, st, s);
    return tkr::launch_emit<tkr::kGroupWgBlock>(a, ptr, cols, n_out, st, s);
}

extern "C" int tkr_last_line_of_user_dev(const int32_t* line_user, int64_t n_lines, int64_t n_users, int64_t* last, void* stream) {
    if (!line_user || !last || n_lines <= 0 || n_users <= 0 || ((uintptr_t)line_user & 3) || ((uintptr_t)last & 7)) return TKR_E_INVAL;
    hipStream_t s = (hipStream_t)stream;
    TKR_CHECK(hipMemsetAsync(last, 0xff, (size_t)n_users * sizeof(int64_t), s));      // -1: no line
    hipLaunchKernelGGL(tkr::last_line_kernel, dim3(tkr::lane_blocks(n_lines)), dim3(tkr::kGroupLaneBlock), 0, s, line_user, n_lines, n_users,
                       reinterpret_cast<long long*>(last));
    TKR_LAUNCH_CHECK();
    return TKR_OK;
}

extern "C" int tkr_compact_rows_count_dev(const int64_t* ptr, int64_t n_rows, int64_t* pos, void* stream) {
    if (!ptr || !pos || n_rows <= 0 || ((uintptr_t)ptr & 7) || ((uintptr_t)pos & 7)) return TKR_E_INVAL;
    hipLaunchKernelGGL(tkr::group_scan_kernel<true>, dim3(1), dim3(tkr::kGroupScanThreads), 0, (hipStream_t)stream, ptr, n_rows, pos,
                       (int64_t*)nullptr);
    TKR_LAUNCH_CHECK();
    return TKR_OK;
}

extern "C" int tkr_compact_rows_emit_dev(const int64_t* ptr, const int64_t* pos, int64_t n_rows, int64_t n_kept, int64_t* rows,
                                         int64_t* out_ptr, int64_t* status, void* stream) {
    if (!ptr || !pos || !out_ptr || !status || n_rows <= 0 || n_kept < 0 || n_kept > n_rows || (n_kept > 0 && !rows) || ((uintptr_t)ptr & 7) ||
        ((uintptr_t)pos & 7) || ((uintptr_t)rows & 7) || ((uintptr_t)out_ptr & 7) || ((uintptr_t)status & 7))
        return TKR_E_INVAL;
    hipStream_t s = (hipStream_t)stream;
    unsigned long long* st = reinterpret_cast<unsigned long long*>(status);
    TKR_CHECK(hipMemsetAsync(st, 0xff, sizeof(unsigned long long), s));
    hipLaunchKernelGGL(tkr::compact_emit_kernel, dim3(tkr::lane_blocks(n_rows)), dim3(tkr::kGroupLaneBlock), 0, s, ptr, pos, n_rows, n_kept, rows,
                       out_ptr, st);
    TKR_LAUNCH_CHECK();
    return TKR_OK;
}
