// K28 / K29 -- the item-neighbourhood model (ItemKNN): built from the likes and served from histories (include/tkr.h; DESIGN.md
// section 4 K28/K29).  Nothing of size n_items x n_items is ever in memory, every sum is an integer or a stated fp32 chain, and the only
// atomics are integer ones: the status word's minimum, LDS counters, the partial counters of a split row.
//
//   knn_check_kernel     the pre-pass of K28: both pointer arrays, every column and row, the entry counts, the norms.  Every later
//                        kernel of the call returns at once when the status word is not clean, so a refused call writes nothing.
//   knn_plan_kernel      one wave per item: work_i = sum over the likers u of n_u.  An item with work_i > heavy_from is HEAVY: it gets
//                        parts_i = min(kKnnMaxParts, likers_i, ceil(work_i / heavy_from)) and a slot in the list of heavy items (an
//                        integer counter; the order of the list changes no result).
//   knn_light_kernel     one workgroup per light item: a uint32 counter per column of the slab in LDS, the likers walked through the
//                        item-major CSR 64 at a time per wave (their list ends are loaded side by side), the lanes along one user's
//                        list, no-return LDS adds.  Then, in the same LDS: counters -> ordered keys (the fp64 formula, one division,
//                        rounded once), a radix select of the N best (key, column) pairs, a bitonic sort of the winners.
//   knn_partial_kernel   part p of heavy item i counts its share of the likers the same way and adds what is not zero to the item's
//                        row of the workspace (integer atomics: order-free).  The heavy items go in batches of as many rows as the
//                        workspace holds.
//   knn_finish_kernel    one workgroup per heavy item of the batch: reads the row (and zeroes it for the next batch), selects as above.
//   A catalogue wider than the slab is walked once per slab; the slab's winners join the running best N and the 2 N are sorted again:
//   the pairs are distinct, so the result does not depend on the slab width, as it does not on heavy_from.
//
//   knn_score_check_kernel   the pre-pass of K29: hist_ptr, the history columns, like_ptr.
//   knn_score_kernel     one workgroup per line: an fp32 accumulator per scenario column of the slab in LDS; the history is walked in
//                        stored order by the workgroup's first wave alone, the lanes along the neighbour list of one history item (ids
//                        inside a list are distinct: plain read-add-write), sixteen list pieces loaded ahead of the adds.  All four
//                        waves then turn the accumulators into ordered keys (0: masked), select and sort the K best as K28 does,
//                        and rank the likes, a wave per like, by counting the pairs in front of it in the same array.  Nothing of a
//                        line passes through global memory on the way.
#include "tkr_common.h"
#include "topk_parts.h"
#include "../../include/tkr.h"

#include <limits.h>
#include <math.h>

#include <algorithm>

// sim(i, j) is defined operation by operation (include/tkr.h): no product may be fused into the sum that follows it
#pragma clang fp contract(off)

namespace tkr {

constexpr int kKnnBlock = 256;
constexpr int kKnnMaxParts = 64;                                 // workgroups that share one heavy row, at most
constexpr int kKnnAhead = 16;                                    // pieces of neighbour lists K29 loads before it adds them
constexpr size_t kKnnLdsBudget = 160 * 1024;                     // what one CU holds
constexpr int kKnnHeadWords = 256 + 8;                           // the digit histogram, four control words (and padding)
// K28's kinds / K29's kinds
enum { kKnnBadPtr = 0, kKnnBadIndex = 1, kKnnCountsDiffer = 2, kKnnBadNorm = 3 };
enum { kKnnScoreBadPtr = 0, kKnnScoreBadCol = 1, kKnnScoreBadLikePtr = 2 };
static_assert((size_t)TKR_KNN_MAX_SLAB * 4 + 2 * TKR_KNN_MAX_N * 8 + (kKnnHeadWords + 2 * kKnnBlock) * 4 <= kKnnLdsBudget, "the widest slab fits beside the lists");

__host__ __device__ inline int knn_sort_width(int want) {        // the power of two that holds the running best and a slab's winners
    int p = 2;
    while (p < 2 * want) p <<= 1;
    return p;
}

__device__ __forceinline__ bool knn_clean(const unsigned long long* status) {
    return __hip_atomic_load(status, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == ~0ull;
}

// ---- the selection both kernels share ---------------------------------------------------------------------------------------------
// keys[0 .. n): an ordered 32-bit key per column base + j of the slab, 0 = not a candidate.  A candidate is the pair
// (key << 32) | column: pairs are distinct, larger = further in front in the canonical order (score descending, ties -> the higher
// column first).  On entry cand[0 .. want) holds the running best (0 = empty); on return it holds the best `want` of those and the
// slab's candidates, descending.  P = knn_sort_width(want) entries; hist: 256 words; ctl: 4 words.  n_total: the columns of all slabs.
template <int BLOCK>
__device__ void knn_select_into(const uint32_t* keys, int n, uint32_t base, uint32_t n_total, int want, uint64_t* cand, int P, uint32_t* hist,
                                uint32_t* ctl) {
    const int tid = threadIdx.x;
    for (int t = want + tid; t < P; t += BLOCK) cand[t] = 0ull;
    if (tid < 4) ctl[tid] = 0u;                                   // 0: candidates, 1: the digit, 2: pairs above it, 3: winners written
    __syncthreads();
    uint32_t mine = 0;
    for (int j = tid; j < n; j += BLOCK) mine += keys[j] != 0u;
    if (mine) atomicAdd(&ctl[0], mine);
    __syncthreads();
    const uint32_t n_cand = ctl[0];
    uint64_t thr = 0ull;                                          // every candidate wins
    if (n_cand > (uint32_t)want) {                                // (uniform) the want-th largest pair, a byte at a time from the top
        uint64_t prefix = 0ull;
        uint32_t left = (uint32_t)want;
        for (int b = 7; b >= 0; --b) {
            if (b < 4 && ((n_total - 1u) >> (8 * b)) == 0u) {     // no column has a bit in this byte
                prefix <<= 8;
                continue;
            }
            for (int t = tid; t < 256; t += BLOCK) hist[t] = 0u;
            __syncthreads();
            for (int j = tid; j < n; j += BLOCK) {
                const uint32_t k = keys[j];
                if (k == 0u) continue;
                const uint64_t pair = ((uint64_t)k << 32) | (uint64_t)(base + (uint32_t)j);
                if (b == 7 || (pair >> (8 * (b + 1))) == prefix) atomicAdd(&hist[(uint32_t)(pair >> (8 * b)) & 255u], 1u);
            }
            __syncthreads();
            if (tid < TKR_WAVE) {                                 // lane l owns the digits 255 - 4 l .. 252 - 4 l, descending
                uint32_t h[4];
#pragma unroll
                for (int q = 0; q < 4; ++q) h[q] = hist[255 - 4 * tid - q];
                const uint32_t s = h[0] + h[1] + h[2] + h[3];
                uint32_t incl = s;
#pragma unroll
                for (int o = 1; o < TKR_WAVE; o <<= 1) {
                    const uint32_t up = (uint32_t)__shfl_up((int)incl, o, TKR_WAVE);
                    if (tid >= o) incl += up;
                }
                uint32_t run = incl - s;
                if (run < left && left <= incl) {                 // one lane: the digit of the left-th largest is one of its four
#pragma unroll
                    for (int q = 0; q < 4; ++q) {
                        if (left <= run + h[q]) {
                            ctl[1] = (uint32_t)(255 - 4 * tid - q);
                            ctl[2] = run;
                            break;
                        }
                        run += h[q];
                    }
                }
            }
            __syncthreads();
            prefix = (prefix << 8) | (uint64_t)ctl[1];
            left -= ctl[2];
        }
        thr = prefix;
    }
    for (int j = tid; j < n; j += BLOCK) {
        const uint32_t k = keys[j];
        if (k == 0u) continue;
        const uint64_t pair = ((uint64_t)k << 32) | (uint64_t)(base + (uint32_t)j);
        if (pair >= thr) {
            const uint32_t pos = atomicAdd(&ctl[3], 1u);
            if (pos < (uint32_t)(P - want)) cand[want + pos] = pair;      // (at most `want` pairs reach thr)
        }
    }
    __syncthreads();
    for (int size = 2; size <= P; size <<= 1) {                   // bitonic, descending; the pairs are distinct, so any network gives one result
        for (int stride = size >> 1; stride > 0; stride >>= 1) {
            for (int t = tid; t < P; t += BLOCK) {
                const int o = t ^ stride;
                if (o > t) {
                    const uint64_t a = cand[t], c = cand[o];
                    const bool desc = (t & size) == 0;
                    if (desc ? a < c : a > c) {
                        cand[t] = c;
                        cand[o] = a;
                    }
                }
            }
            __syncthreads();
        }
    }
}

// ---- K28 --------------------------------------------------------------------------------------------------------------------------
struct KnnBuild {
    const int64_t* u_ptr;
    const int32_t* u_cols;
    const int64_t* i_ptr;
    const int32_t* i_rows;
    const double* norm;
    long long n_u_entries, n_i_entries;
    int n_users, n_items, N, slab, rows, pitch;                   // rows: the heavy items of a batch; pitch: uint32 words of a workspace row
    double shrink;
    long long heavy_from;
    unsigned int* n_heavy;                                        // workspace: the counter, parts [n_items], heavy_list [n_items], the rows
    int32_t* parts;
    int32_t* heavy_list;
    unsigned int* part_rows;
    int32_t* nbr_ids;
    float* nbr_w;
    unsigned long long* status;
};

__device__ __forceinline__ void knn_check_ptr(const int64_t* ptr, long long t, long long n, long long len, long long where,
                                              unsigned long long* status) {
    const long long v = ptr[t];
    bool bad = v < 0 || v > len || (t == 0 && v != 0);
    if (t < n) bad = bad || ptr[t + 1] < v;
    if (bad) status_refuse(status, where, kKnnBadPtr);
}

__global__ __launch_bounds__(kKnnBlock) void knn_check_kernel(KnnBuild a, long long total) {
    // an end outside its array checks no entry (and is refused as a pointer)
    const long long u_end = a.u_ptr[a.n_users], i_end = a.i_ptr[a.n_items];
    const bool u_ok = u_end >= 0 && u_end <= a.n_u_entries, i_ok = i_end >= 0 && i_end <= a.n_i_entries;
    const long long u_n = u_ok ? u_end : 0, i_n = i_ok ? i_end : 0;
    for (long long t = (long long)blockIdx.x * kKnnBlock + threadIdx.x; t < total; t += (long long)gridDim.x * kKnnBlock) {
        if (t <= a.n_users) knn_check_ptr(a.u_ptr, t, a.n_users, a.n_u_entries, t, a.status);
        if (t <= a.n_items) knn_check_ptr(a.i_ptr, t, a.n_items, a.n_i_entries, (long long)a.n_users + 1 + t, a.status);
        if (t < u_n && (uint32_t)a.u_cols[t] >= (uint32_t)a.n_items) status_refuse(a.status, t, kKnnBadIndex);
        if (t < i_n && (uint32_t)a.i_rows[t] >= (uint32_t)a.n_users) status_refuse(a.status, a.n_u_entries + t, kKnnBadIndex);
        if (t < a.n_items) {
            const double v = a.norm[t];
            if (!(v > 0.0 && v < INFINITY)) status_refuse(a.status, t, kKnnBadNorm);
        }
        if (t == 0 && u_ok && i_ok && u_end != i_end) status_refuse(a.status, 0, kKnnCountsDiffer);
    }
}

__global__ __launch_bounds__(kKnnBlock) void knn_plan_kernel(KnnBuild a) {
    if (!knn_clean(a.status)) return;
    const int lane = threadIdx.x & 63;
    const long long i = (long long)blockIdx.x * (kKnnBlock / TKR_WAVE) + (threadIdx.x >> 6);
    if (i >= a.n_items) return;                                   // (a whole wave)
    const long long lo = a.i_ptr[i], hi = a.i_ptr[i + 1];
    long long work = 0;
    for (long long e = lo + lane; e < hi; e += TKR_WAVE) {
        const int u = a.i_rows[e];
        work += a.u_ptr[u + 1] - a.u_ptr[u];
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) work += __shfl_xor(work, o, TKR_WAVE);
    if (lane == 0) {
        int p = 0;
        if (work > a.heavy_from) {
            const long long by_work = (work + a.heavy_from - 1) / a.heavy_from;
            p = (int)max(1ll, min((long long)kKnnMaxParts, min(hi - lo, by_work)));
            a.heavy_list[atomicAdd(a.n_heavy, 1u)] = (int)i;
        }
        a.parts[i] = p;
    }
}

// the likers i_rows[e0 .. e1) of one item: for each, the columns of its list that lie in the slab, counted in LDS.  A wave loads the
// list ends of 64 likers side by side and then takes their lists one by one, the lanes along the list.
__device__ __forceinline__ void knn_count_likers(const KnnBuild& a, long long e0, long long e1, unsigned int* cnt, uint32_t base, uint32_t n) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (long long b0 = e0 + (long long)wave * TKR_WAVE; b0 < e1; b0 += kKnnBlock) {
        long long lo = 0, len = 0;
        if (b0 + lane < e1) {
            const int u = a.i_rows[b0 + lane];
            lo = a.u_ptr[u];
            len = a.u_ptr[u + 1] - lo;
        }
        const int m = (int)min((long long)TKR_WAVE, e1 - b0);
        for (int q = 0; q < m; ++q) {
            const long long qlo = __shfl(lo, q, TKR_WAVE), qlen = __shfl(len, q, TKR_WAVE);
            for (long long x = lane; x < qlen; x += TKR_WAVE) {
                const uint32_t rel = (uint32_t)a.u_cols[qlo + x] - base;
                if (rel < n) __hip_atomic_fetch_add(&cnt[rel], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
            }
        }
    }
}

__device__ __forceinline__ uint32_t knn_sim_key(uint32_t c, double ni, double nj, double shrink) {
    double den = ni * nj;                                         // rounded
    den = den + shrink;                                           // rounded
    const float s = (float)((double)c / den);                     // one division, one rounding to fp32
    return __float_as_uint(s) | 0x80000000u;                      // s >= +0.0: its bits are ordered, and the key of a candidate is never 0
}

// the row of item i from its counters: FROM_ROW = false counts the likers here, true reads (and clears) the row the parts added up
template <bool FROM_ROW>
__device__ __forceinline__ void knn_row(const KnnBuild& a, int i, unsigned int* row, unsigned char* lds) {
    const int P = knn_sort_width(a.N), tid = threadIdx.x;
    uint64_t* cand = reinterpret_cast<uint64_t*>(lds);
    uint32_t* hist = reinterpret_cast<uint32_t*>(lds + (size_t)P * 8);
    uint32_t* ctl = hist + 256;
    uint32_t* keys = hist + kKnnHeadWords;
    for (int t = tid; t < a.N; t += kKnnBlock) cand[t] = 0ull;
    const double ni = a.norm[i];
    const long long e0 = a.i_ptr[i], e1 = a.i_ptr[i + 1];
    for (int base = 0; base < a.n_items; base += a.slab) {
        const int n = min(a.slab, a.n_items - base);
        if (FROM_ROW) {
            for (int j = tid; j < n; j += kKnnBlock) {
                keys[j] = row[base + j];
                row[base + j] = 0u;
            }
        } else {
            for (int j = tid; j < n; j += kKnnBlock) keys[j] = 0u;
            __syncthreads();
            knn_count_likers(a, e0, e1, keys, (uint32_t)base, (uint32_t)n);
        }
        __syncthreads();
        for (int j = tid; j < n; j += kKnnBlock) {
            const uint32_t c = keys[j];
            if (c != 0u) keys[j] = (base + j != i) ? knn_sim_key(c, ni, a.norm[base + j], a.shrink) : 0u;
        }
        __syncthreads();
        knn_select_into<kKnnBlock>(keys, n, (uint32_t)base, (uint32_t)a.n_items, a.N, cand, P, hist, ctl);
    }
    for (int t = tid; t < a.N; t += kKnnBlock) {
        const uint64_t pair = cand[t];
        a.nbr_ids[(size_t)i * a.N + t] = pair ? (int32_t)(uint32_t)pair : -1;
        a.nbr_w[(size_t)i * a.N + t] = pair ? __uint_as_float((uint32_t)(pair >> 32) & 0x7fffffffu) : 0.f;
    }
}

__global__ __launch_bounds__(kKnnBlock) void knn_light_kernel(KnnBuild a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char knn_lds[];
    if (!knn_clean(a.status)) return;
    const int i = blockIdx.x;
    if (a.parts[i] != 0) return;
    knn_row<false>(a, i, nullptr, knn_lds);
}

__global__ __launch_bounds__(kKnnBlock) void knn_partial_kernel(KnnBuild a, int batch) {
    extern __shared__ __attribute__((aligned(16))) unsigned char knn_lds[];
    if (!knn_clean(a.status)) return;
    const long long slot = (long long)batch * a.rows + blockIdx.x;
    if (slot >= (long long)*a.n_heavy) return;
    const int i = a.heavy_list[slot], parts = a.parts[i], p = blockIdx.y;
    if (p >= parts) return;
    const long long lo = a.i_ptr[i], likers = a.i_ptr[i + 1] - lo;
    const long long e0 = lo + likers * p / parts, e1 = lo + likers * (p + 1) / parts;
    unsigned int* cnt = reinterpret_cast<unsigned int*>(knn_lds);
    unsigned int* row = a.part_rows + (size_t)blockIdx.x * a.pitch;
    const int tid = threadIdx.x;
    for (int base = 0; base < a.n_items; base += a.slab) {
        const int n = min(a.slab, a.n_items - base);
        for (int j = tid; j < n; j += kKnnBlock) cnt[j] = 0u;
        __syncthreads();
        knn_count_likers(a, e0, e1, cnt, (uint32_t)base, (uint32_t)n);
        __syncthreads();
        for (int j = tid; j < n; j += kKnnBlock) {
            const unsigned int v = cnt[j];
            if (v) __hip_atomic_fetch_add(&row[base + j], v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
        __syncthreads();
    }
}

__global__ __launch_bounds__(kKnnBlock) void knn_finish_kernel(KnnBuild a, int batch) {
    extern __shared__ __attribute__((aligned(16))) unsigned char knn_lds[];
    if (!knn_clean(a.status)) return;
    const long long slot = (long long)batch * a.rows + blockIdx.x;
    if (slot >= (long long)*a.n_heavy) return;
    knn_row<true>(a, a.heavy_list[slot], a.part_rows + (size_t)blockIdx.x * a.pitch, knn_lds);
}

// ---- K29 --------------------------------------------------------------------------------------------------------------------------
struct KnnScore {
    const int64_t* hist_ptr;
    const int32_t* hist_cols;
    const int32_t* nbr_ids;
    const float* nbr_w;
    const int32_t* col_of_item;
    const uint32_t* mask;
    const int64_t* like_ptr;
    const int32_t* like_cols;
    long long n_hist, n_likes, n_rows;
    int n_items, N, n_cols, mask_pitch, K, slab;
    int32_t* out_ids;
    float* out_scores;
    int32_t* rank_out;
    unsigned long long* status;
};

__global__ __launch_bounds__(kKnnBlock) void knn_score_check_kernel(KnnScore a, long long total) {
    const long long h_end = a.hist_ptr[a.n_rows], h_n = (h_end >= 0 && h_end <= a.n_hist) ? h_end : 0;
    for (long long t = (long long)blockIdx.x * kKnnBlock + threadIdx.x; t < total; t += (long long)gridDim.x * kKnnBlock) {
        if (t <= a.n_rows) {
            const long long v = a.hist_ptr[t];
            bool bad = v < 0 || v > a.n_hist || (t == 0 && v != 0);
            if (t < a.n_rows) bad = bad || a.hist_ptr[t + 1] < v;
            if (bad) status_refuse(a.status, t, kKnnScoreBadPtr);
            if (a.like_ptr) {
                const long long w = a.like_ptr[t];
                bool lbad = w < 0 || w > a.n_likes || (t == 0 && w != 0);
                if (t < a.n_rows) lbad = lbad || a.like_ptr[t + 1] < w;
                if (lbad) status_refuse(a.status, t, kKnnScoreBadLikePtr);
            }
        }
        if (t < h_n && (uint32_t)a.hist_cols[t] >= (uint32_t)a.n_items) status_refuse(a.status, t, kKnnScoreBadCol);
    }
}

// the accumulators of the slab [base, base + n) for line r, then their keys.  The chain of a column runs over the history in stored
// order: the FIRST wave alone walks it, the lanes along the neighbour list of one history item, kKnnAhead list pieces loaded (ids,
// weights, then the mapped columns) ahead of their adds; the workgroup's other waves clear and convert with it
__device__ __forceinline__ void knn_accumulate(const KnnScore& a, long long r, long long hlo, long long hhi, int base, int n, uint32_t* keys) {
    const int tid = threadIdx.x;
    float* acc = reinterpret_cast<float*>(keys);
    __syncthreads();                                              // whoever read the keys of the slab before is done
    for (int j = tid; j < n; j += kKnnBlock) acc[j] = 0.f;
    __syncthreads();
    if (tid < TKR_WAVE) {
        const int lane = tid;
        const int nch = (a.N + TKR_WAVE - 1) / TKR_WAVE;          // pieces of 64 neighbours per history item
        const long long steps = (hhi - hlo) * nch;
        for (long long t0 = 0; t0 < steps; t0 += kKnnAhead) {
            int32_t id[kKnnAhead], col[kKnnAhead];
            float w[kKnnAhead];
#pragma unroll
            for (int u = 0; u < kKnnAhead; ++u) {
                const long long t = t0 + u;
                id[u] = -1;
                w[u] = 0.f;
                if (t < steps) {
                    const long long h = t / nch;
                    const int p = (int)(t - h * nch) * TKR_WAVE + lane;
                    if (p < a.N) {
                        const size_t at = (size_t)a.hist_cols[hlo + h] * a.N + p;
                        id[u] = a.nbr_ids[at];
                        w[u] = a.nbr_w[at];
                    }
                }
            }
#pragma unroll
            for (int u = 0; u < kKnnAhead; ++u) {                 // an id outside [0, n_items) (the -1 padding, a broken table) names nothing
                col[u] = -1;
                if ((uint32_t)id[u] < (uint32_t)a.n_items) col[u] = a.col_of_item ? a.col_of_item[id[u]] : id[u];
            }
#pragma unroll
            for (int u = 0; u < kKnnAhead; ++u) {
                const uint32_t rel = (uint32_t)col[u] - (uint32_t)base;
                if (col[u] >= 0 && rel < (uint32_t)n) acc[rel] = acc[rel] + w[u];
                __builtin_amdgcn_wave_barrier();                  // the adds of one piece stay in front of the next piece's
            }
        }
    }
    __syncthreads();
    for (int j = tid; j < n; j += kKnnBlock) {
        const int c = base + j;
        const bool masked = a.mask && ((a.mask[(size_t)(c >> 5) * a.mask_pitch + r] >> (c & 31)) & 1u);
        float s = acc[j];
        if (s == 0.f) s = 0.f;                                    // -0.0 -> +0.0
        keys[j] = masked ? 0u : rank_bits(s);                     // never 0 for a kept column
    }
    __syncthreads();
}

__global__ __launch_bounds__(kKnnBlock) void knn_score_kernel(KnnScore a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char knn_lds[];
    if (!knn_clean(a.status)) return;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const long long r = blockIdx.x;
    const int want = a.out_ids ? a.K : 0, P = knn_sort_width(max(want, 1));
    uint64_t* cand = reinterpret_cast<uint64_t*>(knn_lds);
    uint32_t* hist = reinterpret_cast<uint32_t*>(knn_lds + (size_t)P * 8);
    uint32_t* ctl = hist + 256;
    uint32_t* lkey = hist + kKnnHeadWords;                        // [kKnnBlock]: the keys of a chunk of likes, 0 = no rank
    uint32_t* lcnt = lkey + kKnnBlock;                            // [kKnnBlock]: the pairs in front of each
    uint32_t* keys = lcnt + kKnnBlock;
    const long long hlo = a.hist_ptr[r], hhi = a.hist_ptr[r + 1];
    const long long llo = a.rank_out ? a.like_ptr[r] : 0, lhi = a.rank_out ? a.like_ptr[r + 1] : 0;
    const int n_slabs = (a.n_cols + a.slab - 1) / a.slab;
    for (int t = tid; t < P; t += kKnnBlock) cand[t] = 0ull;
    if (want) {
        for (int s = 0; s < n_slabs; ++s) {
            const int base = s * a.slab, n = min(a.slab, a.n_cols - base);
            knn_accumulate(a, r, hlo, hhi, base, n, keys);
            knn_select_into<kKnnBlock>(keys, n, (uint32_t)base, (uint32_t)a.n_cols, want, cand, P, hist, ctl);
        }
        if (tid < want) {
            const uint64_t pair = cand[tid];
            a.out_ids[(size_t)r * a.K + tid] = pair ? (int32_t)(uint32_t)pair : -1;
            if (a.out_scores) a.out_scores[(size_t)r * a.K + tid] = pair ? unordered_bits((uint32_t)(pair >> 32)) : -INFINITY;
        }
    } else if (n_slabs == 1 && lhi > llo) {
        knn_accumulate(a, r, hlo, hhi, 0, a.n_cols, keys);
    }
    // the ranks, kKnnBlock likes at a time.  One slab: its keys are still in LDS.  More: the history is walked again, once per slab to
    // fetch the likes' keys and once per slab to count
    for (long long c0 = llo; c0 < lhi; c0 += kKnnBlock) {
        const int m = (int)min((long long)kKnnBlock, lhi - c0);
        __syncthreads();
        lkey[tid] = 0u;
        lcnt[tid] = 0u;
        __syncthreads();
        for (int s = 0; s < n_slabs; ++s) {
            const int base = s * a.slab, n = min(a.slab, a.n_cols - base);
            if (n_slabs > 1) knn_accumulate(a, r, hlo, hhi, base, n, keys);
            if (tid < m) {                                        // a like outside [0, n_cols) is in no slab: its key stays 0
                const uint32_t rel = (uint32_t)a.like_cols[c0 + tid] - (uint32_t)base;
                if (rel < (uint32_t)n) lkey[tid] = keys[rel];
            }
            __syncthreads();
        }
        for (int s = 0; s < n_slabs; ++s) {
            const int base = s * a.slab, n = min(a.slab, a.n_cols - base);
            if (n_slabs > 1) knn_accumulate(a, r, hlo, hhi, base, n, keys);
            for (int x = wave; x < m; x += kKnnBlock / TKR_WAVE) {    // a wave per like, its lanes along the columns
                const uint32_t kl = lkey[x];
                if (kl == 0u) continue;                           // (the whole wave) masked or out of range
                const uint64_t like = ((uint64_t)kl << 32) | (uint64_t)(uint32_t)a.like_cols[c0 + x];
                uint32_t front = 0;
                for (int j0 = 0; j0 < n; j0 += TKR_WAVE) {
                    const int j = j0 + lane;
                    const uint32_t k = j < n ? keys[j] : 0u;
                    const uint64_t pair = ((uint64_t)k << 32) | (uint64_t)(uint32_t)(base + j);
                    front += (uint32_t)__popcll(__ballot(k != 0u && pair > like));
                }
                if (lane == 0) lcnt[x] += front;                  // like x is this wave's alone
            }
            __syncthreads();
        }
        if (tid < m) a.rank_out[c0 + tid] = lkey[tid] ? (int32_t)lcnt[tid] : -1;
    }
}

template <typename Kern>
static int knn_allow_lds(Kern kern, size_t lds) {
    if (lds > 64 * 1024)
        TKR_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)kKnnLdsBudget));
    return TKR_OK;
}

static int knn_check_grid(long long total) { return (int)std::min<long long>((total + kKnnBlock - 1) / kKnnBlock, 1 << 20); }

static long long knn_batch_rows(long long n_items) { return std::min<long long>(n_items, std::max<long long>(64, (n_items + 31) / 32)); }
static long long knn_align16(long long b) { return (b + 15) & ~15ll; }

}  // namespace tkr

extern "C" int64_t tkr_knn_build_workspace_bytes(int64_t n_items) {
    if (n_items < 1 || n_items > INT_MAX) return TKR_EINVAL;
    const long long pitch = (n_items + 3) & ~3ll;
    return 16 + 2 * tkr::knn_align16(n_items * 4) + tkr::knn_batch_rows(n_items) * pitch * 4;
}

extern "C" int tkr_knn_build(const int64_t* u_ptr, const int32_t* u_cols, int64_t n_u_entries, const int64_t* i_ptr, const int32_t* i_rows,
                             int64_t n_i_entries, int64_t n_users, int64_t n_items, const double* norm, double shrink, int32_t N,
                             int64_t heavy_from, int32_t slab_cols, int32_t* nbr_ids, float* nbr_w, void* workspace, int64_t workspace_bytes,
                             int64_t* status, void* stream_) {
    using namespace tkr;
    if (!u_ptr || !i_ptr || !norm || !nbr_ids || !nbr_w || !workspace || !status) return TKR_EINVAL;
    if (((uintptr_t)u_ptr | (uintptr_t)i_ptr | (uintptr_t)norm | (uintptr_t)status) & 7) return TKR_EINVAL;
    if (((uintptr_t)u_cols | (uintptr_t)i_rows | (uintptr_t)nbr_ids | (uintptr_t)nbr_w) & 3) return TKR_EINVAL;
    if ((uintptr_t)workspace & 15) return TKR_EINVAL;
    if (n_u_entries < 0 || n_i_entries < 0 || (n_u_entries > 0 && !u_cols) || (n_i_entries > 0 && !i_rows)) return TKR_EINVAL;
    if (n_users < 1 || n_items < 1 || n_users >= INT_MAX || n_items >= INT_MAX) return TKR_EINVAL;
    if (!(shrink >= 0.0 && shrink < INFINITY) || heavy_from < 0 || slab_cols < 0) return TKR_EINVAL;
    if (N < 1 || N > TKR_KNN_MAX_N || slab_cols > TKR_KNN_MAX_SLAB) return TKR_EUNSUPPORTED;
    if (workspace_bytes < tkr_knn_build_workspace_bytes(n_items)) return TKR_EINVAL;
    hipStream_t stream = (hipStream_t)stream_;

    KnnBuild a;
    a.u_ptr = u_ptr; a.u_cols = u_cols; a.i_ptr = i_ptr; a.i_rows = i_rows; a.norm = norm;
    a.n_u_entries = n_u_entries; a.n_i_entries = n_i_entries;
    a.n_users = (int)n_users; a.n_items = (int)n_items; a.N = N;
    a.slab = (int)std::min<long long>(slab_cols ? slab_cols : TKR_KNN_MAX_SLAB, n_items);
    a.rows = (int)knn_batch_rows(n_items);
    a.pitch = (int)((n_items + 3) & ~3ll);
    a.shrink = shrink;
    a.heavy_from = heavy_from ? heavy_from : TKR_KNN_HEAVY_FROM;
    unsigned char* ws = static_cast<unsigned char*>(workspace);
    a.n_heavy = reinterpret_cast<unsigned int*>(ws);
    a.parts = reinterpret_cast<int32_t*>(ws + 16);
    a.heavy_list = reinterpret_cast<int32_t*>(ws + 16 + knn_align16(n_items * 4));
    a.part_rows = reinterpret_cast<unsigned int*>(ws + 16 + 2 * knn_align16(n_items * 4));
    a.nbr_ids = nbr_ids; a.nbr_w = nbr_w;
    a.status = reinterpret_cast<unsigned long long*>(status);

    const int P = knn_sort_width(N);
    const size_t lds = (size_t)P * 8 + (size_t)kKnnHeadWords * 4 + (size_t)a.slab * 4, lds_part = (size_t)a.slab * 4;
    TKR_CHECK_RC(knn_allow_lds(knn_light_kernel, lds));
    TKR_CHECK_RC(knn_allow_lds(knn_finish_kernel, lds));
    TKR_CHECK_RC(knn_allow_lds(knn_partial_kernel, lds_part));
    TKR_CHECK(hipMemsetAsync(a.status, 0xff, sizeof(unsigned long long), stream));     // -1: nothing refused
    TKR_CHECK(hipMemsetAsync(a.n_heavy, 0, 16, stream));
    TKR_CHECK(hipMemsetAsync(a.part_rows, 0, (size_t)a.rows * a.pitch * 4, stream));
    const long long total = std::max(std::max<long long>(n_users, n_items) + 1, std::max<long long>(n_u_entries, n_i_entries));
    hipLaunchKernelGGL(knn_check_kernel, dim3(knn_check_grid(total)), dim3(kKnnBlock), 0, stream, a, total);
    TKR_LAUNCH_CHECK();
    hipLaunchKernelGGL(knn_plan_kernel, dim3((unsigned)((n_items + 3) / 4)), dim3(kKnnBlock), 0, stream, a);
    TKR_LAUNCH_CHECK();
    hipLaunchKernelGGL(knn_light_kernel, dim3((unsigned)n_items), dim3(kKnnBlock), lds, stream, a);
    TKR_LAUNCH_CHECK();
    // the heavy items, as many at a time as the workspace has rows; a batch past the end of the list finds nothing to do
    const int batches = (int)((n_items + a.rows - 1) / a.rows);
    for (int b = 0; b < batches; ++b) {
        hipLaunchKernelGGL(knn_partial_kernel, dim3(a.rows, kKnnMaxParts), dim3(kKnnBlock), lds_part, stream, a, b);
        TKR_LAUNCH_CHECK();
        hipLaunchKernelGGL(knn_finish_kernel, dim3(a.rows), dim3(kKnnBlock), lds, stream, a, b);
        TKR_LAUNCH_CHECK();
    }
    return TKR_OK;
}

extern "C" int tkr_knn_score(const int64_t* hist_ptr, const int32_t* hist_cols, int64_t n_hist, int64_t n_rows, const int32_t* nbr_ids,
                             const float* nbr_w, int32_t n_items, int32_t N, const int32_t* col_of_item, int32_t n_cols, const uint32_t* mask,
                             int32_t mask_pitch, int32_t K, int32_t* out_ids, float* out_scores, const int64_t* like_ptr,
                             const int32_t* like_cols, int64_t n_likes, int32_t* rank_out, int32_t slab_cols, int64_t* status, void* stream_) {
    using namespace tkr;
    if (!hist_ptr || !nbr_ids || !nbr_w || !status) return TKR_EINVAL;
    if (((uintptr_t)hist_ptr | (uintptr_t)like_ptr | (uintptr_t)status) & 7) return TKR_EINVAL;
    if (n_hist < 0 || (n_hist > 0 && !hist_cols) || n_rows < 1 || n_rows >= INT_MAX) return TKR_EINVAL;
    if (n_items < 1 || n_cols < 1 || N < 1 || slab_cols < 0) return TKR_EINVAL;
    if (!col_of_item && n_cols != n_items) return TKR_EINVAL;
    if (mask && mask_pitch < n_rows) return TKR_EINVAL;
    if (!out_ids && (out_scores || !rank_out)) return TKR_EINVAL;                      // lists, ranks or both
    if (out_ids && K < 1) return TKR_EINVAL;
    if ((like_ptr != nullptr) != (rank_out != nullptr) || n_likes < 0 || (!like_ptr && (like_cols || n_likes)) ||
        (like_ptr && n_likes > 0 && !like_cols))
        return TKR_EINVAL;
    if (N > TKR_KNN_MAX_N || (out_ids && K > TKR_KNN_MAX_K) || slab_cols > TKR_KNN_MAX_SLAB) return TKR_EUNSUPPORTED;
    hipStream_t stream = (hipStream_t)stream_;

    KnnScore a;
    a.hist_ptr = hist_ptr; a.hist_cols = hist_cols; a.nbr_ids = nbr_ids; a.nbr_w = nbr_w; a.col_of_item = col_of_item; a.mask = mask;
    a.like_ptr = like_ptr; a.like_cols = like_cols;
    a.n_hist = n_hist; a.n_likes = n_likes; a.n_rows = n_rows;
    a.n_items = n_items; a.N = N; a.n_cols = n_cols; a.mask_pitch = mask_pitch; a.K = out_ids ? K : 0;
    a.slab = std::min(slab_cols ? slab_cols : TKR_KNN_MAX_SLAB, n_cols);
    a.out_ids = out_ids; a.out_scores = out_scores; a.rank_out = rank_out;
    a.status = reinterpret_cast<unsigned long long*>(status);

    const int P = knn_sort_width(std::max(a.K, 1));
    const size_t lds = (size_t)P * 8 + (size_t)(kKnnHeadWords + 2 * kKnnBlock) * 4 + (size_t)a.slab * 4;
    TKR_CHECK_RC(knn_allow_lds(knn_score_kernel, lds));
    TKR_CHECK(hipMemsetAsync(a.status, 0xff, sizeof(unsigned long long), stream));
    const long long total = std::max<long long>(n_rows + 1, n_hist);
    hipLaunchKernelGGL(knn_score_check_kernel, dim3(knn_check_grid(total)), dim3(kKnnBlock), 0, stream, a, total);
    TKR_LAUNCH_CHECK();
    hipLaunchKernelGGL(knn_score_kernel, dim3((unsigned)n_rows), dim3(kKnnBlock), lds, stream, a);
    TKR_LAUNCH_CHECK();
    return TKR_OK;
}
