// K6 / K7 -- the rank walk of utils.evaluate (utils.py:101-127) on top of K4's filtered lists.
//
// utils.evaluate differs from the CLI's walk (evaluate.py:96-105) in two ways: a hit is bucketed by the item's
// RAW rank t (train-rated items included, utils.py:113-117: j = t // step) and reciprocal ranks 1/(t+1) are
// summed next to the hit counts.  K4 yields the first `total` unrated columns of a user in order; the raw rank of
// the p-th of them is p + (number of the user's train-rated columns ranked before it).  K6 computes exactly that
// count: one wave per row; a lane takes one column, kept or rated, and runs the library's ONE fp32 score chain over it
// (exact_score, csrc/score_chain.h: the bits K4 ranked the kept list by, at any factor width), then the wave counts,
// for every kept column, the rated ones in front of it under the canonical order (descending score, ties -> higher
// column first).  K7 turns (kept ids, raw ranks, like lists) into per-row first-bucket hit counts and
// reciprocal-rank sums; the host sums rows and accumulates buckets (utils.py:115-117: for k in range(j, interval)).
//
// Integer/byte work bound by the row gathers of Vt: (n_rated + total) rows of k floats per user, every lane its own.
#include "tkr_common.h"
#include "topk_parts.h"
#include "../../include/tkr.h"

namespace tkr {

constexpr int kRawMaxK = 256;      // kept columns per row a launch handles
constexpr int kRawSlots = kRawMaxK / 64;      // ... kept in registers: position lane + 64 i belongs to lane

__global__ __launch_bounds__(256) void raw_rank_kernel(const float* __restrict__ U, const int32_t* __restrict__ uidx,
                                                       int n_rows, const float* __restrict__ Vt,
                                                       const float* __restrict__ bias, int k,
                                                       const int64_t* __restrict__ rated_ptr,
                                                       const int32_t* __restrict__ rated_cols,
                                                       const int32_t* __restrict__ ids, int K,
                                                       int32_t* __restrict__ raw_rank) {
    const int lane = threadIdx.x & 63;
    const int r = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (r >= n_rows) return;
    const float* up = U + (size_t)(uidx ? uidx[r] : r) * k;
    // kept columns: the scores K4 ordered them by
    int cp[kRawSlots], before[kRawSlots];
    uint32_t sp[kRawSlots];                                      // rank_bits: K4's order over every fp32 value, every NaN one score above +inf
#pragma unroll
    for (int i = 0; i < kRawSlots; ++i) {
        const int p = lane + 64 * i;
        cp[i] = p < K ? ids[(size_t)r * K + p] : -1;
        sp[i] = 0u;
        before[i] = 0;
        if (cp[i] >= 0) sp[i] = rank_bits(exact_score(up, Vt + (size_t)cp[i] * k, k, bias, cp[i]));
    }
    // rated columns, 64 at a time: lane j scores one, every lane compares it with its kept columns
    const int64_t q1 = rated_ptr[r + 1];
    for (int64_t q0 = rated_ptr[r]; q0 < q1; q0 += 64) {
        const int n = (int)min((int64_t)64, q1 - q0);
        int c = -1;
        uint32_t s = 0u;
        if (lane < n) {
            c = rated_cols[q0 + lane];
            s = rank_bits(exact_score(up, Vt + (size_t)c * k, k, bias, c));
        }
        for (int j = 0; j < n; ++j) {
            const int cj = __shfl(c, j, 64);
            const uint32_t sj = (uint32_t)__shfl((int)s, j, 64);
#pragma unroll
            for (int i = 0; i < kRawSlots; ++i)
                if (cp[i] >= 0 && (sj > sp[i] || (sj == sp[i] && cj > cp[i]))) before[i] += 1;
        }
    }
#pragma unroll
    for (int i = 0; i < kRawSlots; ++i) {
        const int p = lane + 64 * i;
        if (p < K) raw_rank[(size_t)r * K + p] = cp[i] >= 0 ? p + before[i] : -1;
    }
}

// one thread per row: sequential over the kept positions, so the reciprocal-rank sums are reproducible
__global__ void count_hits_rr_kernel(const int32_t* __restrict__ ids, const int32_t* __restrict__ raw_rank, int n_rows, int K,
                                     const int64_t* __restrict__ like_ptr, const int32_t* __restrict__ like_cols, int step,
                                     int interval, int32_t* __restrict__ hit_first, double* __restrict__ rr_first) {
    const int r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= n_rows) return;
    const int64_t lo0 = like_ptr[r], hi0 = like_ptr[r + 1];
    for (int p = 0; p < K; ++p) {
        const int c = ids[(size_t)r * K + p];
        if (c < 0) break;
        int64_t lo = lo0, hi = hi0;
        while (lo < hi) {
            const int64_t mid = (lo + hi) >> 1;
            if (like_cols[mid] < c) lo = mid + 1; else hi = mid;
        }
        if (lo < hi0 && like_cols[lo] == c) {
            const int t = raw_rank[(size_t)r * K + p];
            const int j = t / step;
            if (j < interval) {
                hit_first[(size_t)r * interval + j] += 1;
                rr_first[(size_t)r * interval + j] += 1.0 / (double)(t + 1);
            }
        }
    }
}

}  // namespace tkr

extern "C" int tkr_raw_ranks(const float* U, const int32_t* user_idx, int32_t n_rows, const float* Vt, const float* bias,
                             int32_t k, const int64_t* rated_ptr, const int32_t* rated_cols, const int32_t* ids, int32_t K,
                             int32_t* raw_rank, void* stream) {
    if (!U || !Vt || !rated_ptr || !ids || !raw_rank || n_rows <= 0 || k <= 0 || K <= 0) return TKR_EINVAL;
    if (K > tkr::kRawMaxK) return TKR_EUNSUPPORTED;
    hipLaunchKernelGGL(tkr::raw_rank_kernel, dim3((n_rows + 3) / 4), dim3(256), 0, (hipStream_t)stream, U, user_idx, n_rows, Vt, bias, k,
                       rated_ptr, rated_cols, ids, K, raw_rank);
    TKR_LAUNCH_CHECK();
    return TKR_OK;
}

extern "C" int tkr_count_hits_rr(const int32_t* ids, const int32_t* raw_rank, int32_t n_rows, int32_t K,
                                 const int64_t* like_ptr, const int32_t* like_cols, int32_t step, int32_t interval,
                                 int32_t* hit_first, double* rr_first, void* stream) {
    if (!ids || !raw_rank || !like_ptr || !hit_first || !rr_first || n_rows <= 0 || K <= 0 || step <= 0 || interval <= 0)
        return TKR_EINVAL;
    hipLaunchKernelGGL(tkr::count_hits_rr_kernel, dim3((n_rows + 255) / 256), dim3(256), 0, (hipStream_t)stream, ids, raw_rank,
                       n_rows, K, like_ptr, like_cols, step, interval, hit_first, rr_first);
    TKR_LAUNCH_CHECK();
    return TKR_OK;
}
