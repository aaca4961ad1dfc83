// The wave-per-row step of K25 (csrc/lmf.hip) and K27 (csrc/smf.hip), written ONCE: the sum over a row's likes, the gradient, AdaGrad in
// place and the row's loss terms, for a light row (one wave) and a heavy one (a workgroup of 16 waves over slabs of likes).  MODE says
// what a like weighs and what the gradient is made of; everything else -- the order of every chain, the refusals, the heavy rows' tree --
// is the same code.
//   kLmfLogistic   L = sum_likes (1 - sigma(s)) y,  g = weight * L - D - lam x        (weight: alpha, the weight of a like)
//   kSmfUnit       L = sum_likes y,                 g = L - D - lam x
//   kSmfByLikes    L = sum_likes y,                 g = L - n D - lam x               (n: the likes the row stores, hi - lo)
// Behind the kernels, lmf_step_entry: the host side of both step calls.
#pragma once
#include "lmf_parts.h"

#include <math.h>

#include <algorithm>

namespace tkr {

enum { kLmfLogistic = 0, kSmfUnit = 1, kSmfByLikes = 2 };

// what a wave holds of a sum over likes: L (element j in lane j & 63, register j >> 6) and the two sums of the loss (the same in every lane)
template <int NR>
struct LmfSum {
    float L[NR];
    double sp, ss;
};

template <int NR>
__device__ __forceinline__ void lmf_load_row(const float* __restrict__ row, int K, float (&v)[NR]) {
    const int lane = threadIdx.x & 63;
#pragma unroll
    for (int j = 0; j < NR; ++j) v[j] = lane + 64 * j < K ? row[lane + 64 * j] : 0.f;
}

// the likes cols[first .. first + count) against the row x: an fp32 chain per component from +0.0 in stored order.  A column outside
// [0, n_y) is skipped; -> whether one was.  Called by a whole wave with the same arguments.  (K27: a like weighs 1 and sp stays 0.)
template <int NR, int MODE>
__device__ __forceinline__ bool lmf_like_chain(const float* __restrict__ Y, int n_y, int K, const int32_t* __restrict__ cols, long long first, int count,
                                               const float (&x)[NR], LmfSum<NR>& sum) {
    const int lane = threadIdx.x & 63;
#pragma unroll
    for (int j = 0; j < NR; ++j) sum.L[j] = 0.f;
    sum.sp = sum.ss = 0.0;
    bool skipped = false;
    for (int base = 0; base < count; base += TKR_WAVE) {          // wave-uniform
        const int n_here = min(TKR_WAVE, count - base);
        int mine = -1;
        if (lane < n_here) {
            mine = cols[first + base + lane];
            if ((uint32_t)mine >= (uint32_t)n_y) {
                mine = -1;
                skipped = true;
            }
        }
        for (int i = 0; i < n_here; ++i) {
            const int c = bcast_i(mine, i);
            if (c < 0) continue;                                  // (uniform)
            float y[NR];
            lmf_load_row<NR>(Y + (size_t)c * K, K, y);
            float d = 0.f;
#pragma unroll
            for (int j = 0; j < NR; ++j) d = fmaf(x[j], y[j], d);
            const float s = wave_sum(d);
            if constexpr (MODE == kLmfLogistic) {
                const float w = lmf_sigmoid(-s);                  // 1 - sigma(s)
#pragma unroll
                for (int j = 0; j < NR; ++j) sum.L[j] = fmaf(w, y[j], sum.L[j]);
                sum.sp += (double)lmf_softplus(s);
            } else {
#pragma unroll
                for (int j = 0; j < NR; ++j) sum.L[j] += y[j];
            }
            sum.ss += (double)s;
        }
    }
    return __ballot(skipped) != 0ull;
}

__device__ __forceinline__ double lmf_wave_sum_f64(double v) {    // a fixed tree: v += v(lane ^ 32), ^ 16, .. ^ 1
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d);
    return v;
}

// the gradient, AdaGrad in place and the row's loss terms; x: the row as it came in, sum: over its likes.  One wave.  weight: alpha
// (K25), or what D is multiplied by (K27); fixed = -1 names no column.
template <int NR, int MODE>
__device__ __forceinline__ void lmf_update_row(long long r, int K, int fixed, const float (&x)[NR], const LmfSum<NR>& sum, const float* __restrict__ D,
                                               double weight, double lam, float lr, float* __restrict__ X, float* __restrict__ H,
                                               double* __restrict__ row_loss) {
    const int lane = threadIdx.x & 63;
    double sq = 0.0;
#pragma unroll
    for (int j = 0; j < NR; ++j) {
        const int col = lane + 64 * j;
        if (col < K && col != fixed) {
            const size_t at = (size_t)r * K + col;
            float g;                                              // three terms in fp64, rounded once
            if constexpr (MODE == kLmfLogistic)
                g = (float)(weight * (double)sum.L[j] - (double)D[at] - lam * (double)x[j]);
            else
                g = (float)((double)sum.L[j] - weight * (double)D[at] - lam * (double)x[j]);
            const float hn = fmaf(g, g, H[at]);
            H[at] = hn;
            X[at] = x[j] + (lr * g) / sqrtf(hn);
            sq += (double)x[j] * (double)x[j];
        }
    }
    if (row_loss) {
        sq = lmf_wave_sum_f64(sq);
        if constexpr (MODE == kLmfLogistic) {
            if (lane == 0) row_loss[r] = weight * sum.sp - weight * sum.ss + 0.5 * lam * sq;
        } else {
            if (lane == 0) row_loss[r] = 0.5 * lam * sq - sum.ss;
        }
    }
}

template <int NR, int MODE>
__global__ __launch_bounds__(kLmfBlock) void lmf_step_kernel(const float* __restrict__ Y, int n_y, int K, const float* __restrict__ D,
                                                             const int64_t* __restrict__ like_ptr, const int32_t* __restrict__ like_cols,
                                                             long long n_likes, long long n_x, int fixed, double weight, double lam, float lr,
                                                             long long heavy_from, float* __restrict__ X, float* __restrict__ H,
                                                             double* __restrict__ row_loss, unsigned long long* __restrict__ status,
                                                             int32_t* __restrict__ heavy_count, int32_t* __restrict__ heavy_list) {
    const int lane = threadIdx.x & 63;
    const long long r = (long long)blockIdx.x * kLmfWaves + (threadIdx.x >> 6);
    if (r >= n_x) return;                                         // (wave-uniform, as every exit below: no barrier in this kernel)
    const long long lo = like_ptr[r], hi = like_ptr[r + 1];
    if (!als_ptr_ok(lo, hi, n_likes, r)) {
        if (lane == 0) {
            status_refuse(status, r, kAlsBadPtr);                 // the row is left as it is
            if (row_loss) row_loss[r] = 0.0;
        }
        return;
    }
    if (hi - lo > heavy_from && heavy_list) {
        if (lane == 0) heavy_list[atomicAdd(heavy_count, 1)] = (int32_t)r;
        return;
    }
    float x[NR];
    lmf_load_row<NR>(X + (size_t)r * K, K, x);
    LmfSum<NR> sum;
    if (lmf_like_chain<NR, MODE>(Y, n_y, K, like_cols, lo, (int)(hi - lo), x, sum) && lane == 0)
        status_refuse(status, r, kAlsSkipped);
    lmf_update_row<NR, MODE>(r, K, fixed, x, sum, D, MODE == kSmfByLikes ? (double)(hi - lo) : weight, lam, lr, X, H, row_loss);
}

template <int NR, int MODE>
__global__ __launch_bounds__(kLmfHeavyBlock) void lmf_heavy_kernel(const float* __restrict__ Y, int n_y, int K, const float* __restrict__ D,
                                                                   const int64_t* __restrict__ like_ptr, const int32_t* __restrict__ like_cols,
                                                                   int fixed, double weight, double lam, float lr, float* __restrict__ X,
                                                                   float* __restrict__ H, double* __restrict__ row_loss,
                                                                   unsigned long long* __restrict__ status, const int32_t* __restrict__ heavy_count,
                                                                   const int32_t* __restrict__ heavy_list) {
    __shared__ double part[kLmfHeavyWaves][NR * TKR_WAVE + 2];
    if ((int)blockIdx.x >= *heavy_count) return;                  // (the same word in every thread)
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const long long r = heavy_list[blockIdx.x];
    const long long lo = like_ptr[r], hi = like_ptr[r + 1];       // checked by the step kernel, which listed the row
    const long long n_slabs = (hi - lo + kLmfLikeSlab - 1) / kLmfLikeSlab;
    float x[NR];
    lmf_load_row<NR>(X + (size_t)r * K, K, x);
    double L[NR], sp = 0.0, ss = 0.0;
#pragma unroll
    for (int j = 0; j < NR; ++j) L[j] = 0.0;
    bool skipped = false;
    for (long long b = wave; b < n_slabs; b += kLmfHeavyWaves) {  // wave-uniform
        const long long first = lo + b * kLmfLikeSlab;
        LmfSum<NR> sum;
        skipped |= lmf_like_chain<NR, MODE>(Y, n_y, K, like_cols, first, (int)min((long long)kLmfLikeSlab, hi - first), x, sum);
#pragma unroll
        for (int j = 0; j < NR; ++j) L[j] += (double)sum.L[j];
        sp += sum.sp;
        ss += sum.ss;
    }
    if (skipped && lane == 0) status_refuse(status, r, kAlsSkipped);
#pragma unroll
    for (int j = 0; j < NR; ++j) part[wave][lane + 64 * j] = L[j];
    if (lane == 0) {
        part[wave][NR * TKR_WAVE] = sp;
        part[wave][NR * TKR_WAVE + 1] = ss;
    }
    __syncthreads();                                              // every thread of the workgroup is here: the exit above is uniform
    if (wave != 0) return;
    LmfSum<NR> sum;
    sum.sp = sum.ss = 0.0;
#pragma unroll
    for (int j = 0; j < NR; ++j) L[j] = 0.0;
    for (int w = 0; w < kLmfHeavyWaves; ++w) {
#pragma unroll
        for (int j = 0; j < NR; ++j) L[j] += part[w][lane + 64 * j];
        sum.sp += part[w][NR * TKR_WAVE];
        sum.ss += part[w][NR * TKR_WAVE + 1];
    }
#pragma unroll
    for (int j = 0; j < NR; ++j) sum.L[j] = (float)L[j];
    lmf_update_row<NR, MODE>(r, K, fixed, x, sum, D, MODE == kSmfByLikes ? (double)(hi - lo) : weight, lam, lr, X, H, row_loss);
}

template <int NR, int MODE>
static int lmf_launch_step(hipStream_t stream, const float* Y, int n_y, int K, const float* D, const int64_t* like_ptr, const int32_t* like_cols,
                       long long n_likes, long long n_x, int fixed, double weight, double lam, float lr, long long heavy_from, float* X,
                           float* H, double* row_loss, unsigned long long* st, int32_t* heavy_count, int32_t* heavy_list, long long cap) {
    hipLaunchKernelGGL((lmf_step_kernel<NR, MODE>), dim3((unsigned)((n_x + kLmfWaves - 1) / kLmfWaves)), dim3(kLmfBlock), 0, stream, Y, n_y, K, D, like_ptr,
                       like_cols, n_likes, n_x, fixed, weight, lam, lr, heavy_from, X, H, row_loss, st, heavy_count, heavy_list);
    TKR_LAUNCH_CHECK();
    if (cap > 0) {
        hipLaunchKernelGGL((lmf_heavy_kernel<NR, MODE>), dim3((unsigned)cap), dim3(kLmfHeavyBlock), 0, stream, Y, n_y, K, D, like_ptr, like_cols, fixed, weight,
                           lam, lr, X, H, row_loss, st, heavy_count, heavy_list);
        TKR_LAUNCH_CHECK();
    }
    return TKR_OK;
}

// The checked entry behind tkr_lmf_step_rows and tkr_smf_step_rows: the argument checks, the status word, the list of heavy rows and
// the NR ladder.  The tables hold K = k + extra columns, k <= k_max; fixed_min: 0, or -1 where `fixed` may name no column.
template <int MODE>
static int lmf_step_entry(const float* Y, int32_t n_y, int32_t k, int32_t k_max, int extra, const float* D, const int64_t* like_ptr,
                          const int32_t* like_cols, int64_t n_likes, int64_t n_x, int32_t fixed, int32_t fixed_min, double weight, double lam, double lr,
                          int64_t heavy_from, float* X, float* H, double* row_loss, void* workspace, int64_t workspace_bytes, int64_t* status,
                          void* stream_) {
    if (!Y || !D || !like_ptr || !X || !H || !status || ((uintptr_t)Y & 3) || ((uintptr_t)D & 3) || ((uintptr_t)X & 3) || ((uintptr_t)H & 3) ||
        ((uintptr_t)like_ptr & 7) || ((uintptr_t)like_cols & 3) || ((uintptr_t)status & 7) || ((uintptr_t)row_loss & 7) || ((uintptr_t)workspace & 15))
        return TKR_EINVAL;
    if (n_likes < 0 || (n_likes > 0 && !like_cols) || n_y < 1 || n_x < 1 || n_x > (int64_t)INT_MAX || heavy_from < 1 || workspace_bytes < 0)
        return TKR_EINVAL;
    if (!std::isfinite(weight) || !std::isfinite(lam) || !std::isfinite(lr) || lam < 0.0) return TKR_EINVAL;
    TKR_CHECK_RC(als_check_k(k, k_max));
    const int K = k + extra;
    if (fixed < fixed_min || fixed >= K) return TKR_EINVAL;
    int64_t cap = 0;                                              // listed rows, at most: each has more than heavy_from likes
    if (heavy_from < n_likes) {
        cap = std::min<int64_t>(n_x, n_likes / (heavy_from + 1));
        if (!workspace || workspace_bytes < lmf_list_bytes(n_x)) return TKR_EINVAL;
    }
    hipStream_t stream = (hipStream_t)stream_;
    unsigned long long* st = reinterpret_cast<unsigned long long*>(status);
    TKR_CHECK(hipMemsetAsync(st, 0xff, sizeof(unsigned long long), stream));          // -1: nothing refused
    int32_t* heavy_count = nullptr;
    int32_t* heavy_list = nullptr;
    if (cap > 0) {
        heavy_count = reinterpret_cast<int32_t*>(workspace);
        heavy_list = heavy_count + 4;
        TKR_CHECK(hipMemsetAsync(heavy_count, 0, 16, stream));
    }
#define TKR_LMF_STEP(N)                                                                                                                      \
    return lmf_launch_step<N, MODE>(stream, Y, n_y, K, D, like_ptr, like_cols, (long long)n_likes, (long long)n_x, fixed, weight, lam, (float)lr, \
                                    (long long)heavy_from, X, H, row_loss, st, heavy_count, heavy_list, (long long)cap)
    switch ((K + TKR_WAVE - 1) / TKR_WAVE) {
        case 1: TKR_LMF_STEP(1);
        case 2: TKR_LMF_STEP(2);
        default: TKR_LMF_STEP(3);
    }
#undef TKR_LMF_STEP
}

}  // namespace tkr
