// The pieces of the ALS family (K20 / K21 csrc/als.hip, K24 csrc/als_cg.hip) as device functions: what sums y y^T over a list of rows
// of Y.  A workgroup is 256 threads; the rows are gathered 32 at a time into LDS and the four waves multiply the tile with itself on
// the exact-fp32 MFMA (v_mfma_f32_32x32x2_f32), the contraction over the staged rows, two per instruction: every element of the sum
// is one fp32 fma chain in list order.  Only the 32 x 32 blocks on and above the diagonal are computed; a * b and b * a are the same
// product, so the mirrored element has the same bits.
// slab_sum<KT> and als_emit<KT> are what als_slab_kernel<KT> and als_solve_kernel call (k <= 128, the blocks a wave holds known at
// compile time), and they stay WHOLE: see als_wide_slab_kernel (csrc/als.hip), which shares the indexing, the pitch and the types.
#pragma once
#include "tkr_common.h"
#include "../../include/tkr.h"

#include <limits.h>

namespace tkr {

typedef float als_f32x16 __attribute__((ext_vector_type(16)));

constexpr int kAlsBlock = 256;
constexpr int kAlsWaves = kAlsBlock / TKR_WAVE;
constexpr int kAlsTile = 32;                                      // rows of Y staged at a time = the MFMA's block edge
constexpr int kAlsSlab = TKR_ALS_GRAM_SLAB;
static_assert(kAlsSlab % kAlsTile == 0 && kAlsSlab < (1 << 24), "whole tiles; a slab's count is exact in fp32");

// the kinds of K20, K21, K24 and K25 (no kind 0): an index outside the table was skipped; the row's system cannot be solved (K20: not
// positive definite in fp32, K24: p . q or the solution not finite); like_ptr is wrong at the row.  The last two leave the row as it is
enum { kAlsSkipped = 1, kAlsNotSolved = 2, kAlsBadPtr = 3 };

__host__ __device__ constexpr int als_tiles(int KT) { return KT * (KT + 1) / 2; }
__host__ __device__ constexpr int als_tiles_per_wave(int KT) { return (als_tiles(KT) + kAlsWaves - 1) / kAlsWaves; }
// floats between two staged rows (and two rows of K24's panel of G): the two rows an MFMA reads at once (lanes 0-31, lanes 32-63)
// start 32 banks apart
__host__ __device__ constexpr int als_stage_pitch(int KT) { return (KT & 1) ? KT * 32 : KT * 32 + 32; }

static inline int als_check_k(int32_t k, int32_t k_max) {
    if (k < 1) return TKR_EINVAL;
    return k > k_max ? TKR_EUNSUPPORTED : TKR_OK;
}

__device__ __forceinline__ bool als_ptr_ok(long long lo, long long hi, long long n_likes, long long row) {
    return lo >= 0 && lo <= hi && hi <= n_likes && (row != 0 || lo == 0) && hi - lo <= (long long)INT_MAX;
}

// block `idx` of the upper triangle, row-major: (0,0) (0,1) .. (0,KT-1) (1,1) ..
__device__ __forceinline__ void als_tile_of(int KT, int idx, int& bi, int& bj) {
    bi = 0;
    for (int len = KT; idx >= len; --len) {
        idx -= len;
        ++bi;
    }
    bj = bi + idx;
}

template <int N>
__device__ __forceinline__ void als_zero(als_f32x16 (&acc)[N]) {
#pragma unroll
    for (int s = 0; s < N; ++s)
#pragma unroll
        for (int reg = 0; reg < 16; ++reg) acc[s][reg] = 0.f;
}

// acc += sum over list[first .. first + count) of y y^T (this wave's blocks); col_sum += the column sums (thread j < k: column j, in
// fp64) and n_valid += the rows that were summed (threads < k).  list == nullptr: the rows first .. first + count themselves.  A row
// outside [0, n) is skipped and reported: 4 * word_row + 1, or 4 * (its position in the list) + 1 where word_row < 0.
// Called by all threads of the workgroup with the same arguments; stage [32][SP] floats, cols_s [32] ints.
template <int KT>
__device__ __forceinline__ void slab_sum(const float* __restrict__ Y, int n, int k, const int32_t* __restrict__ list, long long first, int count,
                                         float* stage, int* cols_s, als_f32x16 (&acc)[als_tiles_per_wave(KT)], double& col_sum, int& n_valid,
                                         long long word_row, unsigned long long* status) {
    constexpr int SP = als_stage_pitch(KT), NT = als_tiles(KT), TPW = als_tiles_per_wave(KT);
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, l31 = lane & 31, h = lane >> 5;
    for (int base = 0; base < count; base += kAlsTile) {          // workgroup-uniform
        const int n_here = min(kAlsTile, count - base);
        if (tid < kAlsTile) {
            int c = -1;
            if (tid < n_here) {
                const long long t = first + base + tid;
                c = list ? list[t] : (int)t;
                if ((uint32_t)c >= (uint32_t)n) {
                    status_refuse(status, word_row < 0 ? t : word_row, kAlsSkipped);
                    c = -1;
                }
            }
            cols_s[tid] = c;
        }
        __syncthreads();
        for (int q = tid >> 5; q < kAlsTile * KT; q += kAlsBlock / 32) {       // 32 lanes bring 32 consecutive floats of a row
            const int rr = q / KT, col = (q - rr * KT) * 32 + l31;
            const int c = cols_s[rr];
            stage[rr * SP + col] = (c >= 0 && col < k) ? Y[(size_t)c * k + col] : 0.f;
        }
        __syncthreads();
        if (tid < k) {
            for (int i = 0; i < kAlsTile; ++i) {
                col_sum += (double)stage[i * SP + tid];
                n_valid += cols_s[i] >= 0;
            }
        }
#pragma unroll
        for (int s = 0; s < TPW; ++s) {
            const int idx = wave + kAlsWaves * s;
            if (idx < NT) {                                       // wave-uniform
                int bi, bj;
                als_tile_of(KT, idx, bi, bj);
                const float* ap = stage + h * SP + bi * 32 + l31;
                const float* bp = stage + h * SP + bj * 32 + l31;
#pragma unroll 4
                for (int t = 0; t < kAlsTile; t += 2)
                    acc[s] = __builtin_amdgcn_mfma_f32_32x32x2f32(ap[t * SP], bp[t * SP], acc[s], 0, 0, 0);
            }
        }
        __syncthreads();                                          // the tile is done with (after the last one the caller may reuse stage)
    }
}

// this wave's blocks, element by element: f(p, q, value) for p, q < k, both triangles
template <int KT, typename F>
__device__ __forceinline__ void als_emit(const als_f32x16 (&acc)[als_tiles_per_wave(KT)], int k, F f) {
    constexpr int NT = als_tiles(KT), TPW = als_tiles_per_wave(KT);
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, l31 = lane & 31, h = lane >> 5;
#pragma unroll
    for (int s = 0; s < TPW; ++s) {
        const int idx = wave + kAlsWaves * s;
        if (idx < NT) {
            int bi, bj;
            als_tile_of(KT, idx, bi, bj);
            const int q = bj * 32 + l31;
#pragma unroll
            for (int reg = 0; reg < 16; ++reg) {
                const int p = bi * 32 + (reg & 3) + 8 * (reg >> 2) + 4 * h;
                if (p < k && q < k) {
                    f(p, q, acc[s][reg]);
                    if (bi != bj) f(q, p, acc[s][reg]);
                }
            }
        }
    }
}

}  // namespace tkr
