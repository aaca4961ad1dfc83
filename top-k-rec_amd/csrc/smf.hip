// K27 -- the kernels of softmax matrix factorisation (SMF; top-k-rec_amd/smf.py).  Tables are augmented to K = k + 1 columns, a score is
// s_rc = x_r . y_c over all K of them, and p(c | r) = softmax_c(s_rc) over ALL rows c of Y.  One half-step moves every row r of X
// against the frozen Y:
//
//   lse_r = log sum over ALL rows c of Y of exp(s_rc)                                   tkr_smf_lse_rows
//   D_r   = sum over ALL rows c of Y of exp((s_rc - row_off[r]) - col_off[c]) y_c       tkr_smf_dense_rows
//   L_r   = sum over the likes c of r of y_c, the gradient, AdaGrad, the row's loss     tkr_smf_step_rows  (csrc/lmf_rows.h: K25's row code)
//
//   smf_dense_kernel<KT, LSE>   K25's lmf_dense_kernel with another function between its two products: one workgroup of 256 threads per
//                           (block of 128 rows of X, slab of TKR_SMF_SLAB rows of Y); a wave keeps 32 rows of X in registers as an MFMA
//                           operand, Y comes in tiles of 32 rows in ascending order through LDS ([32][32 KT + 1] floats, columns from K
//                           on are zeros; with it the tile's 32 column offsets), the next tile on its way in registers.  Per tile and
//                           wave, on v_mfma_f32_32x32x2_f32:  S^T = Ytile X^T, the contraction over the K columns in column order (a
//                           lane holds ONE row of X and 16 of the tile's rows), then
//                             LSE:    the lane follows a running maximum m over its scores, tile by tile, and l = sum exp(s - m): where
//                                     a tile raises the maximum, l is scaled by exp(m - m') first; the tile's scores are added in
//                                     register order.  At the slab's end the two lanes of a row are joined: M = max, l = l0 exp(m0 - M)
//                                     + l1 exp(m1 - M).  Nothing but S is formed: there is no second product.
//                             dense:  P = exp((s - row_off) - col_off) from the accumulators into the wave's own [32][33] piece of LDS,
//                                     the A-operand layout, +0 for a row of the tile past the table's end; D += P Ytile, the contraction
//                                     over the tile's rows in order, 32 KT columns of D in accumulators.  An MFMA result is bit for bit a
//                                     k-ordered fmaf chain, so a slab's partial of D[r][j] is ONE fp32 chain from +0.0 over the slab's
//                                     rows in row order, whatever the other rows of the call are.
//                           The score matrix never exists in memory.  Both passes form s by the same instructions in the same order: the
//                           s that exp(s - lse) sees has the bits the lse was made of.
//   smf_lse_reduce_kernel   more than one slab: M = max m, sum l exp(m - M) in ascending slab order in fp64, lse = fp32(M + log sum).
//                           One slab: the dense kernel writes fp32(m + log l), computed in fp64, itself -- the same value.
//   smf_reduce_kernel       more than one slab: the partials of D are added in ascending slab order in fp64 and rounded once.
// exp is exp2(x log2 e) on the hardware's v_exp_f32: exactly 1.0f at +0.0, exactly +0 at -inf (and below -104).  No float atomics.
#include "lmf_rows.h"

#include <math.h>

#include <algorithm>

namespace tkr {

constexpr int kSmfSlab = TKR_SMF_SLAB;
static_assert(kSmfSlab % kLmfTile == 0, "whole tiles");

__device__ __forceinline__ float smf_exp(float x) { return __expf(x); }

template <int KT, bool LSE>
__global__ __launch_bounds__(kLmfBlock) void smf_dense_kernel(const float* __restrict__ X, long long n_x, const float* __restrict__ Y, long long n_y,
                                                              int K, const float* __restrict__ row_off, const float* __restrict__ col_off,
                                                              float* __restrict__ out, size_t out_stride, float* __restrict__ lse_out) {
    constexpr int SP = lmf_stage_pitch(KT), NS = KT * 16, NPF = 4 * KT;
    __shared__ float stage[kLmfTile * SP];
    __shared__ float coff[kLmfTile];
    __shared__ float p_all[LSE ? 1 : kLmfWaves * kLmfTile * kLmfPPitch];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, l31 = lane & 31, h = lane >> 5;
    float* pw = p_all + (LSE ? 0 : wave * (kLmfTile * kLmfPPitch));
    const long long row0 = (long long)blockIdx.x * kLmfRows + wave * kLmfTile, my_row = row0 + l31;
    const long long c_begin = (long long)blockIdx.y * kSmfSlab, c_end = min(n_y, c_begin + (long long)kSmfSlab);
    const bool active = row0 < n_x;                               // (wave-uniform; a wave without rows still stages and meets the barriers)

    float xb[NS];                                                 // B operand of the first product: X[my_row][2 t + h]
#pragma unroll
    for (int t = 0; t < NS; ++t) {
        const int col = 2 * t + h;
        xb[t] = (my_row < n_x && col < K) ? X[(size_t)my_row * K + col] : 0.f;
    }
    const float ro = (!LSE && row_off && my_row < n_x) ? row_off[my_row] : 0.f;
    lmf_f32x16 acc[LSE ? 1 : KT];
    if constexpr (!LSE) {
#pragma unroll
        for (int cb = 0; cb < KT; ++cb)
#pragma unroll
            for (int reg = 0; reg < 16; ++reg) acc[cb][reg] = 0.f;
    }
    float m_run = -INFINITY, l_run = 0.f;                         // LSE: this lane's 16 rows of every tile so far

    float pf[NPF], pc = 0.f;                                      // the next tile: 32 lanes bring 32 consecutive floats of a row
    auto fetch = [&](long long base) {
#pragma unroll
        for (int i = 0; i < NPF; ++i) {
            const int q = (tid >> 5) + (kLmfBlock / 32) * i, rr = q / KT, col = (q - rr * KT) * 32 + l31;
            const long long c = base + rr;
            pf[i] = (c < c_end && col < K) ? Y[(size_t)c * K + col] : 0.f;
        }
        if constexpr (!LSE) pc = (col_off && tid < kLmfTile && base + tid < c_end) ? col_off[base + tid] : 0.f;
    };
    fetch(c_begin);
    for (long long base = c_begin; base < c_end; base += kLmfTile) {     // workgroup-uniform
        __syncthreads();                                          // the tile before is done with
#pragma unroll
        for (int i = 0; i < NPF; ++i) {
            const int q = (tid >> 5) + (kLmfBlock / 32) * i, rr = q / KT, col = (q - rr * KT) * 32 + l31;
            stage[rr * SP + col] = pf[i];
        }
        if constexpr (!LSE)
            if (tid < kLmfTile) coff[tid] = pc;
        __syncthreads();
        if (base + kLmfTile < c_end) fetch(base + kLmfTile);
        if (active) {
            lmf_f32x16 s;
#pragma unroll
            for (int reg = 0; reg < 16; ++reg) s[reg] = 0.f;
            const float* ap = stage + l31 * SP + h;
#pragma unroll
            for (int ch = 0; ch < 2 * KT; ++ch) {
                if (ch * 16 < K) {                                // (uniform) 16 columns at a time; the last ones may be zeros
#pragma unroll
                    for (int tt = 0; tt < 8; ++tt) s = __builtin_amdgcn_mfma_f32_32x32x2f32(ap[2 * (ch * 8 + tt)], xb[ch * 8 + tt], s, 0, 0, 0);
                }
            }
            const int left = (int)min((long long)kLmfTile, c_end - base);       // the tile's rows that are rows of Y
            if constexpr (LSE) {
                float top = m_run;
#pragma unroll
                for (int reg = 0; reg < 16; ++reg) {
                    const int c = (reg & 3) + 8 * (reg >> 2) + 4 * h;  // the tile's row this register holds, for row my_row of X
                    if (c < left) top = fmaxf(top, s[reg]);
                }
                if (top > m_run) {                                // (never with top == -inf: exp(m - top) has an argument)
                    l_run *= smf_exp(m_run - top);
                    m_run = top;
                }
#pragma unroll
                for (int reg = 0; reg < 16; ++reg) {
                    const int c = (reg & 3) + 8 * (reg >> 2) + 4 * h;
                    if (c < left) l_run += smf_exp(s[reg] - m_run);
                }
            } else {
#pragma unroll
                for (int reg = 0; reg < 16; ++reg) {
                    const int c = (reg & 3) + 8 * (reg >> 2) + 4 * h;
                    pw[l31 * kLmfPPitch + c] = c < left ? smf_exp((s[reg] - ro) - coff[c]) : 0.f;
                }
                __builtin_amdgcn_wave_barrier();                  // (the piece is this wave's own: LDS runs a wave's accesses in order)
                const float* pa = pw + l31 * kLmfPPitch + h;
                const float* bp = stage + h * SP + l31;
#pragma unroll 4
                for (int t = 0; t < kLmfTile; t += 2) {
                    const float a = pa[t];
#pragma unroll
                    for (int cb = 0; cb < KT; ++cb) acc[cb] = __builtin_amdgcn_mfma_f32_32x32x2f32(a, bp[t * SP + cb * 32], acc[cb], 0, 0, 0);
                }
                __builtin_amdgcn_wave_barrier();
            }
        }
    }
    if (!active) return;
    if constexpr (LSE) {
        const float m_other = __shfl_xor(m_run, 32);
        const float M = fmaxf(m_run, m_other);                    // finite: lane half 0 holds row 0 of the slab
        const float mine = l_run * smf_exp(m_run - M);            // (a half without rows: 0 * exp(-inf) = +0)
        const float other = __shfl_xor(mine, 32);
        if (h == 0 && my_row < n_x) {
            const float l = mine + other;
            if (gridDim.y == 1) {
                lse_out[my_row] = (float)((double)M + log((double)l));
            } else {
                float* pair = out + ((size_t)blockIdx.y * out_stride + (size_t)my_row) * 2;
                pair[0] = M;
                pair[1] = l;
            }
        }
    } else {
        float* mine = out + (size_t)blockIdx.y * out_stride;
#pragma unroll
        for (int cb = 0; cb < KT; ++cb) {
            const int col = cb * 32 + l31;
#pragma unroll
            for (int reg = 0; reg < 16; ++reg) {
                const long long row = row0 + (reg & 3) + 8 * (reg >> 2) + 4 * h;
                if (row < n_x && col < K) mine[(size_t)row * K + col] = acc[cb][reg];
            }
        }
    }
}

__global__ __launch_bounds__(kLmfBlock) void smf_reduce_kernel(const float* __restrict__ partial, int n_slabs, size_t stride, float* __restrict__ D) {
    const size_t idx = (size_t)blockIdx.x * kLmfBlock + threadIdx.x;
    if (idx >= stride) return;
    double s = 0.0;
    for (int b = 0; b < n_slabs; ++b) s += (double)partial[(size_t)b * stride + idx];
    D[idx] = (float)s;
}

__global__ __launch_bounds__(kLmfBlock) void smf_lse_reduce_kernel(const float* __restrict__ pairs, int n_slabs, size_t n_x, float* __restrict__ lse) {
    const size_t r = (size_t)blockIdx.x * kLmfBlock + threadIdx.x;
    if (r >= n_x) return;
    double M = (double)pairs[2 * r];
    for (int b = 1; b < n_slabs; ++b) M = fmax(M, (double)pairs[((size_t)b * n_x + r) * 2]);
    double s = 0.0;
    for (int b = 0; b < n_slabs; ++b) {
        const float* pair = pairs + ((size_t)b * n_x + r) * 2;
        s += (double)pair[1] * exp((double)pair[0] - M);
    }
    lse[r] = (float)(M + log(s));
}

template <bool LSE>
static int smf_launch_dense(hipStream_t stream, dim3 grid, int KT, const float* X, long long n_x, const float* Y, long long n_y, int K,
                            const float* row_off, const float* col_off, float* out, size_t out_stride, float* lse_out) {
#define TKR_SMF_DENSE(N)                                                                                                                       \
    hipLaunchKernelGGL((smf_dense_kernel<N, LSE>), grid, dim3(kLmfBlock), 0, stream, X, n_x, Y, n_y, K, row_off, col_off, out, out_stride, lse_out); \
    break
    switch (KT) {
        case 1: TKR_SMF_DENSE(1);
        case 2: TKR_SMF_DENSE(2);
        case 3: TKR_SMF_DENSE(3);
        case 4: TKR_SMF_DENSE(4);
        default: TKR_SMF_DENSE(5);
    }
#undef TKR_SMF_DENSE
    TKR_LAUNCH_CHECK();
    return TKR_OK;
}

static int64_t smf_slabs(int64_t n_y) { return (n_y + kSmfSlab - 1) / kSmfSlab; }

// what tkr_smf_lse_rows and tkr_smf_dense_rows check alike -> TKR_OK and the slabs
static int smf_dense_args(const float* X, int64_t n_x, const float* Y, int64_t n_y, int32_t k, const float* out, const void* workspace,
                          int64_t workspace_bytes, int64_t* n_slabs) {
    if (!X || !Y || !out || ((uintptr_t)X & 3) || ((uintptr_t)Y & 3) || ((uintptr_t)out & 3) || ((uintptr_t)workspace & 15)) return TKR_EINVAL;
    if (n_x < 1 || n_y < 1 || n_x > (int64_t)INT_MAX || workspace_bytes < 0) return TKR_EINVAL;
    TKR_CHECK_RC(als_check_k(k, TKR_SMF_MAX_K));
    *n_slabs = smf_slabs(n_y);
    return *n_slabs > 65535 ? TKR_EUNSUPPORTED : TKR_OK;          // (the slabs are the grid's second dimension)
}

}  // namespace tkr

extern "C" int64_t tkr_smf_workspace_bytes(int64_t n_x, int32_t k, int64_t n_y) {
    if (n_x < 1 || n_y < 1 || n_x > (int64_t)INT_MAX) return TKR_EINVAL;
    const int rc = tkr::als_check_k(k, TKR_SMF_MAX_K);
    if (rc != TKR_OK) return rc;
    const int64_t n_slabs = tkr::smf_slabs(n_y), K = k + 1;       // (D's partials hold the lse's pairs: K >= 2)
    const int64_t dense = n_slabs > 1 ? tkr::lmf_align(n_slabs * n_x * K * 4) : 0;
    return std::max(dense, tkr::lmf_list_bytes(n_x));
}

extern "C" int tkr_smf_lse_rows(const float* X, int64_t n_x, const float* Y, int64_t n_y, int32_t k, float* lse, void* workspace,
                                int64_t workspace_bytes, void* stream_) {
    using namespace tkr;
    int64_t n_slabs = 0;
    TKR_CHECK_RC(smf_dense_args(X, n_x, Y, n_y, k, lse, workspace, workspace_bytes, &n_slabs));
    if (n_slabs > 1 && (!workspace || workspace_bytes < lmf_align(n_slabs * n_x * 8))) return TKR_EINVAL;
    const int K = k + 1;
    hipStream_t stream = (hipStream_t)stream_;
    const dim3 grid((unsigned)((n_x + kLmfRows - 1) / kLmfRows), (unsigned)n_slabs);
    float* pairs = reinterpret_cast<float*>(workspace);
    TKR_CHECK_RC(smf_launch_dense<true>(stream, grid, (K + 31) / 32, X, n_x, Y, n_y, K, nullptr, nullptr, pairs, (size_t)n_x, lse));
    if (n_slabs > 1) {
        hipLaunchKernelGGL(smf_lse_reduce_kernel, dim3((unsigned)((n_x + kLmfBlock - 1) / kLmfBlock)), dim3(kLmfBlock), 0, stream, pairs, (int)n_slabs,
                           (size_t)n_x, lse);
        TKR_LAUNCH_CHECK();
    }
    return TKR_OK;
}

extern "C" int tkr_smf_dense_rows(const float* X, int64_t n_x, const float* Y, int64_t n_y, int32_t k, const float* row_off, const float* col_off,
                                  float* D, void* workspace, int64_t workspace_bytes, void* stream_) {
    using namespace tkr;
    int64_t n_slabs = 0;
    TKR_CHECK_RC(smf_dense_args(X, n_x, Y, n_y, k, D, workspace, workspace_bytes, &n_slabs));
    if (((uintptr_t)row_off & 3) || ((uintptr_t)col_off & 3)) return TKR_EINVAL;
    const int K = k + 1;
    const size_t stride = (size_t)n_x * K;
    if (n_slabs > 1 && (!workspace || workspace_bytes < lmf_align(n_slabs * n_x * (int64_t)K * 4))) return TKR_EINVAL;
    float* out = n_slabs > 1 ? reinterpret_cast<float*>(workspace) : D;
    hipStream_t stream = (hipStream_t)stream_;
    const dim3 grid((unsigned)((n_x + kLmfRows - 1) / kLmfRows), (unsigned)n_slabs);
    TKR_CHECK_RC(smf_launch_dense<false>(stream, grid, (K + 31) / 32, X, n_x, Y, n_y, K, row_off, col_off, out, stride, nullptr));
    if (n_slabs > 1) {
        hipLaunchKernelGGL(smf_reduce_kernel, dim3((unsigned)((stride + kLmfBlock - 1) / kLmfBlock)), dim3(kLmfBlock), 0, stream, out, (int)n_slabs, stride, D);
        TKR_LAUNCH_CHECK();
    }
    return TKR_OK;
}

extern "C" int tkr_smf_step_rows(const float* Y, int32_t n_y, int32_t k, const float* D, const int64_t* like_ptr, const int32_t* like_cols,
                                 int64_t n_likes, int64_t n_x, int32_t fixed, int32_t scale_by_likes, double lam, double lr, int64_t heavy_from,
                                 float* X, float* H, double* row_loss, void* workspace, int64_t workspace_bytes, int64_t* status, void* stream_) {
    using namespace tkr;
    if (!Y || !D || !like_ptr || !X || !H || !status || ((uintptr_t)Y & 3) || ((uintptr_t)D & 3) || ((uintptr_t)X & 3) || ((uintptr_t)H & 3) ||
        ((uintptr_t)like_ptr & 7) || ((uintptr_t)like_cols & 3) || ((uintptr_t)status & 7) || ((uintptr_t)row_loss & 7) || ((uintptr_t)workspace & 15))
        return TKR_EINVAL;
    if (n_likes < 0 || (n_likes > 0 && !like_cols) || n_y < 1 || n_x < 1 || n_x > (int64_t)INT_MAX || heavy_from < 1 || workspace_bytes < 0)
        return TKR_EINVAL;
    if (!std::isfinite(lam) || !std::isfinite(lr) || lam < 0.0 || (scale_by_likes != 0 && scale_by_likes != 1)) return TKR_EINVAL;
    TKR_CHECK_RC(als_check_k(k, TKR_SMF_MAX_K));
    const int K = k + 1;
    if (fixed < -1 || fixed >= K) return TKR_EINVAL;
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
    const int NR = (K + TKR_WAVE - 1) / TKR_WAVE;
#define TKR_SMF_STEP(N, MODE)                                                                                                                  \
    return lmf_launch_step<N, MODE>(stream, Y, n_y, K, D, like_ptr, like_cols, (long long)n_likes, (long long)n_x, fixed, 1.0, lam, (float)lr, \
                                    (long long)heavy_from, X, H, row_loss, st, heavy_count, heavy_list, (long long)cap)
    if (scale_by_likes) {
        switch (NR) {
            case 1: TKR_SMF_STEP(1, kSmfByLikes);
            case 2: TKR_SMF_STEP(2, kSmfByLikes);
            default: TKR_SMF_STEP(3, kSmfByLikes);
        }
    }
    switch (NR) {
        case 1: TKR_SMF_STEP(1, kSmfUnit);
        case 2: TKR_SMF_STEP(2, kSmfUnit);
        default: TKR_SMF_STEP(3, kSmfUnit);
    }
#undef TKR_SMF_STEP
}
