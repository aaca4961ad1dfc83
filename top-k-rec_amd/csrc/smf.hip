// K27 -- the kernels of softmax matrix factorisation (SMF; top-k-rec_amd/smf.py).  Tables are augmented to K = k + 1 columns, a score is
// s_rc = x_r . y_c over all K of them, and p(c | r) = softmax_c(s_rc) over ALL rows c of Y.  One half-step moves every row r of X
// against the frozen Y:
//
//   lse_r = log sum over ALL rows c of Y of exp(s_rc)                                   tkr_smf_lse_rows
//   D_r   = sum over ALL rows c of Y of exp((s_rc - row_off[r]) - col_off[c]) y_c       tkr_smf_dense_rows
//   L_r   = sum over the likes c of r of y_c, the gradient, AdaGrad, the row's loss     tkr_smf_step_rows  (csrc/lmf_rows.h: K25's row code)
//
//   smf_dense_kernel<KT, LSE>   csrc/dense_tiles.h's tile pipeline, as K25's lmf_dense_kernel is, with another function between its two
//                           products: one workgroup of 256 threads per
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
//   dense_reduce_kernel     (csrc/dense_tiles.h) more than one slab: the partials of D are added in ascending slab order in fp64 and
//                           rounded once.
// exp is exp2(x log2 e) on the hardware's v_exp_f32: exactly 1.0f at +0.0, exactly +0 at -inf (and below -104).  No float atomics.
#include "dense_tiles.h"
#include "lmf_rows.h"

#include <math.h>

#include <algorithm>

namespace tkr {

constexpr int kSmfSlab = TKR_SMF_SLAB;
static_assert(kSmfSlab % kLmfTile == 0, "whole tiles");

__device__ __forceinline__ float smf_exp(float x) { return __expf(x); }

// csrc/dense_tiles.h's pipeline; LSE: its first product alone, with the running maximum and l behind it
template <int KT, bool LSE>
__global__ __launch_bounds__(kLmfBlock) void smf_dense_kernel(const float* __restrict__ X, long long n_x, const float* __restrict__ Y, long long n_y,
                                                              int K, const float* __restrict__ row_off, const float* __restrict__ col_off,
                                                              float* __restrict__ out, size_t out_stride, float* __restrict__ lse_out) {
    __shared__ float stage[kLmfTile * lmf_stage_pitch(KT)];
    __shared__ float coff[kLmfTile];
    __shared__ float p_all[LSE ? 1 : kLmfWaves * kLmfTile * kLmfPPitch];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, l31 = lane & 31, h = lane >> 5;
    float* pw = p_all + (LSE ? 0 : wave * (kLmfTile * kLmfPPitch));
    const long long row0 = (long long)blockIdx.x * kLmfRows + wave * kLmfTile, my_row = row0 + l31;
    const long long c_begin = (long long)blockIdx.y * kSmfSlab, c_end = min(n_y, c_begin + (long long)kSmfSlab);
    const bool active = row0 < n_x;                               // (wave-uniform; a wave without rows still stages and meets the barriers)

    float xb[KT * 16], pf[4 * KT], pc = 0.f;                      // pc: with the next tile, its column offset (threads 0 .. 31)
    dense_load_x<KT>(X, n_x, K, my_row, xb);
    const float ro = (!LSE && row_off && my_row < n_x) ? row_off[my_row] : 0.f;
    lmf_f32x16 acc[LSE ? 1 : KT];
    if constexpr (!LSE) dense_clear<KT>(acc);
    float m_run = -INFINITY, l_run = 0.f;                         // LSE: this lane's 16 rows of every tile so far

    auto fetch = [&](long long base) {
        dense_fetch_tile<KT>(Y, K, base, c_end, pf);
        if constexpr (!LSE) pc = (col_off && tid < kLmfTile && base + tid < c_end) ? col_off[base + tid] : 0.f;
    };
    fetch(c_begin);
    for (long long base = c_begin; base < c_end; base += kLmfTile) {     // workgroup-uniform
        __syncthreads();                                          // the tile before is done with
        dense_stage_tile<KT>(stage, pf);
        if constexpr (!LSE)
            if (tid < kLmfTile) coff[tid] = pc;
        __syncthreads();
        if (base + kLmfTile < c_end) fetch(base + kLmfTile);
        if (active) {
            const lmf_f32x16 s = dense_scores<KT>(stage, K, xb);
            const int left = (int)min((long long)kLmfTile, c_end - base);       // the tile's rows that are rows of Y
            if constexpr (LSE) {
                float top = m_run;
#pragma unroll
                for (int reg = 0; reg < 16; ++reg)
                    if (dense_acc_row(reg, h) < left) top = fmaxf(top, s[reg]);
                if (top > m_run) {                                // (never with top == -inf: exp(m - top) has an argument)
                    l_run *= smf_exp(m_run - top);
                    m_run = top;
                }
#pragma unroll
                for (int reg = 0; reg < 16; ++reg)
                    if (dense_acc_row(reg, h) < left) l_run += smf_exp(s[reg] - m_run);
            } else {
#pragma unroll
                for (int reg = 0; reg < 16; ++reg) {
                    const int c = dense_acc_row(reg, h);
                    pw[l31 * kLmfPPitch + c] = c < left ? smf_exp((s[reg] - ro) - coff[c]) : 0.f;
                }
                dense_accumulate<KT>(pw, stage, acc);
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
        dense_store<KT>(out + (size_t)blockIdx.y * out_stride, row0, n_x, K, acc);
    }
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
static int smf_launch_dense(hipStream_t stream, int64_t n_slabs, const float* X, long long n_x, const float* Y, long long n_y, int K,
                            const float* row_off, const float* col_off, float* out, size_t out_stride, float* lse_out) {
    const dim3 grid = dense_grid(n_x, n_slabs);
    dense_for_kt(K, [&](auto kt) {
        hipLaunchKernelGGL((smf_dense_kernel<decltype(kt)::value, LSE>), grid, dim3(kLmfBlock), 0, stream, X, n_x, Y, n_y, K, row_off, col_off, out,
                           out_stride, lse_out);
    });
    TKR_LAUNCH_CHECK();
    return TKR_OK;
}

}  // namespace tkr

extern "C" int64_t tkr_smf_workspace_bytes(int64_t n_x, int32_t k, int64_t n_y) {
    if (n_x < 1 || n_y < 1 || n_x > (int64_t)INT_MAX) return TKR_EINVAL;
    const int rc = tkr::als_check_k(k, TKR_SMF_MAX_K);
    if (rc != TKR_OK) return rc;
    const int64_t n_slabs = (n_y + tkr::kSmfSlab - 1) / tkr::kSmfSlab, K = k + 1;      // (D's partials hold the lse's pairs: K >= 2)
    const int64_t dense = n_slabs > 1 ? tkr::lmf_align(n_slabs * n_x * K * 4) : 0;
    return std::max(dense, tkr::lmf_list_bytes(n_x));
}

extern "C" int tkr_smf_lse_rows(const float* X, int64_t n_x, const float* Y, int64_t n_y, int32_t k, float* lse, void* workspace,
                                int64_t workspace_bytes, void* stream_) {
    using namespace tkr;
    int64_t n_slabs = 0;
    TKR_CHECK_RC(dense_args(X, n_x, Y, n_y, k, TKR_SMF_MAX_K, kSmfSlab, lse, workspace, workspace_bytes, &n_slabs));
    if (n_slabs > 1 && (!workspace || workspace_bytes < lmf_align(n_slabs * n_x * 8))) return TKR_EINVAL;
    hipStream_t stream = (hipStream_t)stream_;
    float* pairs = reinterpret_cast<float*>(workspace);
    TKR_CHECK_RC(smf_launch_dense<true>(stream, n_slabs, X, n_x, Y, n_y, k + 1, nullptr, nullptr, pairs, (size_t)n_x, lse));
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
    TKR_CHECK_RC(dense_args(X, n_x, Y, n_y, k, TKR_SMF_MAX_K, kSmfSlab, D, workspace, workspace_bytes, &n_slabs));
    if (((uintptr_t)row_off & 3) || ((uintptr_t)col_off & 3)) return TKR_EINVAL;
    const int K = k + 1;
    const size_t stride = (size_t)n_x * K;
    if (n_slabs > 1 && (!workspace || workspace_bytes < lmf_align(n_slabs * n_x * (int64_t)K * 4))) return TKR_EINVAL;
    float* out = n_slabs > 1 ? reinterpret_cast<float*>(workspace) : D;
    hipStream_t stream = (hipStream_t)stream_;
    TKR_CHECK_RC(smf_launch_dense<false>(stream, n_slabs, X, n_x, Y, n_y, K, row_off, col_off, out, stride, nullptr));
    return n_slabs > 1 ? dense_reduce(stream, out, n_slabs, stride, D, nullptr, n_x, nullptr) : TKR_OK;
}

extern "C" int tkr_smf_step_rows(const float* Y, int32_t n_y, int32_t k, const float* D, const int64_t* like_ptr, const int32_t* like_cols,
                                 int64_t n_likes, int64_t n_x, int32_t fixed, int32_t scale_by_likes, double lam, double lr, int64_t heavy_from,
                                 float* X, float* H, double* row_loss, void* workspace, int64_t workspace_bytes, int64_t* status, void* stream_) {
    if (scale_by_likes != 0 && scale_by_likes != 1) return TKR_EINVAL;
    const auto entry = scale_by_likes ? tkr::lmf_step_entry<tkr::kSmfByLikes> : tkr::lmf_step_entry<tkr::kSmfUnit>;
    return entry(Y, n_y, k, TKR_SMF_MAX_K, 1, D, like_ptr, like_cols, n_likes, n_x, fixed, -1, 1.0, lam, lr, heavy_from, X, H, row_loss, workspace,
                 workspace_bytes, status, stream_);
}
