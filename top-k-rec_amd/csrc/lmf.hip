// K25 -- the two kernels of logistic matrix factorisation (LMF; top-k-rec_amd/lmf.py).  Tables are augmented to K = k + 2 columns, a
// score is s_rc = x_r . y_c over all K of them, and one half-step of the alternation moves every row r of X against the frozen Y:
//
//   D_r = sum over ALL rows c of Y of  sigma(s_rc) y_c            tkr_lmf_dense_rows   (and sp_r = sum_c softplus(s_rc))
//   L_r = sum over the likes c of r of (1 - sigma(s_rc)) y_c      tkr_lmf_step_rows    (and the gradient, AdaGrad, the row's loss)
//
//   lmf_dense_kernel<KT>    one workgroup of 256 threads per (block of 128 rows of X, slab of TKR_LMF_SLAB rows of Y); a wave owns 32 rows
//                           of X and keeps them in registers as an MFMA operand.  Y comes in tiles of 32 rows, in ascending order,
//                           through LDS ([32][32 KT + 1] floats: both products read it without a bank conflict; columns from K on are
//                           zeros), the next tile on its way in registers while this one is multiplied.  Per tile and wave, on
//                           v_mfma_f32_32x32x2_f32:
//                             S^T = Ytile X^T      the contraction over the K columns in column order;
//                             P = sigma(S)         from the accumulators (a lane holds ONE row of X, 16 of the tile's rows) into the
//                                                  wave's own [32][33] piece of LDS, the A-operand layout of the next product;
//                             D += P Ytile         the contraction over the tile's rows in order, 32 KT columns of D in accumulators.
//                           An MFMA result is bit for bit a k-ordered fmaf chain, so a slab's partial of D[r][j] is ONE fp32 chain from
//                           +0.0 over the slab's rows in row order, whatever the other rows of the call are.  The score matrix never
//                           exists in memory.  With sp wanted a lane also adds softplus of its 16 scores per tile, in fp64, in tile-row
//                           order; the two lanes of a row are added at the end.
//   lmf_reduce_kernel       more than one slab: the partials are added in ascending slab order in fp64 and rounded once (K20's Gram
//                           rule).  One slab: the dense kernel writes D and sp itself -- fp32 -> fp64 -> fp32 is the identity.
// The two kernels of the step are csrc/lmf_rows.h's, in its mode kLmfLogistic (K27's step is the same code in another mode):
//   lmf_step_kernel<NR>     one wave per row: the row, its slot and the gradient in registers (element j of the row in lane j & 63,
//                           register j >> 6).  Whole rows of Y are gathered through L2, 64 like columns read at a time; per like the
//                           score is one fixed tree (lane chains by fma from +0.0 over its registers, then the DPP tree of wave_sum),
//                           L takes one fma per component in stored order.  A row with more than heavy_from likes is not summed here:
//                           it is put on a list (an integer counter; the order of the list changes no result).
//   lmf_heavy_kernel<NR>    one workgroup of 16 waves per listed row.  Its likes are cut into slabs of TKR_LMF_LIKE_SLAB; slab j is
//                           summed by wave j mod 16 as the step kernel sums a row (an fp32 chain from +0.0), a wave adds its slabs in
//                           ascending order in fp64, wave 0 adds the 16 waves in ascending order in fp64 and rounds once.
// No float atomics; the atomics are the status word's minimum and the list's counter.  Nothing refused is used as an index.
#include "lmf_rows.h"

#include <math.h>

#include <algorithm>

namespace tkr {

template <int KT, bool LOSS>
__global__ __launch_bounds__(kLmfBlock) void lmf_dense_kernel(const float* __restrict__ X, long long n_x, const float* __restrict__ Y,
                                                              long long n_y, int K, float* __restrict__ out, size_t out_stride,
                                                              double* __restrict__ sp_out, size_t sp_stride) {
    constexpr int SP = lmf_stage_pitch(KT), NS = KT * 16, NPF = 4 * KT;
    __shared__ float stage[kLmfTile * SP];
    __shared__ float p_all[kLmfWaves * kLmfTile * kLmfPPitch];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, l31 = lane & 31, h = lane >> 5;
    float* pw = p_all + wave * (kLmfTile * kLmfPPitch);
    const long long row0 = (long long)blockIdx.x * kLmfRows + wave * kLmfTile, my_row = row0 + l31;
    const long long c_begin = (long long)blockIdx.y * kLmfSlab, c_end = min(n_y, c_begin + (long long)kLmfSlab);
    const bool active = row0 < n_x;                               // (wave-uniform; a wave without rows still stages and meets the barriers)

    float xb[NS];                                                 // B operand of the first product: X[my_row][2 t + h]
#pragma unroll
    for (int t = 0; t < NS; ++t) {
        const int col = 2 * t + h;
        xb[t] = (my_row < n_x && col < K) ? X[(size_t)my_row * K + col] : 0.f;
    }
    lmf_f32x16 acc[KT];
#pragma unroll
    for (int cb = 0; cb < KT; ++cb)
#pragma unroll
        for (int reg = 0; reg < 16; ++reg) acc[cb][reg] = 0.f;
    double sp_sum = 0.0;

    float pf[NPF];                                                // the next tile: 32 lanes bring 32 consecutive floats of a row
    auto fetch = [&](long long base) {
#pragma unroll
        for (int i = 0; i < NPF; ++i) {
            const int q = (tid >> 5) + (kLmfBlock / 32) * i, rr = q / KT, col = (q - rr * KT) * 32 + l31;
            const long long c = base + rr;
            pf[i] = (c < c_end && col < K) ? Y[(size_t)c * K + col] : 0.f;
        }
    };
    fetch(c_begin);
    for (long long base = c_begin; base < c_end; base += kLmfTile) {     // workgroup-uniform
        __syncthreads();                                          // the tile before is done with
#pragma unroll
        for (int i = 0; i < NPF; ++i) {
            const int q = (tid >> 5) + (kLmfBlock / 32) * i, rr = q / KT, col = (q - rr * KT) * 32 + l31;
            stage[rr * SP + col] = pf[i];
        }
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
#pragma unroll
            for (int reg = 0; reg < 16; ++reg) {
                const int c = (reg & 3) + 8 * (reg >> 2) + 4 * h;  // the tile's row this register holds, for row my_row of X
                pw[l31 * kLmfPPitch + c] = lmf_sigmoid(s[reg]);
                if constexpr (LOSS)
                    if (base + c < c_end) sp_sum += (double)lmf_softplus(s[reg]);
            }
            __builtin_amdgcn_wave_barrier();                      // (the piece is this wave's own: LDS runs a wave's accesses in order)
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
    if (!active) return;
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
    if constexpr (LOSS) {
        const double other = __shfl_xor(sp_sum, 32);
        if (h == 0 && my_row < n_x) sp_out[(size_t)blockIdx.y * sp_stride + my_row] = sp_sum + other;
    }
}

__global__ __launch_bounds__(kLmfBlock) void lmf_reduce_kernel(const float* __restrict__ partial, int n_slabs, size_t stride, float* __restrict__ D,
                                                               const double* __restrict__ sp_partial, size_t n_x, double* __restrict__ sp) {
    const size_t idx = (size_t)blockIdx.x * kLmfBlock + threadIdx.x;
    if (idx < stride) {
        double s = 0.0;
        for (int b = 0; b < n_slabs; ++b) s += (double)partial[(size_t)b * stride + idx];
        D[idx] = (float)s;
    }
    if (sp && idx < n_x) {
        double s = 0.0;
        for (int b = 0; b < n_slabs; ++b) s += sp_partial[(size_t)b * n_x + idx];
        sp[idx] = s;
    }
}

template <int KT>
static int launch_dense(hipStream_t stream, dim3 grid, const float* X, long long n_x, const float* Y, long long n_y, int K, float* out, size_t out_stride,
                        double* sp_out, size_t sp_stride) {
    if (sp_out)
        hipLaunchKernelGGL((lmf_dense_kernel<KT, true>), grid, dim3(kLmfBlock), 0, stream, X, n_x, Y, n_y, K, out, out_stride, sp_out, sp_stride);
    else
        hipLaunchKernelGGL((lmf_dense_kernel<KT, false>), grid, dim3(kLmfBlock), 0, stream, X, n_x, Y, n_y, K, out, out_stride, sp_out, sp_stride);
    TKR_LAUNCH_CHECK();
    return TKR_OK;
}

static int64_t lmf_slabs(int64_t n_y) { return (n_y + kLmfSlab - 1) / kLmfSlab; }

}  // namespace tkr

extern "C" int64_t tkr_lmf_workspace_bytes(int64_t n_x, int32_t k, int64_t n_y) {
    if (n_x < 1 || n_y < 1 || n_x > (int64_t)INT_MAX) return TKR_EINVAL;
    const int rc = tkr::als_check_k(k, TKR_LMF_MAX_K);
    if (rc != TKR_OK) return rc;
    const int64_t n_slabs = tkr::lmf_slabs(n_y), K = k + 2;
    const int64_t dense = n_slabs > 1 ? tkr::lmf_align(n_slabs * n_x * K * 4) + tkr::lmf_align(n_slabs * n_x * 8) : 0;
    return std::max(dense, tkr::lmf_list_bytes(n_x));
}

extern "C" int tkr_lmf_dense_rows(const float* X, int64_t n_x, const float* Y, int64_t n_y, int32_t k, float* D, double* sp, void* workspace,
                                  int64_t workspace_bytes, void* stream_) {
    using namespace tkr;
    if (!X || !Y || !D || ((uintptr_t)X & 3) || ((uintptr_t)Y & 3) || ((uintptr_t)D & 3) || ((uintptr_t)sp & 7) || ((uintptr_t)workspace & 15))
        return TKR_EINVAL;
    if (n_x < 1 || n_y < 1 || n_x > (int64_t)INT_MAX || workspace_bytes < 0) return TKR_EINVAL;
    TKR_CHECK_RC(als_check_k(k, TKR_LMF_MAX_K));
    const int K = k + 2, KT = (K + 31) / 32;
    const int64_t n_slabs = lmf_slabs(n_y);
    if (n_slabs > 65535) return TKR_EUNSUPPORTED;                  // (the slabs are the grid's second dimension)
    const size_t stride = (size_t)n_x * K;
    float* out = D;
    double* sp_out = sp;
    if (n_slabs > 1) {
        const int64_t front = lmf_align(n_slabs * n_x * (int64_t)K * 4);
        if (!workspace || workspace_bytes < front + (sp ? lmf_align(n_slabs * n_x * 8) : 0)) return TKR_EINVAL;
        out = reinterpret_cast<float*>(workspace);
        if (sp) sp_out = reinterpret_cast<double*>(reinterpret_cast<unsigned char*>(workspace) + front);
    }
    hipStream_t stream = (hipStream_t)stream_;
    const dim3 grid((unsigned)((n_x + kLmfRows - 1) / kLmfRows), (unsigned)n_slabs);
    switch (KT) {
        case 1: TKR_CHECK_RC(launch_dense<1>(stream, grid, X, n_x, Y, n_y, K, out, stride, sp_out, (size_t)n_x)); break;
        case 2: TKR_CHECK_RC(launch_dense<2>(stream, grid, X, n_x, Y, n_y, K, out, stride, sp_out, (size_t)n_x)); break;
        case 3: TKR_CHECK_RC(launch_dense<3>(stream, grid, X, n_x, Y, n_y, K, out, stride, sp_out, (size_t)n_x)); break;
        case 4: TKR_CHECK_RC(launch_dense<4>(stream, grid, X, n_x, Y, n_y, K, out, stride, sp_out, (size_t)n_x)); break;
        default: TKR_CHECK_RC(launch_dense<5>(stream, grid, X, n_x, Y, n_y, K, out, stride, sp_out, (size_t)n_x)); break;
    }
    if (n_slabs > 1) {
        hipLaunchKernelGGL(lmf_reduce_kernel, dim3((unsigned)((stride + kLmfBlock - 1) / kLmfBlock)), dim3(kLmfBlock), 0, stream, out, (int)n_slabs, stride,
                           D, sp_out, (size_t)n_x, sp);
        TKR_LAUNCH_CHECK();
    }
    return TKR_OK;
}

extern "C" int tkr_lmf_step_rows(const float* Y, int32_t n_y, int32_t k, const float* D, const int64_t* like_ptr, const int32_t* like_cols,
                                 int64_t n_likes, int64_t n_x, int32_t fixed, double alpha, double lam, double lr, int64_t heavy_from, float* X,
                                 float* H, double* row_loss, void* workspace, int64_t workspace_bytes, int64_t* status, void* stream_) {
    using namespace tkr;
    if (!Y || !D || !like_ptr || !X || !H || !status || ((uintptr_t)Y & 3) || ((uintptr_t)D & 3) || ((uintptr_t)X & 3) || ((uintptr_t)H & 3) ||
        ((uintptr_t)like_ptr & 7) || ((uintptr_t)like_cols & 3) || ((uintptr_t)status & 7) || ((uintptr_t)row_loss & 7) || ((uintptr_t)workspace & 15))
        return TKR_EINVAL;
    if (n_likes < 0 || (n_likes > 0 && !like_cols) || n_y < 1 || n_x < 1 || n_x > (int64_t)INT_MAX || heavy_from < 1 || workspace_bytes < 0)
        return TKR_EINVAL;
    if (!std::isfinite(alpha) || !std::isfinite(lam) || !std::isfinite(lr) || lam < 0.0) return TKR_EINVAL;
    TKR_CHECK_RC(als_check_k(k, TKR_LMF_MAX_K));
    const int K = k + 2;
    if (fixed < 0 || fixed >= K) return TKR_EINVAL;
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
#define TKR_LMF_STEP(N)                                                                                                                       \
    return lmf_launch_step<N, kLmfLogistic>(stream, Y, n_y, K, D, like_ptr, like_cols, (long long)n_likes, (long long)n_x, fixed, alpha, lam, (float)lr,        \
                          (long long)heavy_from, X, H, row_loss, st, heavy_count, heavy_list, (long long)cap)
    switch (NR) {
        case 1: TKR_LMF_STEP(1);
        case 2: TKR_LMF_STEP(2);
        default: TKR_LMF_STEP(3);
    }
#undef TKR_LMF_STEP
}
