// The tile pipeline of the fused dense pass of K25 (csrc/lmf.hip: lmf_dense_kernel) and K27 (csrc/smf.hip: smf_dense_kernel), written
// ONCE: everything of the two kernels but the function between their two products.  One workgroup of kLmfBlock threads owns kLmfRows
// rows of X (a wave 32 of them, in registers as an MFMA operand) and one slab of rows of Y, which come in tiles of kLmfTile rows in
// ascending order through LDS, the next tile on its way in registers while this one is multiplied.  A kernel is
//
//     dense_load_x;  dense_fetch_tile(first tile)
//     for every tile of the slab (workgroup-uniform):
//         __syncthreads();  dense_stage_tile;  [what else the kernel stages]  __syncthreads();  dense_fetch_tile(next tile)
//         if the wave has rows:  s = dense_scores;  [its own function of s, into the wave's P piece]  dense_accumulate
//     dense_store
//
// No piece holds a __syncthreads(): the two barriers of a tile stand in the kernels, under workgroup-uniform control, and a wave without
// rows still fetches and stages.  No piece knows which kernel calls it.  On v_mfma_f32_32x32x2_f32 an MFMA result is bit for bit a
// k-ordered fmaf chain: dense_scores contracts over the K columns in column order, dense_accumulate over the tile's rows in row order,
// so a slab's partial of D[r][j] is ONE fp32 chain from +0.0 over the slab's rows in row order, whatever the other rows of the call
// are.  Behind the pieces, what the dense entry points share on the host: the argument check, the grid, the KT ladder, the reduction.
#pragma once
#include "lmf_parts.h"

#include <type_traits>

namespace tkr {

// the tile's row that register `reg` of an accumulator block holds in lane half h (the 32x32 layout: 4 rows, then 8 on)
__device__ __forceinline__ int dense_acc_row(int reg, int h) { return (reg & 3) + 8 * (reg >> 2) + 4 * h; }

template <int KT>
__device__ __forceinline__ void dense_clear(lmf_f32x16 (&acc)[KT]) {
#pragma unroll
    for (int cb = 0; cb < KT; ++cb)
#pragma unroll
        for (int reg = 0; reg < 16; ++reg) acc[cb][reg] = 0.f;
}

// B operand of the first product: X[my_row][2 t + h], zeros past the table's end and from column K on
template <int KT>
__device__ __forceinline__ void dense_load_x(const float* X, long long n_x, int K, long long my_row, float (&xb)[KT * 16]) {
    const int tid = threadIdx.x, lane = tid & 63, h = lane >> 5;
#pragma unroll
    for (int t = 0; t < KT * 16; ++t) {
        const int col = 2 * t + h;
        xb[t] = (my_row < n_x && col < K) ? X[(size_t)my_row * K + col] : 0.f;
    }
}

// where float i of a thread's 4 KT lies in the staged tile: 32 lanes bring 32 consecutive floats of a row
template <int KT>
__device__ __forceinline__ void dense_tile_slot(int i, int& rr, int& col) {
    const int tid = threadIdx.x, lane = tid & 63, l31 = lane & 31, q = (tid >> 5) + (kLmfBlock / 32) * i;
    rr = q / KT;
    col = (q - rr * KT) * 32 + l31;
}

// the tile of rows base .. base + 31 of Y into registers; zeros from row c_end and from column K on
template <int KT>
__device__ __forceinline__ void dense_fetch_tile(const float* Y, int K, long long base, long long c_end, float (&pf)[4 * KT]) {
#pragma unroll
    for (int i = 0; i < 4 * KT; ++i) {
        int rr, col;
        dense_tile_slot<KT>(i, rr, col);
        const long long c = base + rr;
        pf[i] = (c < c_end && col < K) ? Y[(size_t)c * K + col] : 0.f;
    }
}

// ... and from the registers into stage ([kLmfTile][lmf_stage_pitch(KT)]).  Between the two barriers of a tile
template <int KT>
__device__ __forceinline__ void dense_stage_tile(float* stage, const float (&pf)[4 * KT]) {
#pragma unroll
    for (int i = 0; i < 4 * KT; ++i) {
        int rr, col;
        dense_tile_slot<KT>(i, rr, col);
        stage[rr * lmf_stage_pitch(KT) + col] = pf[i];
    }
}

// S^T = Ytile X^T: register reg of the result is the score of row my_row of X against row dense_acc_row(reg, h) of the tile
template <int KT>
__device__ __forceinline__ lmf_f32x16 dense_scores(const float* stage, int K, const float (&xb)[KT * 16]) {
    const int tid = threadIdx.x, lane = tid & 63, l31 = lane & 31, h = lane >> 5;
    lmf_f32x16 s;
#pragma unroll
    for (int reg = 0; reg < 16; ++reg) s[reg] = 0.f;
    const float* ap = stage + l31 * lmf_stage_pitch(KT) + h;
#pragma unroll
    for (int ch = 0; ch < 2 * KT; ++ch) {
        if (ch * 16 < K) {                                        // (uniform) 16 columns at a time; the last ones may be zeros
#pragma unroll
            for (int tt = 0; tt < 8; ++tt) s = __builtin_amdgcn_mfma_f32_32x32x2f32(ap[2 * (ch * 8 + tt)], xb[ch * 8 + tt], s, 0, 0, 0);
        }
    }
    return s;
}

// D += P Ytile out of the wave's own piece pw ([kLmfTile][kLmfPPitch], P[my row][tile row]: the A-operand layout), which this wave
// has just written: the piece is its own and LDS runs a wave's accesses in order, so a wave barrier on either side is enough
template <int KT>
__device__ __forceinline__ void dense_accumulate(const float* pw, const float* stage, lmf_f32x16 (&acc)[KT]) {
    const int tid = threadIdx.x, lane = tid & 63, l31 = lane & 31, h = lane >> 5;
    __builtin_amdgcn_wave_barrier();
    const float* pa = pw + l31 * kLmfPPitch + h;
    const float* bp = stage + h * lmf_stage_pitch(KT) + l31;
#pragma unroll 4
    for (int t = 0; t < kLmfTile; t += 2) {
        const float a = pa[t];
#pragma unroll
        for (int cb = 0; cb < KT; ++cb) acc[cb] = __builtin_amdgcn_mfma_f32_32x32x2f32(a, bp[t * lmf_stage_pitch(KT) + cb * 32], acc[cb], 0, 0, 0);
    }
    __builtin_amdgcn_wave_barrier();
}

// the wave's 32 rows from row0 on, KT blocks of 32 columns, to `mine` ([n_x][K])
template <int KT>
__device__ __forceinline__ void dense_store(float* mine, long long row0, long long n_x, int K, const lmf_f32x16 (&acc)[KT]) {
    const int tid = threadIdx.x, lane = tid & 63, l31 = lane & 31, h = lane >> 5;
#pragma unroll
    for (int cb = 0; cb < KT; ++cb) {
        const int col = cb * 32 + l31;
#pragma unroll
        for (int reg = 0; reg < 16; ++reg) {
            const long long row = row0 + dense_acc_row(reg, h);
            if (row < n_x && col < K) mine[(size_t)row * K + col] = acc[cb][reg];
        }
    }
}

// more than one slab: the partials of D are added in ascending slab order in fp64 and rounded once (K20's Gram rule), and with SP the
// fp64 partials of sp [n_slabs][n_x] likewise.  One slab: the dense kernel writes D itself -- fp32 -> fp64 -> fp32 is the identity
template <bool SP>
__global__ __launch_bounds__(kLmfBlock) void dense_reduce_kernel(const float* __restrict__ partial, int n_slabs, size_t stride, float* __restrict__ D,
                                                                 const double* __restrict__ sp_partial, size_t n_x, double* __restrict__ sp) {
    const size_t idx = (size_t)blockIdx.x * kLmfBlock + threadIdx.x;
    if (idx < stride) {
        double s = 0.0;
        for (int b = 0; b < n_slabs; ++b) s += (double)partial[(size_t)b * stride + idx];
        D[idx] = (float)s;
    }
    if constexpr (SP) {
        if (idx < n_x) {
            double s = 0.0;
            for (int b = 0; b < n_slabs; ++b) s += sp_partial[(size_t)b * n_x + idx];
            sp[idx] = s;
        }
    }
}

static int dense_reduce(hipStream_t stream, const float* partial, int64_t n_slabs, size_t stride, float* D, const double* sp_partial, int64_t n_x,
                        double* sp) {
    const dim3 grid((unsigned)((stride + kLmfBlock - 1) / kLmfBlock));
    if (sp)
        hipLaunchKernelGGL(dense_reduce_kernel<true>, grid, dim3(kLmfBlock), 0, stream, partial, (int)n_slabs, stride, D, sp_partial, (size_t)n_x, sp);
    else
        hipLaunchKernelGGL(dense_reduce_kernel<false>, grid, dim3(kLmfBlock), 0, stream, partial, (int)n_slabs, stride, D, sp_partial, (size_t)n_x, sp);
    TKR_LAUNCH_CHECK();
    return TKR_OK;
}

// what every dense entry point checks alike (out: its fp32 result) -> TKR_OK and the slabs of `slab` rows of Y
static int dense_args(const float* X, int64_t n_x, const float* Y, int64_t n_y, int32_t k, int32_t k_max, int64_t slab, const float* out,
                      const void* workspace, int64_t workspace_bytes, int64_t* n_slabs) {
    if (!X || !Y || !out || ((uintptr_t)X & 3) || ((uintptr_t)Y & 3) || ((uintptr_t)out & 3) || ((uintptr_t)workspace & 15)) return TKR_EINVAL;
    if (n_x < 1 || n_y < 1 || n_x > (int64_t)INT_MAX || workspace_bytes < 0) return TKR_EINVAL;
    TKR_CHECK_RC(als_check_k(k, k_max));
    *n_slabs = (n_y + slab - 1) / slab;
    return *n_slabs > 65535 ? TKR_EUNSUPPORTED : TKR_OK;          // (the slabs are the grid's second dimension)
}

static dim3 dense_grid(int64_t n_x, int64_t n_slabs) { return dim3((unsigned)((n_x + kLmfRows - 1) / kLmfRows), (unsigned)n_slabs); }

// the one ladder over KT = ceil(K / 32), 1 .. 5: launch(std::integral_constant<int, KT>)
template <class Launch>
static void dense_for_kt(int K, Launch&& launch) {
    switch ((K + 31) / 32) {
        case 1: launch(std::integral_constant<int, 1>()); break;
        case 2: launch(std::integral_constant<int, 2>()); break;
        case 3: launch(std::integral_constant<int, 3>()); break;
        case 4: launch(std::integral_constant<int, 4>()); break;
        default: launch(std::integral_constant<int, 5>()); break;
    }
}

}  // namespace tkr
