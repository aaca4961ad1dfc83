// The one fp32 score of a (user, item) pair, for every kernel that scores pairs outside the MFMA tiles (K4's rescoring and wide rows,
// K6, K8's likes, K12, K16, K17, K19): the fma chain, its tail and the rated-item bit.
//
// The chain is the fp32 dot product of the fp32-MFMA kernel, bit for bit: v_mfma_f32_32x32x2_f32 adds the product of k-half 0, then the
// product of k-half 1, one fused multiply-add each (measured: scripts/probe_mfma_order.py, 100 % of 7,680 scores at k = 50, 64, 100,
// 128) -- so with KH = ceil(k / 2): acc <- fma(v[kk], u[kk], acc); acc <- fma(v[KH+kk], u[KH+kk], acc) for kk = 0 .. KH-1 (the second
// only while KH + kk < k), then fl(acc + bias) and -0.0 -> +0.0 as the filter of that kernel does.  A chain stays in ONE lane from the
// first product to the last: reduced across lanes it would have other bits.
#pragma once
#include "tkr_common.h"

namespace tkr {

// Four steps of the chain: factors kk .. kk + 3 of both k-halves (v0 / u0: half 0, v1 / u1: half 1).  The order (half 0, half 1) x
// (x, y, z, w) is written here and nowhere else.
__device__ __forceinline__ void chain_step4(float& acc, const float4 v0, const float4 v1, const float4 u0, const float4 u1) {
    acc = fmaf(v0.x, u0.x, acc); acc = fmaf(v1.x, u1.x, acc);
    acc = fmaf(v0.y, u0.y, acc); acc = fmaf(v1.y, u1.y, acc);
    acc = fmaf(v0.z, u0.z, acc); acc = fmaf(v1.z, u1.z, acc);
    acc = fmaf(v0.w, u0.w, acc); acc = fmaf(v1.w, u1.w, acc);
}

// -0.0 -> +0.0: a score of zero ties with 0.0 like numpy, whatever its sign
__device__ __forceinline__ float chain_pos_zero(float s) { return s + 0.0f; }

// the tail of a score: fl(acc + bias), then -0.0 -> +0.0
__device__ __forceinline__ float chain_finish(float acc, float bias_value) { return chain_pos_zero(acc + bias_value); }
// ... with bias[col], or 0 where the model has no item bias
__device__ __forceinline__ float chain_finish(float acc, const float* bias, int col) { return chain_finish(acc, bias ? bias[col] : 0.f); }

// B steps of the chain from kk on, one factor of each half per step, for N rows against one shared row
template <int N, int B, bool ROWS_FIRST>
__device__ __forceinline__ void chain_pairs(const float* __restrict__ shared, const float* const (&rows)[N], int KH, int kk, float (&acc)[N]) {
    float u0[B], u1[B], v0[N][B], v1[N][B];
    if constexpr (!ROWS_FIRST) {
#pragma unroll
        for (int q = 0; q < B; ++q) { u0[q] = shared[kk + q]; u1[q] = shared[KH + kk + q]; }
    }
#pragma unroll
    for (int q = 0; q < B; ++q)
#pragma unroll
        for (int n = 0; n < N; ++n) { v0[n][q] = rows[n][kk + q]; v1[n][q] = rows[n][KH + kk + q]; }
    if constexpr (ROWS_FIRST) {
#pragma unroll
        for (int q = 0; q < B; ++q) { u0[q] = shared[kk + q]; u1[q] = shared[KH + kk + q]; }
    }
#pragma unroll
    for (int q = 0; q < B; ++q)
#pragma unroll
        for (int n = 0; n < N; ++n) { acc[n] = fmaf(v0[n][q], u0[q], acc[n]); acc[n] = fmaf(v1[n][q], u1[q], acc[n]); }
}

// The chains of N rows against one shared row, side by side: per row the chain above, the shared row loaded once for all N.
// k % 8 == 0: both halves of a row are 16-byte aligned, float4 loads, UNROLL chunks of each half in flight.  Other widths: one step
// at a time, the factor of half 1 while there is one (the last step of an odd k has none); with BLOCK > 1 the steps that have a factor
// in each half (KH, or KH - 1 at an odd k) go first, BLOCK at a time and then singly, and the plain loop is left the odd factor.
// ROWS_FIRST: a chunk of the N rows is asked for before the shared row's.  The loads are all that UNROLL, BLOCK and ROWS_FIRST change
// (they are what the callers measured, and what their register counts hang on); the bits are the same for every choice.
template <int N, int UNROLL, int BLOCK, bool ROWS_FIRST>
__device__ __forceinline__ void chain_rows(const float* __restrict__ shared, const float* const (&rows)[N], int k, float (&acc)[N]) {
    const int KH = (k + 1) >> 1;
#pragma unroll
    for (int n = 0; n < N; ++n) acc[n] = 0.f;
    if ((k & 7) == 0) {
#pragma unroll UNROLL
        for (int kk = 0; kk < KH; kk += 4) {
            float4 u0, u1, v0[N], v1[N];
            if constexpr (!ROWS_FIRST) { u0 = *reinterpret_cast<const float4*>(shared + kk); u1 = *reinterpret_cast<const float4*>(shared + KH + kk); }
#pragma unroll
            for (int n = 0; n < N; ++n) {
                v0[n] = *reinterpret_cast<const float4*>(rows[n] + kk);
                v1[n] = *reinterpret_cast<const float4*>(rows[n] + KH + kk);
            }
            if constexpr (ROWS_FIRST) { u0 = *reinterpret_cast<const float4*>(shared + kk); u1 = *reinterpret_cast<const float4*>(shared + KH + kk); }
#pragma unroll
            for (int n = 0; n < N; ++n) chain_step4(acc[n], v0[n], v1[n], u0, u1);
        }
        return;
    }
    int kk = 0;
    if constexpr (BLOCK > 1) {                                   // the steps that have a factor in each half, both loaded in one round trip
        const int both = k - KH;
        for (; kk + BLOCK <= both; kk += BLOCK) chain_pairs<N, BLOCK, ROWS_FIRST>(shared, rows, KH, kk, acc);
        for (; kk < both; ++kk) chain_pairs<N, 1, ROWS_FIRST>(shared, rows, KH, kk, acc);
    }
    for (; kk < KH; ++kk) {                                      // what is left: at BLOCK = 1 every step, else the odd factor
        const float u0 = shared[kk];
#pragma unroll
        for (int n = 0; n < N; ++n) acc[n] = fmaf(rows[n][kk], u0, acc[n]);
        if (KH + kk < k) {
            const float u1 = shared[KH + kk];
#pragma unroll
            for (int n = 0; n < N; ++n) acc[n] = fmaf(rows[n][KH + kk], u1, acc[n]);
        }
    }
}

// the score of one pair: user row `up`, item row `vp`, bias[col] when there is a bias
__device__ __forceinline__ float exact_score(const float* __restrict__ up, const float* __restrict__ vp, int k, const float* bias, int col) {
    const float* const rows[1] = {vp};
    float acc[1];
    chain_rows<1, 8, 1, true>(up, rows, k, acc);                 // 32 loads in flight: two memory round trips per 128 factors
    return chain_finish(acc[0], bias, col);
}

// column c is rated for `row`: bit c & 31 of word (c >> 5, row) of the rated-item mask (csrc/topk.hip tkr_build_rated_mask)
__device__ __forceinline__ bool col_masked(const uint32_t* __restrict__ mask, int pitch, int row, int c) {
    return (mask[(size_t)(c >> 5) * pitch + row] >> (c & 31)) & 1u;
}

}  // namespace tkr
