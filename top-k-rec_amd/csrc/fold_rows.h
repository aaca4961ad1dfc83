// What the two fold-in kernels share (K9 csrc/foldin.hip: new users, K10 csrc/foldin_items.hip: new items): the constants of the
// step and the row of a wave held in registers.
#pragma once
#include "tkr_common.h"

namespace tkr {

constexpr float kFoldRho = 0.9f, kFoldEps = 1e-10f;      // oracle/ref_np.py RHO, EPS (TF RMSPropOptimizer defaults)
constexpr int kFoldWaves = 4;                            // users per workgroup of the register form
constexpr int kFoldMaxLds = 160 * 1024;                  // one workgroup's LDS on gfx950: the widest row of the generic form

// lane l owns the NE contiguous elements [l NE, l NE + NE) of a row, as in K2 (csrc/bpr_step.hip load_row): VEC = full rows at a
// 16-byte aligned base, one unpredicated vector access per lane; otherwise clamped addresses and a select, never a predicated load
template <int NE, bool VEC>
__device__ __forceinline__ void fold_load(const float* __restrict__ base, int k, int lane, float (&r)[NE]) {
    const int e0 = lane * NE;
    if constexpr (VEC && NE == 1) {
        r[0] = base[e0];
    } else if constexpr (VEC && NE == 2) {
        const float2 v = *reinterpret_cast<const float2*>(base + e0);
        r[0] = v.x; r[1] = v.y;
    } else if constexpr (VEC && NE % 4 == 0) {
#pragma unroll
        for (int q = 0; q < NE; q += 4) {
            const float4 v = *reinterpret_cast<const float4*>(base + e0 + q);
            r[q] = v.x; r[q + 1] = v.y; r[q + 2] = v.z; r[q + 3] = v.w;
        }
    } else {
#pragma unroll
        for (int q = 0; q < NE; ++q) {
            const float v = base[min(e0 + q, k - 1)];
            r[q] = (e0 + q < k) ? v : 0.f;
        }
    }
}

template <int NE, bool VEC>
__device__ __forceinline__ void fold_store(float* __restrict__ base, int k, int lane, const float (&r)[NE]) {
    const int e0 = lane * NE;
    if constexpr (VEC && NE == 1) {
        base[e0] = r[0];
    } else if constexpr (VEC && NE == 2) {
        *reinterpret_cast<float2*>(base + e0) = make_float2(r[0], r[1]);
    } else if constexpr (VEC && NE % 4 == 0) {
#pragma unroll
        for (int q = 0; q < NE; q += 4) *reinterpret_cast<float4*>(base + e0 + q) = make_float4(r[q], r[q + 1], r[q + 2], r[q + 3]);
    } else {
#pragma unroll
        for (int q = 0; q < NE; ++q)
            if (e0 + q < k) base[e0 + q] = r[q];
    }
}

// triplets whose rows are in flight together: 2 G NE registers of rows
template <int NE> constexpr int kFoldGroup = NE == 1 ? 8 : NE == 2 ? 4 : 2;

}  // namespace tkr
