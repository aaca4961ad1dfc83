// The fold-in kernels (K9 csrc/foldin.hip: new users, K10 csrc/foldin_items.hip: new items): the constants of the step, the row of
// a wave held in registers, and the one body both sides run -- in registers (fold_kernel) and in LDS (fold_wide_kernel) -- with
// its launch (launch_fold).
//
// One wave owns a row `w` from the first step to the last: w, its RMSProp slot and the gradient sum stay with the wave.  Per step
// lane p draws triplet p, the indices are broadcast, the two rows of every triplet are gathered through L2, and the sums run in the
// order p = 0 .. P-1.  No plan, no row versions, no atomics, no ordering between waves.  A side (UserSide, ItemSide) supplies
// what differs:
//   Args            the argument block: start / out / loss / trip, m, k, mode, steps, P, lr, k0, k1, first_row and the side's own
//   Side(a, x)      the state of row x that the draw needs;  steps(a): how many steps the row takes (0: it keeps its start)
//   draw            lane p's triplet of step t as a FoldTriplet, written to a.trip in the side's layout when asked for
//   row_a, row_b    the rows of a triplet in the side's two tables;  biases: the two biases that enter the score
//   dot             one element of the two dot products;  score: x_p from them;  coef, dir: the triplet adds coef * dir to the
//                   gradient;  lam: the weight of its regulariser term;  penalty: the regulariser of the objective
//   kBias           the row has a bias of its own: bias_grad, update_bias, store_bias, and a step without any triplet is skipped
#pragma once
#include "tkr_common.h"

namespace tkr {

constexpr float kFoldRho = 0.9f, kFoldEps = 1e-10f;      // oracle/ref_np.py RHO, EPS (TF RMSPropOptimizer defaults)
constexpr int kFoldWaves = 4;                            // rows per workgroup of the register form
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

// lane p's triplet of a step: the role the wave's row takes in it (< 0: no legal draw, the triplet contributes nothing) and its rows
// in the side's tables A and B, which can be loaded whatever the role
struct FoldTriplet { int role, ia, ib; };

// the Philox counter of triplet `lane` of step t of row x: a row's stream does not depend on who shares the call
template <class Args>
__device__ __forceinline__ uint64_t fold_counter(const Args& a, int64_t x, int t, int lane) {
    return ((a.first_row + (uint64_t)x) * (uint64_t)a.steps + (uint64_t)t) * (uint64_t)a.P + (uint64_t)lane;
}

// TF SparseApplyRMSProp, momentum 0 (oracle/ref_np.py _rmsprop_rows)
__device__ __forceinline__ void fold_rmsprop(float& ms, float& w, float g, float lr) {
    ms = kFoldRho * ms + (1.f - kFoldRho) * g * g;
    w = w - lr * g / sqrtf(ms + kFoldEps);
}

// a value's term of the regulariser
__device__ __forceinline__ float fold_reg_value(bool l2, float w) { return l2 ? 0.5f * w * w : fabsf(w); }

// ---- k <= 512: w, its slot and the gradient sum in registers, NE = ceil(k / 64) elements per lane, kFoldWaves rows per workgroup.
// The rows of G triplets are all requested before the first reduction of the group.
template <class Side, int NE, bool VEC>
__global__ __launch_bounds__(kFoldWaves * TKR_WAVE) void fold_kernel(const typename Side::Args a) {
    constexpr int G = kFoldGroup<NE>;
    const int lane = threadIdx.x & (TKR_WAVE - 1);
    const int64_t x = __builtin_amdgcn_readfirstlane((int)(blockIdx.x * kFoldWaves + (threadIdx.x >> 6)));
    if (x >= a.m) return;
    const int k = a.k, P = a.P;
    float w[NE], ms[NE], g[NE];
    if (a.start) fold_load<NE, VEC>(a.start + (size_t)x * k, k, lane, w);
    else {
#pragma unroll
        for (int e = 0; e < NE; ++e) w[e] = 0.f;
    }
#pragma unroll
    for (int e = 0; e < NE; ++e) ms[e] = 1.f;
    Side side(a, x);
    const bool l2 = a.mode == 0;
    float loss = 0.f;
    const int T = side.steps(a);
    for (int t = 0; t < T; ++t) {
        const FoldTriplet d = side.draw(a, x, t, lane);
        if constexpr (Side::kBias)
            if (__ballot(d.role >= 0) == 0) continue;     // no triplet in this step: nothing moves, not even the slots
        const bool want_loss = a.loss != nullptr && t == T - 1;
#pragma unroll
        for (int e = 0; e < NE; ++e) g[e] = 0.f;
        float gb = 0.f, loss_x = 0.f;
        int n1 = 0, n0 = 0;                              // triplets of role 1 / role 0 so far
        for (int done = 0; done < P; done += G) {
            const int n = min(G, P - done);             // (q < n, not done + q < P: the latter costs the user side 2-8 VGPRs and a wave per SIMD)
            float ra[G][NE], rb[G][NE], ba[G], bb[G];
            int role[G];
#pragma unroll
            for (int q = 0; q < G; ++q) {              // slots beyond the last triplet load its rows again (valid addresses) and are not used
                const int src = min(done + q, P - 1);
                role[q] = q < n ? bcast_i(d.role, src) : -1;
                const int ia = bcast_i(d.ia, src), ib = bcast_i(d.ib, src);
                fold_load<NE, VEC>(Side::row_a(a, ia), k, lane, ra[q]);
                fold_load<NE, VEC>(Side::row_b(a, ib), k, lane, rb[q]);
                Side::biases(a, ia, ib, ba[q], bb[q]);
            }
#pragma unroll
            for (int q = 0; q < G; ++q) {
                if (role[q] >= 0) {                     // wave-uniform
                    float da = 0.f, db = 0.f;
#pragma unroll
                    for (int e = 0; e < NE; ++e) Side::dot(w[e], ra[q][e], rb[q][e], da, db);
                    wave_sum2(da, db);
                    const float xs = side.score(role[q], ba[q], bb[q], da, db);
                    const float s = sigmoid_neg(xs);
                    const float c = Side::coef(role[q], s), lam = Side::lam(a, role[q]);
                    if (want_loss) loss_x += softplus_neg(xs);
                    n1 += role[q] == 1;
                    n0 += role[q] != 1;
                    // (the regulariser's derivative is written out: behind a helper function hipcc fuses this line's product and sum
                    // at NE >= 2, which moves the last bit of the user rows: DESIGN.md section 4, K9 "Registers")
#pragma unroll
                    for (int e = 0; e < NE; ++e) g[e] += c * Side::dir(ra[q][e], rb[q][e]) + lam * (l2 ? w[e] : sgn(w[e]));
                    if constexpr (Side::kBias) gb += side.bias_grad(a, c, l2);
                }
            }
        }
        if (want_loss) {                                 // the regulariser of the objective: the same w in all its terms
            float r = 0.f;
#pragma unroll
            for (int e = 0; e < NE; ++e) r += fold_reg_value(l2, w[e]);
            loss = loss_x + side.penalty(a, wave_sum(r), n1, n0);
        }
#pragma unroll
        for (int e = 0; e < NE; ++e) fold_rmsprop(ms[e], w[e], g[e], a.lr);
        if constexpr (Side::kBias) side.update_bias(a, gb);
    }
    fold_store<NE, VEC>(a.out + (size_t)x * k, k, lane, w);
    if (lane == 0) {
        if constexpr (Side::kBias) side.store_bias(a, x);
        if (a.loss) a.loss[x] = loss;
    }
}

// ---- any width: w, its slot and the gradient sum in LDS (3 k floats), one wave = one workgroup = one row.  Element e belongs to
// lane e % 64 in every pass, so no lane ever reads what another wrote: no barrier.  Every triplet costs two passes over its rows
// (the dot products, then the gradient), as in bpr_wide_kernel; sums run lane-strided instead of lane-contiguous.
template <class Side>
__global__ __launch_bounds__(TKR_WAVE) void fold_wide_kernel(const typename Side::Args a) {
    extern __shared__ float4 fold_lds[];
    const int lane = threadIdx.x;
    const int64_t x = blockIdx.x;
    const int k = a.k, P = a.P;
    float* w = reinterpret_cast<float*>(fold_lds);
    float* ms = w + k;
    float* g = ms + k;
    for (int e = lane; e < k; e += TKR_WAVE) {
        w[e] = a.start ? a.start[(size_t)x * k + e] : 0.f;
        ms[e] = 1.f;
    }
    Side side(a, x);
    const bool l2 = a.mode == 0;
    float loss = 0.f;
    const int T = side.steps(a);
    for (int t = 0; t < T; ++t) {
        const FoldTriplet d = side.draw(a, x, t, lane);
        if constexpr (Side::kBias)
            if (__ballot(d.role >= 0) == 0) continue;
        const bool want_loss = a.loss != nullptr && t == T - 1;
        float gb = 0.f, loss_x = 0.f;
        int n1 = 0, n0 = 0;
        bool first = true;
        for (int p = 0; p < P; ++p) {
            const int role = bcast_i(d.role, p);
            if (role < 0) continue;                      // wave-uniform
            const int ia = bcast_i(d.ia, p), ib = bcast_i(d.ib, p);
            const float* ra = Side::row_a(a, ia);
            const float* rb = Side::row_b(a, ib);
            float ba, bb, da = 0.f, db = 0.f;
            Side::biases(a, ia, ib, ba, bb);
            for (int e = lane; e < k; e += TKR_WAVE) Side::dot(w[e], ra[e], rb[e], da, db);
            wave_sum2(da, db);
            const float xs = side.score(role, ba, bb, da, db);
            const float s = sigmoid_neg(xs);
            const float c = Side::coef(role, s), lam = Side::lam(a, role);
            if (want_loss) loss_x += softplus_neg(xs);
            n1 += role == 1;
            n0 += role != 1;
            for (int e = lane; e < k; e += TKR_WAVE) {
                const float part = c * Side::dir(ra[e], rb[e]) + lam * (l2 ? w[e] : sgn(w[e]));
                g[e] = first ? part : g[e] + part;
            }
            if constexpr (Side::kBias) gb += side.bias_grad(a, c, l2);
            first = false;
        }
        if (want_loss) {
            float r = 0.f;
            for (int e = lane; e < k; e += TKR_WAVE) r += fold_reg_value(l2, w[e]);
            loss = loss_x + side.penalty(a, wave_sum(r), n1, n0);
        }
        for (int e = lane; e < k; e += TKR_WAVE) {
            float m2 = ms[e], we = w[e];
            fold_rmsprop(m2, we, g[e], a.lr);
            ms[e] = m2;
            w[e] = we;
        }
        if constexpr (Side::kBias) side.update_bias(a, gb);
    }
    for (int e = lane; e < k; e += TKR_WAVE) a.out[(size_t)x * k + e] = w[e];
    if (lane == 0) {
        if constexpr (Side::kBias) side.store_bias(a, x);
        if (a.loss) a.loss[x] = loss;
    }
}

template <class Side, int NE>
static int launch_fold_rows(const typename Side::Args& a, bool aligned, hipStream_t s) {
    const dim3 grid((a.m + kFoldWaves - 1) / kFoldWaves), block(kFoldWaves * TKR_WAVE);
    if (aligned && a.k == NE * TKR_WAVE) hipLaunchKernelGGL((fold_kernel<Side, NE, true>), grid, block, 0, s, a);
    else hipLaunchKernelGGL((fold_kernel<Side, NE, false>), grid, block, 0, s, a);
    return (int)hipGetLastError();
}

// `bases`: the row tables, the start and the output of the call, or-ed: the vector form needs every one of them 16-byte aligned
template <class Side>
static int launch_fold(const typename Side::Args& a, uintptr_t bases, hipStream_t s) {
    const int ne = (a.k + TKR_WAVE - 1) / TKR_WAVE;
    const bool aligned = (bases & 15) == 0;
    if (ne == 1) return launch_fold_rows<Side, 1>(a, aligned, s);
    if (ne == 2) return launch_fold_rows<Side, 2>(a, aligned, s);
    if (ne <= 4) return launch_fold_rows<Side, 4>(a, aligned, s);
    if (ne <= 8) return launch_fold_rows<Side, 8>(a, aligned, s);
    const size_t lds = (size_t)3 * a.k * sizeof(float);
    if (lds > (size_t)kFoldMaxLds) return TKR_EUNSUPPORTED;
    if (lds > 48 * 1024)
        TKR_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(fold_wide_kernel<Side>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    hipLaunchKernelGGL(fold_wide_kernel<Side>, dim3(a.m), dim3(TKR_WAVE), lds, s, a);
    return (int)hipGetLastError();
}

}  // namespace tkr
