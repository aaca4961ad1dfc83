// K9 -- fold-in: user vectors for histories the model was not trained on, against FROZEN item factors.
//
// The reference has no such call (a user exists only as a row trained by single/bpr.py:136-150).  The step is the model's own:
// for one user, T times, the BPR step of single/bpr.py:81-100 on a batch of P triplets that all carry this user -- x = b_i - b_j +
// <u, v_i - v_j>, g = sum_p [-sigma(-x_p) (v_i - v_j) + lu u] (mode 1: lu sign(u)) in the order p = 0 .. P-1, one RMSProp update of u
// (slot from 1.0) -- with the item rows, their biases and their slots left alone (tests/_foldin_oracle.py restates it with
// oracle/ref_np.py bpr_step).
//
// Users are independent and nothing but U is written: one wave owns a user from the first step to the last.  u, its slot and the
// gradient sum stay in registers (ceil(k / 64) elements per lane, k <= 512; wider rows: foldin_wide_kernel keeps them in LDS).  No
// plan, no row versions, no atomics, no ordering between waves.  Per step: lane p draws triplet p (sampler_draw.h draw_pair, stream
// 1: counter = (((first_row + x) T + t) P + p, round, 1) -- a user's stream does not depend on who shares the call), the indices are
// broadcast, and the 2 P item rows come through L2 (the item table is 5-9 MB at the benchmark shapes: it never leaves the caches)
// in groups whose loads are all issued before the first reduction of the group.
#include <math.h>

#include "fold_rows.h"
#include "sampler_draw.h"
#include "../../include/tkr.h"

namespace tkr {

struct FoldArgs {
    const float* V;
    const float* b;              // nullable
    const int64_t* hist_ptr;
    const int32_t* hist_cols;
    const float* U0;             // nullable: zeros
    float* U;
    float* loss;                 // nullable
    int32_t* trip;               // nullable
    int32_t m, n_items, k, mode, steps, P;
    float lu, lr;
    uint32_t k0, k1;
    uint64_t first_row;
};

// the draw of step t for user x: lane p < P holds triplet p.  `cols` is the user's row (ascending, unique: positives and membership
// test read the same array), 0 < deg < n_items.
__device__ __forceinline__ void fold_draw(const FoldArgs& a, const int32_t* __restrict__ cols, int deg, int64_t x, int t, int lane,
                                          int& di, int& dj) {
    di = 0;
    dj = 0;
    if (lane < a.P) {
        const uint64_t g = ((a.first_row + (uint64_t)x) * (uint64_t)a.steps + (uint64_t)t) * (uint64_t)a.P + (uint64_t)lane;
        const uint32_t c0 = (uint32_t)g, c1 = (uint32_t)(g >> 32);
        const u32x4 w0 = philox4x32_10(c0, c1, 0u, 1u, a.k0, a.k1);
        draw_pair<1u>(cols, cols, 0, deg, (uint32_t)a.n_items, w0, c0, c1, a.k0, a.k1, di, dj);
        if (a.trip) reinterpret_cast<int2*>(a.trip)[((size_t)x * a.steps + t) * a.P + lane] = make_int2(di, dj);
    }
}

template <int NE, bool VEC>
__global__ __launch_bounds__(kFoldWaves * TKR_WAVE) void foldin_kernel(const FoldArgs a) {
    constexpr int G = kFoldGroup<NE>;
    const int lane = threadIdx.x & (TKR_WAVE - 1);
    const int64_t x = __builtin_amdgcn_readfirstlane((int)(blockIdx.x * kFoldWaves + (threadIdx.x >> 6)));
    if (x >= a.m) return;
    const int k = a.k, P = a.P;
    float u[NE], ms[NE], g[NE];
    if (a.U0) fold_load<NE, VEC>(a.U0 + (size_t)x * k, k, lane, u);
    else {
#pragma unroll
        for (int e = 0; e < NE; ++e) u[e] = 0.f;
    }
#pragma unroll
    for (int e = 0; e < NE; ++e) ms[e] = 1.f;
    const int64_t lo = a.hist_ptr[x], hi = a.hist_ptr[x + 1];
    const int deg = (int)(hi - lo);
    const bool l2 = a.mode == 0;
    float loss = 0.f;
    // an empty history has no positive, one that covers the catalogue no negative: both keep the start vector, decided before any draw
    const int T = (deg <= 0 || deg >= a.n_items) ? 0 : a.steps;
    const int32_t* cols = a.hist_cols + lo;
    for (int t = 0; t < T; ++t) {
        int di, dj;
        fold_draw(a, cols, deg, x, t, lane, di, dj);
        const bool want_loss = a.loss != nullptr && t == T - 1;
#pragma unroll
        for (int e = 0; e < NE; ++e) g[e] = 0.f;
        float loss_x = 0.f;
        for (int done = 0; done < P; done += G) {
            const int n = min(G, P - done);
            float vi[G][NE], vj[G][NE], bi[G], bj[G];
#pragma unroll
            for (int q = 0; q < G; ++q) {              // slots beyond the last triplet load its rows again (valid addresses) and are not used
                const int src = min(done + q, P - 1);
                const int i = bcast_i(di, src), j = bcast_i(dj, src);
                fold_load<NE, VEC>(a.V + (size_t)i * k, k, lane, vi[q]);
                fold_load<NE, VEC>(a.V + (size_t)j * k, k, lane, vj[q]);
                bi[q] = a.b ? a.b[i] : 0.f;
                bj[q] = a.b ? a.b[j] : 0.f;
            }
#pragma unroll
            for (int q = 0; q < G; ++q) {
                if (q < n) {                            // wave-uniform
                    float xi = 0.f, xj = 0.f;
#pragma unroll
                    for (int e = 0; e < NE; ++e) {
                        xi = fmaf(u[e], vi[q][e], xi);
                        xj = fmaf(u[e], vj[q][e], xj);
                    }
                    wave_sum2(xi, xj);
                    const float xs = bi[q] - bj[q] + xi - xj;
                    const float s = sigmoid_neg(xs);
                    if (want_loss) loss_x += softplus_neg(xs);
#pragma unroll
                    for (int e = 0; e < NE; ++e) g[e] += -s * (vi[q][e] - vj[q][e]) + a.lu * (l2 ? u[e] : sgn(u[e]));
                }
            }
        }
        if (want_loss) {                                 // the regulariser of the objective: the same u in all P terms
            float r = 0.f;
#pragma unroll
            for (int e = 0; e < NE; ++e) r += l2 ? 0.5f * u[e] * u[e] : fabsf(u[e]);
            loss = loss_x + (float)P * a.lu * wave_sum(r);
        }
#pragma unroll
        for (int e = 0; e < NE; ++e) {                   // TF SparseApplyRMSProp, momentum 0 (oracle/ref_np.py _rmsprop_rows)
            ms[e] = kFoldRho * ms[e] + (1.f - kFoldRho) * g[e] * g[e];
            u[e] = u[e] - a.lr * g[e] / sqrtf(ms[e] + kFoldEps);
        }
    }
    fold_store<NE, VEC>(a.U + (size_t)x * k, k, lane, u);
    if (a.loss && lane == 0) a.loss[x] = loss;
}

// ---- any width: u, its slot and the gradient sum in LDS (3 k floats), one wave = one workgroup = one user.  Element e belongs to
// lane e % 64 in every pass, so no lane ever reads what another wrote: no barrier.  Every triplet costs two passes over its rows
// (the dot products, then the gradient), as in bpr_wide_kernel; sums run lane-strided instead of lane-contiguous.
__global__ __launch_bounds__(TKR_WAVE) void foldin_wide_kernel(const FoldArgs a) {
    extern __shared__ float4 fold_lds[];
    const int lane = threadIdx.x;
    const int64_t x = blockIdx.x;
    const int k = a.k, P = a.P;
    float* u = reinterpret_cast<float*>(fold_lds);
    float* ms = u + k;
    float* g = ms + k;
    for (int e = lane; e < k; e += TKR_WAVE) {
        u[e] = a.U0 ? a.U0[(size_t)x * k + e] : 0.f;
        ms[e] = 1.f;
    }
    const int64_t lo = a.hist_ptr[x], hi = a.hist_ptr[x + 1];
    const int deg = (int)(hi - lo);
    const bool l2 = a.mode == 0;
    float loss = 0.f;
    const int T = (deg <= 0 || deg >= a.n_items) ? 0 : a.steps;
    const int32_t* cols = a.hist_cols + lo;
    for (int t = 0; t < T; ++t) {
        int di, dj;
        fold_draw(a, cols, deg, x, t, lane, di, dj);
        const bool want_loss = a.loss != nullptr && t == T - 1;
        float loss_x = 0.f;
        for (int p = 0; p < P; ++p) {
            const int i = bcast_i(di, p), j = bcast_i(dj, p);
            const float* vi = a.V + (size_t)i * k;
            const float* vj = a.V + (size_t)j * k;
            const float bi = a.b ? a.b[i] : 0.f, bj = a.b ? a.b[j] : 0.f;
            float xi = 0.f, xj = 0.f;
            for (int e = lane; e < k; e += TKR_WAVE) {
                const float o = u[e];
                xi = fmaf(o, vi[e], xi);
                xj = fmaf(o, vj[e], xj);
            }
            wave_sum2(xi, xj);
            const float xs = bi - bj + xi - xj;
            const float s = sigmoid_neg(xs);
            if (want_loss) loss_x += softplus_neg(xs);
            for (int e = lane; e < k; e += TKR_WAVE) {
                const float o = u[e];
                const float part = -s * (vi[e] - vj[e]) + a.lu * (l2 ? o : sgn(o));
                g[e] = p == 0 ? part : g[e] + part;
            }
        }
        if (want_loss) {
            float r = 0.f;
            for (int e = lane; e < k; e += TKR_WAVE) r += l2 ? 0.5f * u[e] * u[e] : fabsf(u[e]);
            loss = loss_x + (float)P * a.lu * wave_sum(r);
        }
        for (int e = lane; e < k; e += TKR_WAVE) {
            const float ge = g[e];
            const float m2 = kFoldRho * ms[e] + (1.f - kFoldRho) * ge * ge;
            ms[e] = m2;
            u[e] = u[e] - a.lr * ge / sqrtf(m2 + kFoldEps);
        }
    }
    for (int e = lane; e < k; e += TKR_WAVE) a.U[(size_t)x * k + e] = u[e];
    if (a.loss && lane == 0) a.loss[x] = loss;
}

template <int NE>
static int launch_fold(const FoldArgs& a, bool vec, hipStream_t s) {
    const dim3 grid((a.m + kFoldWaves - 1) / kFoldWaves), block(kFoldWaves * TKR_WAVE);
    if (vec) hipLaunchKernelGGL((foldin_kernel<NE, true>), grid, block, 0, s, a);
    else hipLaunchKernelGGL((foldin_kernel<NE, false>), grid, block, 0, s, a);
    return (int)hipGetLastError();
}

}  // namespace tkr

extern "C" int tkr_bpr_foldin(const float* V, const float* b, int32_t n_items, int32_t k, const int64_t* hist_ptr,
                              const int32_t* hist_cols, int32_t m, const float* U0, float lu, float lr, int32_t mode, int32_t steps,
                              int32_t triplets, uint64_t seed, uint64_t first_row, float* U, float* loss, int32_t* trip, void* stream) {
    if (!V || !hist_ptr || !hist_cols || !U) return TKR_EINVAL;
    if (n_items <= 0 || k <= 0 || m < 0 || steps < 1 || triplets < 1 || triplets > TKR_WAVE) return TKR_EINVAL;
    if ((mode != 0 && mode != 1) || !(lr == lr) || !(lu == lu)) return TKR_EINVAL;
    if (m == 0) return TKR_OK;
    tkr::FoldArgs a;
    a.V = V; a.b = b; a.hist_ptr = hist_ptr; a.hist_cols = hist_cols; a.U0 = U0; a.U = U; a.loss = loss; a.trip = trip;
    a.m = m; a.n_items = n_items; a.k = k; a.mode = mode; a.steps = steps; a.P = triplets;
    a.lu = lu; a.lr = lr;
    a.k0 = (uint32_t)seed; a.k1 = (uint32_t)(seed >> 32);
    a.first_row = first_row;
    hipStream_t s = (hipStream_t)stream;
    const int ne = (k + TKR_WAVE - 1) / TKR_WAVE;
    const bool aligned = (((uintptr_t)V | (uintptr_t)U | (uintptr_t)U0) & 15) == 0;
    if (ne == 1) return tkr::launch_fold<1>(a, aligned && k == 64, s);
    if (ne == 2) return tkr::launch_fold<2>(a, aligned && k == 128, s);
    if (ne <= 4) return tkr::launch_fold<4>(a, aligned && k == 256, s);
    if (ne <= 8) return tkr::launch_fold<8>(a, aligned && k == 512, s);
    const size_t lds = (size_t)3 * k * sizeof(float);
    if (lds > (size_t)tkr::kFoldMaxLds) return TKR_EUNSUPPORTED;
    if (lds > 48 * 1024)
        TKR_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(tkr::foldin_wide_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    hipLaunchKernelGGL(tkr::foldin_wide_kernel, dim3(m), dim3(TKR_WAVE), lds, s, a);
    TKR_LAUNCH_CHECK();
    return TKR_OK;
}
