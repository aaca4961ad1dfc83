// K16 -- learn the weights of a linear fusion of several trained models (the reference's old/methods/bfusion.py + ranking_fusion.py and
// efusion.py).  Serving a fused model needs no kernel: sum_m w_m (<U_m[u], V_m[i]> + b_m[i]) is the inner product of two concatenated
// tables (top-k-rec_amd/fusion.py fuse).  Learning the weights needs the per-model scores of sampled triplets or of every training
// like: gathers over M table pairs.  Every score here is exact_score (csrc/score_chain.h) as it stands -- the bits of K4 and K12 --
// sequential in one lane, never reduced across lanes (chain_scores below: exact_score's chain with more loads in flight).
//
//   fusion_features_kernel       a lane per triplet g = first_triplet + t: draw_triplet (csrc/sampler_draw.h, K1's stream) then, model
//                                by model, D[t, m] = fl(s_m(u, i) - s_m(u, j)), the two chains side by side on one load of the user's factors.
//                                No atomics, no workspace.
//   fusion_sgd_kernel            ONE workgroup walks the batches in order (they depend on each other through W alone): thread `tid`
//                                takes rows tid, tid + kSgdThreads, ... of the batch, W is read from LDS at the top of a batch, the
//                                M gradient sums and the loss go through the one fixed tree (wave_sum: DPP; then the waves in wave
//                                order through LDS).  Which thread takes which row depends on the row's place in its batch only, so a
//                                call cut into chunks of whole batches gives the bits of the whole call.
//   fusion_user_weights_kernel   a wave per user: lanes take likes l, l + 64, ..., the user's rows are uniform over the wave; the
//                                squared errors go through wave_sum.
#include "tkr_common.h"
#include "score_chain.h"
#include "sampler_draw.h"
#include "../../include/tkr.h"

#pragma clang fp contract(off)   // every rounding below is written out: fmaf where one is meant, two roundings elsewhere

namespace tkr {

constexpr int kFusionMax = TKR_FUSION_MAX_MODELS;
constexpr int kSgdThreads = 1024, kSgdWaves = kSgdThreads / TKR_WAVE;
constexpr int kUwWaves = 4;

// exact_score's chain (csrc/score_chain.h chain_rows) for N item rows against one user row, with other loads: the user's factors are
// loaded once for the positive and the negative of a triplet, and at a width that is no multiple of 8 (k = 50, the reference's
// default) eight steps of both halves are in flight at a time instead of one (measured: DESIGN.md section 4 K16).
template <int N>
__device__ __forceinline__ void chain_scores(const float* __restrict__ up, const float* const (&vp)[N], int k, float (&acc)[N]) {
    chain_rows<N, 4, 8, false>(up, vp, k, acc);
}

__global__ __launch_bounds__(256) void fusion_features_kernel(
    const tkr_fusion_models md, const int32_t* __restrict__ tr_users, uint32_t n_tr, const int32_t* __restrict__ row_ptr,
    const int32_t* __restrict__ pos_cols, const int32_t* __restrict__ cols_sorted, uint32_t n_items, uint64_t seed,
    uint64_t first_triplet, int64_t count, float* __restrict__ D_out, int32_t* __restrict__ trip_out) {
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= count) return;
    int u, i, j;
    draw_triplet(tr_users, n_tr, row_ptr, pos_cols, cols_sorted, n_items, (uint32_t)seed, (uint32_t)(seed >> 32),
                 first_triplet + (uint64_t)t, u, i, j);
    if (trip_out) {
        trip_out[t * 3 + 0] = u;
        trip_out[t * 3 + 1] = i;
        trip_out[t * 3 + 2] = j;
    }
    // ids come from the caller's CSR; one outside the tables is never used as an index
    const bool inside = (uint32_t)u < (uint32_t)md.n_users && (uint32_t)i < n_items && (uint32_t)j < n_items;
    const int M = md.n_models;
    for (int m = 0; m < M; ++m) {                                // uniform: the model's pointers are scalar loads of the argument block
        float d = __builtin_nanf("");
        if (inside) {
            const int k = md.m[m].k;
            const float* const vp[2] = {md.m[m].V + (size_t)i * k, md.m[m].V + (size_t)j * k};
            float acc[2];
            chain_scores<2>(md.m[m].U + (size_t)u * k, vp, k, acc);
            d = chain_finish(acc[0], md.m[m].bias, i) - chain_finish(acc[1], md.m[m].bias, j);
        }
        D_out[t * M + m] = d;
    }
}

// M: the number of models, a compile-time constant so that W, the row and the M sums stay in registers; VEC: the rows of D are
// 16-byte aligned (M % 4 == 0 and D itself aligned) and come in float4 loads.  (A row per thread means a wave's loads are M * 4 bytes
// apart: with one dword load per column every cache line is walked M times.  Measured: DESIGN.md section 4 K16.)
template <int M, bool VEC>
__global__ __launch_bounds__(kSgdThreads) void fusion_sgd_kernel(const float* __restrict__ D, int batch, int64_t n_batches, float lr,
                                                                float lambda_w, float* __restrict__ W, float* __restrict__ loss_out) {
    __shared__ float Wl[kFusionMax];
    __shared__ float red[kSgdWaves][kFusionMax + 1];
    constexpr int kRowsInFlight = M <= 4 ? 4 : 2;
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    if (tid < M) Wl[tid] = W[tid];
    __syncthreads();
    for (int64_t b = 0; b < n_batches; ++b) {
        float w[M], g[M];
#pragma unroll
        for (int m = 0; m < M; ++m) { w[m] = Wl[m]; g[m] = 0.f; }
        float loss = 0.f;
        const float* Db = D + (size_t)b * batch * M;
#pragma unroll kRowsInFlight
        for (int r = tid; r < batch; r += kSgdThreads) {
            const float* row = Db + (size_t)r * M;
            float d[M];
            if constexpr (VEC) {
#pragma unroll
                for (int m = 0; m < M; m += 4) {
                    const float4 v = *reinterpret_cast<const float4*>(row + m);
                    d[m] = v.x; d[m + 1] = v.y; d[m + 2] = v.z; d[m + 3] = v.w;
                }
            } else {
#pragma unroll
                for (int m = 0; m < M; ++m) d[m] = row[m];
            }
            float x = 0.f;
#pragma unroll
            for (int m = 0; m < M; ++m) x = fmaf(w[m], d[m], x);
            const float sg = sigmoid_neg(x);
            loss = loss + softplus_neg(x);
#pragma unroll
            for (int m = 0; m < M; ++m) g[m] = fmaf(sg, d[m], g[m]);
        }
#pragma unroll
        for (int m = 0; m < M; ++m) g[m] = wave_sum(g[m]);
        loss = wave_sum(loss);
        if (lane == 0) {
#pragma unroll
            for (int m = 0; m < M; ++m) red[wave][m] = g[m];
            red[wave][kFusionMax] = loss;
        }
        __syncthreads();
        if (tid < M) {                                           // column tid: the waves in wave order, then the step on the W of this batch
            float s = 0.f;
            for (int q = 0; q < kSgdWaves; ++q) s = s + red[q][tid];
            const float wm = Wl[tid];
            Wl[tid] = wm + lr * (s - lambda_w * wm);
        } else if (tid == TKR_WAVE && loss_out) {                // a thread of another wave: the loss of this batch, on the same W
            float s = 0.f, ww = 0.f;
            for (int q = 0; q < kSgdWaves; ++q) s = s + red[q][kFusionMax];
#pragma unroll
            for (int m = 0; m < M; ++m) ww = fmaf(w[m], w[m], ww);
            loss_out[b] = s + 0.5f * lambda_w * ww;
        }
        __syncthreads();
    }
    if (tid < M) W[tid] = Wl[tid];
}

template <int M>
static void launch_sgd(const float* D, int batch, int64_t n_batches, float lr, float lambda_w, float* W, float* loss_out, hipStream_t stream) {
    if constexpr (M % 4 == 0) {
        if (((uintptr_t)D & 15) == 0) {
            hipLaunchKernelGGL((fusion_sgd_kernel<M, true>), dim3(1), dim3(kSgdThreads), 0, stream, D, batch, n_batches, lr, lambda_w, W, loss_out);
            return;
        }
    }
    hipLaunchKernelGGL((fusion_sgd_kernel<M, false>), dim3(1), dim3(kSgdThreads), 0, stream, D, batch, n_batches, lr, lambda_w, W, loss_out);
}

__global__ __launch_bounds__(kUwWaves * TKR_WAVE) void fusion_user_weights_kernel(
    const tkr_fusion_models md, const int64_t* __restrict__ like_ptr, const int32_t* __restrict__ like_cols, float* __restrict__ rmse_out,
    float* __restrict__ w_out) {
    const int lane = threadIdx.x & 63;
    const int64_t u = (int64_t)blockIdx.x * kUwWaves + (threadIdx.x >> 6);
    if (u >= md.n_users) return;
    const int64_t e0 = like_ptr[u], len = like_ptr[u + 1] - e0;
    const int M = md.n_models;
    const float n = (float)(len > 1 ? len : 1);
    float mine = 0.f, total = 0.f;                               // lane m keeps r[u, m]; total is uniform
    for (int m = 0; m < M; ++m) {
        const int k = md.m[m].k;
        const float* up = md.m[m].U + (size_t)u * k;
        float acc = 0.f;
        for (int64_t e = lane; e < len; e += 64) {
            const int c = like_cols[e0 + e];
            // a column outside the table is never dereferenced: the user's figures come out NaN
            float s = __builtin_nanf("");
            if ((uint32_t)c < (uint32_t)md.n_items) {
                const float* const vp[1] = {md.m[m].V + (size_t)c * k};
                float one[1];
                chain_scores<1>(up, vp, k, one);
                s = chain_finish(one[0], md.m[m].bias, c);
            }
            const float err = s - 1.0f;
            acc = fmaf(err, err, acc);
        }
        const float r = sqrtf(wave_sum(acc) / n);
        total = total + r;
        if (lane == m) mine = r;
    }
    const float mean = total / (float)M;
    if (lane < M) {
        rmse_out[u * M + lane] = mine;
        w_out[u * M + lane] = mean == 0.f ? 1.0f : expf(-(mine - mean));
    }
}

static bool models_ok(const tkr_fusion_models* md) {
    if (!md || md->n_models < 1 || md->n_models > kFusionMax || md->n_users < 1 || md->n_items < 1) return false;
    for (int m = 0; m < md->n_models; ++m)
        if (!md->m[m].U || !md->m[m].V || md->m[m].k < 1) return false;
    return true;
}

}  // namespace tkr

extern "C" int tkr_fusion_features(const tkr_fusion_models* models, const int32_t* tr_users, int32_t n_tr, const int32_t* row_ptr,
                                   const int32_t* pos_cols, const int32_t* cols_sorted, int32_t n_items, uint64_t seed,
                                   uint64_t first_triplet, int64_t count, float* D_out, int32_t* trip_out, void* stream_) {
    if (!tkr::models_ok(models) || !tr_users || !row_ptr || !pos_cols || !cols_sorted || !D_out) return TKR_EINVAL;
    if (n_tr < 1 || n_items < 1 || n_items != models->n_items || count < 1 || count > ((int64_t)1 << 31) * 256 - 256) return TKR_EINVAL;
    hipLaunchKernelGGL(tkr::fusion_features_kernel, dim3((unsigned)((count + 255) / 256)), dim3(256), 0, (hipStream_t)stream_, *models,
                       tr_users, (uint32_t)n_tr, row_ptr, pos_cols, cols_sorted, (uint32_t)n_items, seed, first_triplet, count, D_out,
                       trip_out);
    TKR_LAUNCH_CHECK();
    return TKR_OK;
}

extern "C" int tkr_fusion_sgd(const float* D, int64_t n_rows, int32_t n_models, int32_t batch, int64_t n_batches, float lr, float lambda_w,
                              float* W, float* loss_out, void* stream_) {
    if (!D || !W || n_models < 1 || n_models > tkr::kFusionMax || batch < 1 || n_batches < 1 || n_rows < 1) return TKR_EINVAL;
    if (n_batches > n_rows / batch) return TKR_EINVAL;           // every batch lies inside D
    hipStream_t stream = (hipStream_t)stream_;
    switch (n_models) {
#define TKR_SGD_CASE(M) case M: tkr::launch_sgd<M>(D, batch, n_batches, lr, lambda_w, W, loss_out, stream); break;
        TKR_SGD_CASE(1) TKR_SGD_CASE(2) TKR_SGD_CASE(3) TKR_SGD_CASE(4) TKR_SGD_CASE(5) TKR_SGD_CASE(6) TKR_SGD_CASE(7) TKR_SGD_CASE(8)
        TKR_SGD_CASE(9) TKR_SGD_CASE(10) TKR_SGD_CASE(11) TKR_SGD_CASE(12) TKR_SGD_CASE(13) TKR_SGD_CASE(14) TKR_SGD_CASE(15) TKR_SGD_CASE(16)
#undef TKR_SGD_CASE
    }
    TKR_LAUNCH_CHECK();
    return TKR_OK;
}

extern "C" int tkr_fusion_user_weights(const tkr_fusion_models* models, const int64_t* like_ptr, const int32_t* like_cols, int32_t n_users,
                                       float* rmse_out, float* w_out, void* stream_) {
    if (!tkr::models_ok(models) || !like_ptr || !like_cols || !rmse_out || !w_out) return TKR_EINVAL;
    if (n_users < 1 || n_users != models->n_users) return TKR_EINVAL;
    hipLaunchKernelGGL(tkr::fusion_user_weights_kernel, dim3((unsigned)((n_users + tkr::kUwWaves - 1) / tkr::kUwWaves)),
                       dim3(tkr::kUwWaves * TKR_WAVE), 0, (hipStream_t)stream_, *models, like_ptr, like_cols, rmse_out, w_out);
    TKR_LAUNCH_CHECK();
    return TKR_OK;
}
