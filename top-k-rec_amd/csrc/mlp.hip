// K22 -- a dense MLP content encoder (d -> hidden .. -> k, sigmoid hidden layers, linear output) applied and trained on the GPU: the
// encoder of DPM (top-k-rec_amd/als.py MLP, DPM; the reference's single/mlp.py, single/dpm.py).  include/tkr.h states the contract.
//
//   mlp_check_kernel        the pre-pass over `rows` / `order`: status = 4 t + 1 for the smallest t whose index lies outside [0, n).
//                           EVERY later kernel of the call reads the status word first and returns when it is not -1: nothing
//                           refused is used as an index, and a refused call writes no parameter, slot or output.
//   mlp_gemm_kernel<TRANS>  one 64 x 64 tile of  C = A B  per workgroup and slab of the contraction: four waves, a 32 x 32 block each
//                           on the exact-fp32 MFMA (v_mfma_f32_32x32x2_f32: per element one fp32 fma chain in contraction order from
//                           +0.0).  A is [m, kdim] (its rows gathered through `rows` for the first layer), B = W [kdim, n] (forward)
//                           or W^T with W [n, kdim] (TRANS: a delta carried back through a layer).  The contraction is cut into slabs
//                           of TKR_MLP_SLAB, one workgroup each, so that a wide W is streamed by ceil(kdim / SLAB) times more
//                           workgroups than the output has tiles; a slab's sum goes to an fp32 partial [slab][m][n] in the workspace.
//   mlp_reduce_kernel       adds the partials in ascending slab order in fp64, rounds once, then bias and activation (forward) or
//                           the factor h (1 - h) (a delta).
//   mlp_loss_kernel         one workgroup: delta_L = F - Y[rows], batch_loss = 1/2 sum (y - F)^2 with differences and sum in fp64.
//   mlp_update_kernel       the fused step of one layer: a workgroup owns a 64 x 64 tile of W, stages the batch's input activations
//                           and deltas 32 rows at a time in LDS, forms g = A^T delta on the MFMA (one fma chain per element in batch
//                           order from +0.0) and applies dense RMSProp to the tile in registers: W and its slot are read once and
//                           stored once, g never exists in memory.  The bias gradient is the same chain with A = 1 (the workgroups
//                           of the first row of tiles).
// Staging: a tile read along the contraction ([row][c], the operand whose memory runs along c) has a pitch of 33 floats, one read
// across it ([c][col]) a pitch of 64: a ds_read_b32 is served per 32-lane half over 32 banks, and both are conflict-free there.
// No float atomics; the only atomic is the status word's minimum.  Every fp32 operation of this file is rounded on its own:
#pragma clang fp contract(off)
#include "tkr_common.h"
#include "../../include/tkr.h"

#include <limits.h>
#include <math.h>

#include <algorithm>

namespace tkr {

typedef float mlp_f32x16 __attribute__((ext_vector_type(16)));

constexpr int kMlpBlock = 256;
constexpr int kMlpTile = 64;                                      // a workgroup's tile edge: 2 x 2 waves of 32 x 32
constexpr int kMlpStep = 32;                                      // contraction entries staged at a time
constexpr int kMlpPitchT = kMlpStep + 1;                          // [row][c]
constexpr int kMlpPitchN = kMlpTile;                              // [c][col]
constexpr int kMlpSlab = TKR_MLP_SLAB;
constexpr int kMlpChunk = TKR_MLP_FORWARD_CHUNK;
constexpr int kMlpMaxWidth = 1 << 21;                             // a grid's y and z dimensions stay below 65,536
constexpr unsigned long long kMlpClean = ~0ull;
static_assert(kMlpSlab % kMlpStep == 0 && kMlpChunk % kMlpTile == 0, "whole steps, whole tiles");

enum { kMlpLinear = 0, kMlpSigmoid = 1, kMlpDelta = 2 };
enum { kMlpBadIndex = 1 };                                        // the one kind of K22's status word: entry `where` of rows / order is outside [0, n)

// row of the 32 x 32 block that register `reg` of lane half h holds (the column is the lane & 31)
__device__ __forceinline__ int mlp_acc_row(int reg, int h) { return (reg & 3) + 8 * (reg >> 2) + 4 * h; }

__global__ __launch_bounds__(kMlpBlock) void mlp_check_kernel(const int32_t* __restrict__ idx, long long m, int n,
                                                              unsigned long long* __restrict__ status) {
    for (long long t = (long long)blockIdx.x * kMlpBlock + threadIdx.x; t < m; t += (long long)gridDim.x * kMlpBlock)
        if ((uint32_t)idx[t] >= (uint32_t)n) status_refuse(status, t, kMlpBadIndex);
}

template <bool TRANS>
__global__ __launch_bounds__(kMlpBlock) void mlp_gemm_kernel(const float* __restrict__ A, int lda, const int32_t* __restrict__ rows, int m,
                                                             const float* __restrict__ W, int ldw, int kdim, int n,
                                                             float* __restrict__ partial, const unsigned long long* __restrict__ status) {
    __shared__ float As[kMlpTile * kMlpPitchT];
    __shared__ float Bs[TRANS ? kMlpTile * kMlpPitchT : kMlpStep * kMlpPitchN];
    if (*status != kMlpClean) return;                             // (the same word in every thread of the grid)
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, l31 = lane & 31, h = lane >> 5;
    const int wi = wave >> 1, wj = wave & 1;
    const int m0 = blockIdx.y * kMlpTile, n0 = blockIdx.x * kMlpTile;
    const int c_lo = blockIdx.z * kMlpSlab, c_hi = min(kdim, c_lo + kMlpSlab);
    // the staged rows of A this thread brings: row (tid >> 5) + 8 q, column tid & 31 of the step
    const float* a_row[kMlpTile / 8];
#pragma unroll
    for (int q = 0; q < kMlpTile / 8; ++q) {
        const int t = m0 + (tid >> 5) + 8 * q;
        a_row[q] = t < m ? A + (size_t)(rows ? rows[t] : t) * lda : nullptr;
    }
    mlp_f32x16 acc;
#pragma unroll
    for (int reg = 0; reg < 16; ++reg) acc[reg] = 0.f;
    for (int c0 = c_lo; c0 < c_hi; c0 += kMlpStep) {              // workgroup-uniform
        {
            const int c = c0 + l31;
#pragma unroll
            for (int q = 0; q < kMlpTile / 8; ++q) As[((tid >> 5) + 8 * q) * kMlpPitchT + l31] = (a_row[q] && c < c_hi) ? a_row[q][c] : 0.f;
        }
        if constexpr (TRANS) {                                    // B(c, i) = W[i][c]: memory runs along c, staged as A is
            const int c = c0 + l31;
#pragma unroll
            for (int q = 0; q < kMlpTile / 8; ++q) {
                const int ii = (tid >> 5) + 8 * q, i = n0 + ii;
                Bs[ii * kMlpPitchT + l31] = (i < n && c < c_hi) ? W[(size_t)i * ldw + c] : 0.f;
            }
        } else {                                                  // B(c, j) = W[c][j]: memory runs along j
            const int jj = tid & 63, j = n0 + jj;
#pragma unroll
            for (int q = 0; q < kMlpStep / 4; ++q) {
                const int cc = (tid >> 6) + 4 * q, c = c0 + cc;
                Bs[cc * kMlpPitchN + jj] = (j < n && c < c_hi) ? W[(size_t)c * ldw + j] : 0.f;
            }
        }
        __syncthreads();
        const float* ap = As + (wi * 32 + l31) * kMlpPitchT + h;
        const float* bp = TRANS ? Bs + (wj * 32 + l31) * kMlpPitchT + h : Bs + h * kMlpPitchN + wj * 32 + l31;
#pragma unroll
        for (int t = 0; t < kMlpStep; t += 2)
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(ap[t], TRANS ? bp[t] : bp[t * kMlpPitchN], acc, 0, 0, 0);
        __syncthreads();
    }
    float* out = partial + (size_t)blockIdx.z * (size_t)m * (size_t)n;
    const int j = n0 + wj * 32 + l31;
#pragma unroll
    for (int reg = 0; reg < 16; ++reg) {
        const int t = m0 + wi * 32 + mlp_acc_row(reg, h);
        if (t < m && j < n) out[(size_t)t * n + j] = acc[reg];
    }
}

// out[t][j], t < m, j < n: z = fp32(sum over the slabs in fp64), then
//   kMlpLinear   z + bias[j]
//   kMlpSigmoid  1 / (1 + expf(-(z + bias[j])))
//   kMlpDelta    z * (h * (1 - h)), h = act[t][j]: the delta of a sigmoid layer from what came back through the layer above it
__global__ __launch_bounds__(kMlpBlock) void mlp_reduce_kernel(const float* __restrict__ partial, int n_slabs, long long mn, int n,
                                                               const float* __restrict__ bias, const float* __restrict__ act, int mode,
                                                               float* __restrict__ out, const unsigned long long* __restrict__ status) {
    if (*status != kMlpClean) return;
    const long long idx = (long long)blockIdx.x * kMlpBlock + threadIdx.x;
    if (idx >= mn) return;
    double s = 0.0;
    for (int b = 0; b < n_slabs; ++b) s += (double)partial[(size_t)b * (size_t)mn + idx];
    const float z = (float)s;
    if (mode == kMlpDelta) {
        const float hv = act[idx];
        out[idx] = z * (hv * (1.f - hv));
        return;
    }
    const float x = z + bias[idx % n];
    out[idx] = mode == kMlpSigmoid ? 1.f / (1.f + expf(-x)) : x;
}

__global__ __launch_bounds__(kMlpBlock) void mlp_loss_kernel(const float* __restrict__ F, const float* __restrict__ Y,
                                                             const int32_t* __restrict__ rows, int bn, int k, float* __restrict__ delta,
                                                             double* __restrict__ loss_out, const unsigned long long* __restrict__ status) {
    __shared__ double red[kMlpBlock];
    if (*status != kMlpClean) return;
    const int tid = threadIdx.x;
    double s = 0.0;
    for (int idx = tid; idx < bn * k; idx += kMlpBlock) {
        const int b = idx / k, j = idx - b * k;
        const float y = Y[(size_t)rows[b] * k + j], f = F[idx];
        delta[idx] = f - y;
        const double d = (double)y - (double)f;
        s += d * d;
    }
    red[tid] = s;
    __syncthreads();
    if (tid == 0) {
        double total = 0.0;
        for (int i = 0; i < kMlpBlock; ++i) total += red[i];
        *loss_out = 0.5 * total;
    }
}

// dense RMSProp of oracle/ref_np.py:338-341, every operation rounded on its own (the file runs with contraction off; division and
// square root are correctly rounded)
__device__ __forceinline__ void mlp_rmsprop(float* __restrict__ w, float* __restrict__ ms, float g, float lr) {
    constexpr float rho = 0.9f, one_minus_rho = 1.0f - rho, eps = 1e-10f;
    const float q = g * g;
    const float m0 = *ms;
    const float m1 = m0 + (q - m0) * one_minus_rho;
    *ms = m1;
    *w = *w - (lr * g) / sqrtf(m1 + eps);
}

__global__ __launch_bounds__(kMlpBlock) void mlp_update_kernel(const float* __restrict__ A, int lda, const int32_t* __restrict__ rows, int bn,
                                                               const float* __restrict__ delta, int n_in, int n_out, float* __restrict__ W,
                                                               float* __restrict__ msW, float* __restrict__ bias, float* __restrict__ msb,
                                                               float lr, const unsigned long long* __restrict__ status) {
    __shared__ float As[kMlpStep * kMlpPitchN];                   // [b][i]
    __shared__ float Ds[kMlpStep * kMlpPitchN];                   // [b][j]
    if (*status != kMlpClean) return;
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, l31 = lane & 31, h = lane >> 5;
    const int wi = wave >> 1, wj = wave & 1;
    const int i0 = blockIdx.y * kMlpTile, j0 = blockIdx.x * kMlpTile;
    const bool with_bias = blockIdx.y == 0 && wi == 0;            // (wave-uniform)
    mlp_f32x16 acc, accb;
#pragma unroll
    for (int reg = 0; reg < 16; ++reg) acc[reg] = accb[reg] = 0.f;
    const int cc = tid & 63;
    for (int b0 = 0; b0 < bn; b0 += kMlpStep) {                   // workgroup-uniform
#pragma unroll
        for (int q = 0; q < kMlpStep / 4; ++q) {
            const int bb = (tid >> 6) + 4 * q, b = b0 + bb;
            float a = 0.f, d = 0.f;
            if (b < bn) {
                if (i0 + cc < n_in) a = A[(size_t)(rows ? rows[b] : b) * lda + i0 + cc];
                if (j0 + cc < n_out) d = delta[(size_t)b * n_out + j0 + cc];
            }
            As[bb * kMlpPitchN + cc] = a;
            Ds[bb * kMlpPitchN + cc] = d;
        }
        __syncthreads();
        const float* ap = As + h * kMlpPitchN + wi * 32 + l31;
        const float* dp = Ds + h * kMlpPitchN + wj * 32 + l31;
#pragma unroll
        for (int t = 0; t < kMlpStep; t += 2) {
            const float d = dp[t * kMlpPitchN];
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(ap[t * kMlpPitchN], d, acc, 0, 0, 0);
            if (with_bias) accb = __builtin_amdgcn_mfma_f32_32x32x2f32(1.0f, d, accb, 0, 0, 0);      // (a padded row has d = 0)
        }
        __syncthreads();
    }
    const int j = j0 + wj * 32 + l31;
    if (j >= n_out) return;
#pragma unroll
    for (int reg = 0; reg < 16; ++reg) {
        const int i = i0 + wi * 32 + mlp_acc_row(reg, h);
        if (i < n_in) {
            const size_t at = (size_t)i * n_out + j;
            mlp_rmsprop(W + at, msW + at, acc[reg], lr);
        }
    }
    if (with_bias && h == 0) mlp_rmsprop(bias + j, msb + j, accb[0], lr);      // every row of the block holds the column's sum
}

static int64_t mlp_align(int64_t floats) { return (floats + 3) / 4 * 4; }      // pieces of the workspace start on 16 bytes
static int64_t mlp_slabs(int64_t kdim) { return (kdim + kMlpSlab - 1) / kMlpSlab; }

// the shape of the net alone: what the workspace is sized by
static int mlp_check_shape(const tkr_mlp_net* net) {
    if (!net || net->n_layers < 1 || net->n_layers > TKR_MLP_MAX_LAYERS) return TKR_EINVAL;
    for (int l = 0; l <= net->n_layers; ++l)
        if (net->width[l] < 1) return TKR_EINVAL;
    for (int l = 0; l <= net->n_layers; ++l)
        if (net->width[l] > kMlpMaxWidth) return TKR_EUNSUPPORTED;
    return TKR_OK;
}

static int mlp_check_net(const tkr_mlp_net* net, bool with_slots) {
    if (!net || net->n_layers < 1 || net->n_layers > TKR_MLP_MAX_LAYERS) return TKR_EINVAL;
    for (int l = 0; l < net->n_layers; ++l) {
        if (!net->W[l] || !net->bias[l] || ((uintptr_t)net->W[l] & 3) || ((uintptr_t)net->bias[l] & 3)) return TKR_EINVAL;
        if (with_slots && (!net->msW[l] || !net->msb[l] || ((uintptr_t)net->msW[l] & 3) || ((uintptr_t)net->msb[l] & 3))) return TKR_EINVAL;
    }
    return mlp_check_shape(net);
}

// floats of the slab partials of `r` rows: every layer forwards, and (backward) every layer but the first carries a delta back
static int64_t mlp_partial_floats(const tkr_mlp_net* net, int64_t r, bool backward) {
    int64_t most = 0;
    for (int l = 0; l < net->n_layers; ++l) {
        most = std::max(most, mlp_slabs(net->width[l]) * r * net->width[l + 1]);
        if (backward && l > 0) most = std::max(most, mlp_slabs(net->width[l + 1]) * r * net->width[l]);
    }
    return mlp_align(most);
}

static int64_t mlp_forward_floats(const tkr_mlp_net* net, int64_t m) {
    const int64_t r = std::min<int64_t>(m, kMlpChunk);
    int64_t hidden = 0;
    for (int l = 1; l < net->n_layers; ++l) hidden = std::max<int64_t>(hidden, net->width[l]);
    return 2 * mlp_align(r * hidden) + mlp_partial_floats(net, r, false);
}

static int64_t mlp_fit_floats(const tkr_mlp_net* net, int64_t batch) {
    int64_t total = mlp_partial_floats(net, batch, true);
    for (int l = 0; l < net->n_layers; ++l) total += 2 * mlp_align(batch * net->width[l + 1]);
    return total;
}

// out [r][width[l + 1]] = layer l applied to the r rows of `in` (gathered through `rows` where it is not null)
static int mlp_layer_forward(hipStream_t stream, const tkr_mlp_net* net, int l, const float* in, const int32_t* rows, int r, float* partial,
                             float* out, const unsigned long long* st) {
    const int n_in = net->width[l], n_out = net->width[l + 1], n_slabs = (int)mlp_slabs(n_in);
    const dim3 grid((n_out + kMlpTile - 1) / kMlpTile, (r + kMlpTile - 1) / kMlpTile, n_slabs);
    hipLaunchKernelGGL(mlp_gemm_kernel<false>, grid, dim3(kMlpBlock), 0, stream, in, n_in, rows, r, (const float*)net->W[l], n_out, n_in, n_out,
                       partial, st);
    TKR_LAUNCH_CHECK();
    const long long mn = (long long)r * n_out;
    hipLaunchKernelGGL(mlp_reduce_kernel, dim3((unsigned)((mn + kMlpBlock - 1) / kMlpBlock)), dim3(kMlpBlock), 0, stream, (const float*)partial,
                       n_slabs, mn, n_out, (const float*)net->bias[l], (const float*)nullptr, l + 1 < net->n_layers ? kMlpSigmoid : kMlpLinear, out,
                       st);
    TKR_LAUNCH_CHECK();
    return TKR_OK;
}

static int mlp_check_rows(hipStream_t stream, const int32_t* idx, int64_t m, int n, unsigned long long* st) {
    TKR_CHECK(hipMemsetAsync(st, 0xff, sizeof(unsigned long long), stream));          // -1: nothing refused
    if (!idx || m == 0) return TKR_OK;
    const unsigned blocks = (unsigned)std::min<int64_t>((m + kMlpBlock - 1) / kMlpBlock, 2048);
    hipLaunchKernelGGL(mlp_check_kernel, dim3(blocks), dim3(kMlpBlock), 0, stream, idx, (long long)m, n, st);
    TKR_LAUNCH_CHECK();
    return TKR_OK;
}

}  // namespace tkr

extern "C" int64_t tkr_mlp_workspace_bytes(const tkr_mlp_net* net, int64_t m, int32_t batch) {
    if (m < 0 || batch < 0 || batch > TKR_MLP_MAX_BATCH || tkr::mlp_check_shape(net) != TKR_OK) return TKR_EINVAL;
    return 4 * std::max(tkr::mlp_forward_floats(net, m), batch > 0 ? tkr::mlp_fit_floats(net, batch) : 0);
}

extern "C" int tkr_mlp_forward(const tkr_mlp_net* net, const float* X, int32_t n, const int32_t* rows, int64_t m, float* out, void* workspace,
                               int64_t workspace_bytes, int64_t* status, void* stream_) {
    using namespace tkr;
    TKR_CHECK_RC(mlp_check_net(net, false));
    if (!X || !out || !status || ((uintptr_t)X & 3) || ((uintptr_t)out & 3) || ((uintptr_t)rows & 3) || ((uintptr_t)status & 7) ||
        ((uintptr_t)workspace & 15))
        return TKR_EINVAL;
    if (n < 1 || m < 0 || (!rows && m > n) || workspace_bytes < 0) return TKR_EINVAL;
    if (m > 0 && (!workspace || workspace_bytes < 4 * mlp_forward_floats(net, m))) return TKR_EINVAL;
    hipStream_t stream = (hipStream_t)stream_;
    unsigned long long* st = reinterpret_cast<unsigned long long*>(status);
    TKR_CHECK_RC(mlp_check_rows(stream, rows, m, n, st));
    if (m == 0) return TKR_OK;
    const int L = net->n_layers, k = net->width[L];
    const int64_t r_most = std::min<int64_t>(m, kMlpChunk);
    int64_t hidden = 0;
    for (int l = 1; l < L; ++l) hidden = std::max<int64_t>(hidden, net->width[l]);
    float* ws = reinterpret_cast<float*>(workspace);
    float* buf[2] = {ws, ws + mlp_align(r_most * hidden)};
    float* partial = ws + 2 * mlp_align(r_most * hidden);
    for (int64_t c0 = 0; c0 < m; c0 += kMlpChunk) {
        const int r = (int)std::min<int64_t>(kMlpChunk, m - c0);
        const float* in = rows ? X : X + (size_t)c0 * net->width[0];
        const int32_t* in_rows = rows ? rows + c0 : nullptr;
        for (int l = 0; l < L; ++l) {
            float* dst = l + 1 < L ? buf[l & 1] : out + (size_t)c0 * k;
            TKR_CHECK_RC(mlp_layer_forward(stream, net, l, in, in_rows, r, partial, dst, st));
            in = dst;
            in_rows = nullptr;
        }
    }
    return TKR_OK;
}

extern "C" int tkr_mlp_fit(const tkr_mlp_net* net, const float* X, int32_t n, const float* Y, const int32_t* order, int64_t m, int32_t batch,
                           float lr, double* batch_loss, void* workspace, int64_t workspace_bytes, int64_t* status, void* stream_) {
    using namespace tkr;
    TKR_CHECK_RC(mlp_check_net(net, true));
    if (!X || !Y || !status || ((uintptr_t)X & 3) || ((uintptr_t)Y & 3) || ((uintptr_t)order & 3) || ((uintptr_t)status & 7) ||
        ((uintptr_t)batch_loss & 7) || ((uintptr_t)workspace & 15))
        return TKR_EINVAL;
    if (n < 1 || m < 0 || batch < 1 || !std::isfinite(lr) || lr < 0.f || workspace_bytes < 0) return TKR_EINVAL;
    if (batch > TKR_MLP_MAX_BATCH) return TKR_EUNSUPPORTED;
    if (m > 0 && (!order || !batch_loss || !workspace || workspace_bytes < 4 * mlp_fit_floats(net, batch))) return TKR_EINVAL;
    hipStream_t stream = (hipStream_t)stream_;
    unsigned long long* st = reinterpret_cast<unsigned long long*>(status);
    TKR_CHECK_RC(mlp_check_rows(stream, order, m, n, st));
    if (m == 0) return TKR_OK;
    const int L = net->n_layers, k = net->width[L];
    float* ws = reinterpret_cast<float*>(workspace);
    float *act[TKR_MLP_MAX_LAYERS], *delta[TKR_MLP_MAX_LAYERS];
    for (int l = 0; l < L; ++l) {
        act[l] = ws;
        ws += mlp_align((int64_t)batch * net->width[l + 1]);
        delta[l] = ws;
        ws += mlp_align((int64_t)batch * net->width[l + 1]);
    }
    float* partial = ws;
    const int64_t n_batches = (m + batch - 1) / batch;
    for (int64_t t = 0; t < n_batches; ++t) {
        const int32_t* rows = order + t * batch;
        const int bn = (int)std::min<int64_t>(batch, m - t * batch);
        // 1. forward, the activations kept
        for (int l = 0; l < L; ++l)
            TKR_CHECK_RC(mlp_layer_forward(stream, net, l, l ? act[l - 1] : X, l ? nullptr : rows, bn, partial, act[l], st));
        // 2. the objective before the update, and delta_L = F - Y
        hipLaunchKernelGGL(mlp_loss_kernel, dim3(1), dim3(kMlpBlock), 0, stream, (const float*)act[L - 1], Y, rows, bn, k, delta[L - 1],
                           batch_loss + t, st);
        TKR_LAUNCH_CHECK();
        // 3. delta_{l-1} = (delta_l W_l^T) h (1 - h), through the parameters as they were
        for (int l = L - 1; l >= 1; --l) {
            const int n_in = net->width[l], n_out = net->width[l + 1], n_slabs = (int)mlp_slabs(n_out);
            const dim3 grid((n_in + kMlpTile - 1) / kMlpTile, (bn + kMlpTile - 1) / kMlpTile, n_slabs);
            hipLaunchKernelGGL(mlp_gemm_kernel<true>, grid, dim3(kMlpBlock), 0, stream, (const float*)delta[l], n_out, (const int32_t*)nullptr, bn,
                               (const float*)net->W[l], n_out, n_out, n_in, partial, st);
            TKR_LAUNCH_CHECK();
            const long long mn = (long long)bn * n_in;
            hipLaunchKernelGGL(mlp_reduce_kernel, dim3((unsigned)((mn + kMlpBlock - 1) / kMlpBlock)), dim3(kMlpBlock), 0, stream,
                               (const float*)partial, n_slabs, mn, n_in, (const float*)nullptr, (const float*)act[l - 1], kMlpDelta, delta[l - 1], st);
            TKR_LAUNCH_CHECK();
        }
        // 4. every layer's gradient and step in one launch
        for (int l = 0; l < L; ++l) {
            const int n_in = net->width[l], n_out = net->width[l + 1];
            const dim3 grid((n_out + kMlpTile - 1) / kMlpTile, (n_in + kMlpTile - 1) / kMlpTile);
            hipLaunchKernelGGL(mlp_update_kernel, grid, dim3(kMlpBlock), 0, stream, l ? (const float*)act[l - 1] : X, n_in, l ? nullptr : rows, bn,
                               (const float*)delta[l], n_in, n_out, net->W[l], net->msW[l], net->bias[l], net->msb[l], lr, st);
            TKR_LAUNCH_CHECK();
        }
    }
    return TKR_OK;
}
