// K18 -- what a resampling method needs from a full-rank evaluation: the metric values of every test line, and sums of them over
// lines drawn with replacement.
//
//   line_metrics_kernel        a wave per test line.  The line's ranks >= 0 become bits of a bitmap of n_cols bits in LDS (integer OR
//                              atomics, as K15; the bit that is already there is a rank named twice), P, sum rho and rho_0 are integer
//                              reductions over the wave, and lane b walks the bits below K_b = step (b + 1) in ascending order: hits,
//                              the DCG and the precision sum of bucket b, added sequentially from 0.0.  gain and ideal are the caller's
//                              tables: no logarithm here, every float operation is one IEEE add or divide.  The bitmap is zeroed once
//                              per workgroup; a line clears its own bits again (a second pass over its ranks), so a line costs its
//                              length, not n_cols.  Nothing read from the input is used as an index before it is checked.
//   bootstrap_partial_kernel   a wave per (replicate r, chunk of kBootChunk draws).  64 lanes draw 128 line indices (one Philox block
//                              each, stream word 3); LPR lanes -- the power of two >= C, at least 8 -- read one row of X together, so
//                              64 / LPR rows per load instruction, 16 loads in flight per lane.  Rows lie `pitch` doubles apart: a
//                              pitch of whole 64- / 128-byte lines (the wrapper pads to one) reads 14-27 % faster than 184- or
//                              368-byte rows that straddle lines.  Lane group g adds its draws in
//                              ascending order, the groups are added in a butterfly, the chunk's sums go to the workspace.
//   bootstrap_finish_kernel    out[r, c] = the chunks' sums, chunk ascending.
// The summation tree of the bootstrap depends on (n, C) alone -- not on the pitch: no float atomics, the same bits in every run.
#include "tkr_common.h"
#include "../../include/tkr.h"

#include <limits.h>

namespace tkr {

constexpr int kLineRows = 4;                                      // lines (waves) of one workgroup at most
constexpr size_t kLineLdsBudget = 160 * 1024;                     // what one CU holds
constexpr int kLineMaxGrid = 2048;
constexpr int kBootChunk = TKR_BOOT_CHUNK;                        // draws one wave sums: part of the definition of the result's bits
constexpr int kBootWaves = 4;
constexpr int kBootMaxGrid = 1 << 16;
constexpr int kBootInFlight = 16;                                 // loads a lane issues before it adds
static_assert(kBootChunk % 128 == 0, "a wave draws 128 lines at a time");
static_assert((size_t)TKR_LINE_MAX_COLS / 8 <= kLineLdsBudget, "one line's bitmap fits one workgroup");

enum { kBadRankLow = 0, kBadRankHigh = 1, kBadRankTwice = 2, kBadLinePtr = 3 };

__global__ __launch_bounds__(kLineRows * TKR_WAVE) void line_metrics_kernel(const int32_t* __restrict__ ranks, int64_t n_likes,
                                                                          const int64_t* __restrict__ like_ptr,
                                                                          const int64_t* __restrict__ rated_ptr, int64_t n_lines, int n_cols,
                                                                          int step, int interval, int W, const double* __restrict__ gain,
                                                                          const double* __restrict__ ideal, double* __restrict__ X,
                                                                          unsigned long long* __restrict__ status) {
#pragma clang fp contract(off)
    extern __shared__ __attribute__((aligned(16))) uint32_t line_lds[];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, rows = blockDim.x >> 6;
    uint32_t* bm = line_lds + (size_t)wave * W;                    // W words: max(n_cols, total) bits
    const int C = 3 * interval + 5;
    if (blockIdx.x == 0 && threadIdx.x == 0 && (like_ptr[0] != 0 || rated_ptr[0] != 0)) status_refuse(status, 0, kBadLinePtr);
    for (int w = lane; w < W; w += TKR_WAVE) bm[w] = 0u;
    __syncthreads();
    for (int64_t base = (int64_t)blockIdx.x * rows; base < n_lines; base += (int64_t)gridDim.x * rows) {     // uniform over the workgroup
        const int64_t r = base + wave;
        const bool active = r < n_lines;
        int64_t lo = 0, hi = 0;
        int cap = 0;                                               // the line's unrated columns: a rank is below it
        bool ok = false;
        if (active) {
            lo = like_ptr[r];
            hi = like_ptr[r + 1];
            const int64_t rlo = rated_ptr[r], rhi = rated_ptr[r + 1];
            ok = lo >= 0 && hi >= lo && hi <= n_likes && rlo >= 0 && rhi >= rlo && rhi - rlo <= (int64_t)n_cols;
            if (!ok && lane == 0) status_refuse(status, r, kBadLinePtr);
            cap = ok ? n_cols - (int)(rhi - rlo) : 0;
        }
        int P = 0, first = INT_MAX, bad = 4;                      // the smallest kind this lane met
        int64_t sum = 0;
        if (ok) {
            for (int64_t e = lo + lane; e < hi; e += TKR_WAVE) {
                const int rk = ranks[e];
                if (rk < -1) {
                    bad = kBadRankLow;
                } else if (rk >= cap) {
                    bad = min(bad, (int)kBadRankHigh);             // never a bit index
                } else if (rk >= 0) {
                    const uint32_t bit = 1u << (rk & 31);
                    if (atomicOr(&bm[rk >> 5], bit) & bit) bad = min(bad, (int)kBadRankTwice);
                    ++P;
                    sum += rk;
                    first = min(first, rk);
                }
            }
        }
        if (bad < 4) status_refuse(status, r, bad);
        const bool good = ok && __ballot(bad < 4) == 0ull;        // uniform over the wave
        for (int d = 32; d; d >>= 1) {
            P += __shfl_xor(P, d);
            sum += __shfl_xor(sum, d);
            first = min(first, __shfl_xor(first, d));
        }
        __syncthreads();                                           // the line's bits are set
        if (active) {
            double* row = X + (size_t)r * C;
            if (!good) {
                for (int c = lane; c < C; c += TKR_WAVE) row[c] = 0.0;
            } else {
                if (lane == 0) {
                    const int64_t N = (int64_t)cap - P;
                    const bool pairs = P >= 1 && N >= 1;
                    row[interval] = (double)(hi - lo);
                    row[interval + 1] = pairs ? 1.0 - (double)(sum - (int64_t)P * (P - 1) / 2) / (double)((int64_t)P * N) : 0.0;
                    row[interval + 2] = pairs ? 1.0 : 0.0;
                    row[interval + 3] = P >= 1 ? 1.0 / (double)(first + 1) : 0.0;
                    row[interval + 4] = P >= 1 ? 1.0 : 0.0;
                }
                for (int b = lane; b < interval; b += TKR_WAVE) {
                    const int K = step * (b + 1);                  // <= total: inside gain, ideal and the bitmap
                    int q = 0;
                    double dcg = 0.0, ap = 0.0;
                    for (int w = 0; w * 32 < K; ++w) {
                        uint32_t bits = bm[w];
                        if (K - w * 32 < 32) bits &= (1u << (K - w * 32)) - 1u;
                        while (bits) {
                            const int rho = w * 32 + __ffs(bits) - 1;
                            bits &= bits - 1u;
                            ++q;
                            dcg = dcg + gain[rho];
                            ap = ap + (double)q / (double)(rho + 1);
                        }
                    }
                    const int depth = min(P, K);
                    row[b] = (double)q;
                    row[interval + 5 + b] = P >= 1 ? dcg / ideal[depth] : 0.0;
                    row[2 * interval + 5 + b] = P >= 1 ? ap / (double)depth : 0.0;
                }
            }
        }
        __syncthreads();                                           // every lane has read the bits
        if (ok) {
            for (int64_t e = lo + lane; e < hi; e += TKR_WAVE) {
                const int rk = ranks[e];
                if (rk >= 0 && rk < cap) atomicAnd(&bm[rk >> 5], ~(1u << (rk & 31)));
            }
        }
        __syncthreads();                                           // the bitmap is empty again
    }
}

template <int LPR>
__global__ __launch_bounds__(kBootWaves * TKR_WAVE) void bootstrap_partial_kernel(const double* __restrict__ X, int64_t n, int C,
                                                                                int64_t pitch, int64_t n_chunks, int64_t n_tasks, uint32_t k0,
                                                                                uint32_t k1, double* __restrict__ partial) {
    constexpr int G = TKR_WAVE / LPR;                              // rows one load instruction reads
    constexpr int SUB = 128 / G;                                   // load instructions per 128 draws
    static_assert(SUB % kBootInFlight == 0, "whole batches of loads");
    const int lane = threadIdx.x & 63;
    const int g = lane / LPR, c = lane % LPR;
    const bool col = c < C;
    for (int64_t task = (int64_t)blockIdx.x * kBootWaves + (threadIdx.x >> 6); task < n_tasks; task += (int64_t)gridDim.x * kBootWaves) {
        const int64_t r = task / n_chunks, chunk = task - r * n_chunks;
        const int64_t t0 = chunk * kBootChunk, t1 = min(n, t0 + (int64_t)kBootChunk);
        double acc = 0.0;
        for (int64_t tb = t0; tb < t1; tb += 128) {                // uniform over the wave
            const uint64_t p = (uint64_t)(tb >> 1) + (uint64_t)lane;
            const u32x4 w = philox4x32_10((uint32_t)p, (uint32_t)(p >> 32), (uint32_t)r, 3u, k0, k1);
            const int even = (int)mulhi64(w.x, w.y, (uint32_t)n), odd = (int)mulhi64(w.z, w.w, (uint32_t)n);       // both in [0, n)
            for (int j0 = 0; j0 < SUB && tb + (int64_t)j0 * G < t1; j0 += kBootInFlight) {
                double v[kBootInFlight];
#pragma unroll
                for (int u = 0; u < kBootInFlight; ++u) {
                    const int d = (j0 + u) * G + g;                // the draw tb + d: of Philox block d >> 1
                    const int a = __shfl(even, d >> 1), b = __shfl(odd, d >> 1);
                    const int idx = (d & 1) ? b : a;
                    v[u] = (col && tb + d < t1) ? X[(size_t)idx * pitch + c] : 0.0;
                }
#pragma unroll
                for (int u = 0; u < kBootInFlight; ++u) acc += v[u];
            }
        }
        for (int off = LPR; off < TKR_WAVE; off <<= 1) acc += __shfl_xor(acc, off);
        if (g == 0 && col) partial[(size_t)task * C + c] = acc;
    }
}

__global__ __launch_bounds__(256) void bootstrap_finish_kernel(const double* __restrict__ partial, int64_t n_out, int64_t n_chunks, int C,
                                                              double* __restrict__ out) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n_out; i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t r = i / C;
        const int c = (int)(i - r * C);
        double sum = 0.0;
        for (int64_t k = 0; k < n_chunks; ++k) sum += partial[(size_t)(r * n_chunks + k) * C + c];
        out[i] = sum;
    }
}

}  // namespace tkr

extern "C" int tkr_line_metrics(const int32_t* ranks, int64_t n_likes, const int64_t* like_ptr, const int64_t* rated_ptr, int64_t n_lines,
                                int32_t n_cols, int32_t step, int32_t total, const double* gain, const double* ideal, double* X,
                                int64_t* status, void* stream_) {
    if (!like_ptr || !rated_ptr || !gain || !ideal || !X || !status || (!ranks && n_likes != 0)) return TKR_EINVAL;
    if ((((uintptr_t)like_ptr | (uintptr_t)rated_ptr | (uintptr_t)gain | (uintptr_t)ideal | (uintptr_t)X | (uintptr_t)status) & 7) ||
        ((uintptr_t)ranks & 3))
        return TKR_EINVAL;
    if (n_likes < 0 || n_lines < 1 || n_cols < 1 || step < 1 || total < 1) return TKR_EINVAL;
    if (total > TKR_LINE_MAX_TOTAL || n_cols > TKR_LINE_MAX_COLS) return TKR_EUNSUPPORTED;
    hipStream_t stream = (hipStream_t)stream_;
    unsigned long long* st = reinterpret_cast<unsigned long long*>(status);
    TKR_CHECK(hipMemsetAsync(st, 0xff, sizeof(unsigned long long), stream));          // -1: nothing refused
    const int W = ((n_cols > total ? n_cols : total) + 31) >> 5;
    const size_t fit = tkr::kLineLdsBudget / ((size_t)W * 4);
    const int rows = fit >= (size_t)tkr::kLineRows ? tkr::kLineRows : (int)fit;      // >= 1: TKR_LINE_MAX_COLS bits fit
    const size_t lds = (size_t)rows * W * 4;
    if (lds > 64 * 1024)
        TKR_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(tkr::line_metrics_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                      (int)tkr::kLineLdsBudget));
    const int64_t groups = (n_lines + rows - 1) / rows;
    const int grid = (int)(groups < tkr::kLineMaxGrid ? groups : tkr::kLineMaxGrid);
    hipLaunchKernelGGL(tkr::line_metrics_kernel, dim3(grid), dim3(rows * TKR_WAVE), lds, stream, ranks, n_likes, like_ptr, rated_ptr, n_lines,
                       n_cols, step, total / step, W, gain, ideal, X, st);
    TKR_LAUNCH_CHECK();
    return TKR_OK;
}

extern "C" int tkr_bootstrap_sums(const double* X, int64_t n, int32_t C, int64_t pitch, int32_t R, uint64_t seed, double* out,
                                  void* workspace, int64_t workspace_bytes, void* stream_) {
    if (!X || !out || !workspace || (((uintptr_t)X | (uintptr_t)out | (uintptr_t)workspace) & 7)) return TKR_EINVAL;
    if (C < 1 || C > TKR_BOOT_MAX_COLUMNS || n < 1 || n > (int64_t)INT32_MAX || R < 1 || pitch < C) return TKR_EINVAL;
    const int64_t n_chunks = (n + tkr::kBootChunk - 1) / tkr::kBootChunk, n_tasks = (int64_t)R * n_chunks;
    if (workspace_bytes < n_tasks * C * 8) return TKR_EINVAL;
    hipStream_t stream = (hipStream_t)stream_;
    double* partial = reinterpret_cast<double*>(workspace);
    const uint32_t k0 = (uint32_t)seed, k1 = (uint32_t)(seed >> 32);
    const int64_t groups = (n_tasks + tkr::kBootWaves - 1) / tkr::kBootWaves;
    const int grid = (int)(groups < tkr::kBootMaxGrid ? groups : tkr::kBootMaxGrid);
    auto kern = C <= 8 ? tkr::bootstrap_partial_kernel<8> : C <= 16 ? tkr::bootstrap_partial_kernel<16>
              : C <= 32 ? tkr::bootstrap_partial_kernel<32> : tkr::bootstrap_partial_kernel<64>;
    hipLaunchKernelGGL(kern, dim3(grid), dim3(tkr::kBootWaves * TKR_WAVE), 0, stream, X, n, (int)C, pitch, n_chunks, n_tasks,
                       k0, k1, partial);
    TKR_LAUNCH_CHECK();
    const int64_t n_out = (int64_t)R * C, fgroups = (n_out + 255) / 256;
    hipLaunchKernelGGL(tkr::bootstrap_finish_kernel, dim3((int)(fgroups < tkr::kBootMaxGrid ? fgroups : tkr::kBootMaxGrid)), dim3(256), 0, stream,
                       partial, n_out, n_chunks, (int)C, out);
    TKR_LAUNCH_CHECK();
    return TKR_OK;
}
