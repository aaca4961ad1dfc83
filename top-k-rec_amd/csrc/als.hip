// K20 -- the two kernels of implicit-feedback ALS (WMF; top-k-rec_amd/als.py); K21, their content-aware form (CER), below.  One half-step of the alternation is
//
//   G = scale * sum over the rated rows y of  y y^T  (+ ridge I)                               tkr_als_gram
//   for every row r with likes:  (G + w_like * sum_{y in L_r} y y^T + ridge I) x_r = w_rhs * sum_{y in L_r} y      tkr_als_solve_rows
//
// Both are built on ONE piece of code, slab_sum (csrc/als_parts.h): a workgroup of 256 threads sums y y^T over a list of rows of Y.  The rows are
// gathered 32 at a time into LDS (columns padded with zeros to whole 32-blocks, a refused row staged as zeros), and the four waves
// multiply the tile with itself on the exact-fp32 MFMA (v_mfma_f32_32x32x2_f32): the contraction runs over the staged rows, two per
// instruction, so every element of the sum is one fp32 fma chain in list order -- the same bits run to run.  Only the 32 x 32 blocks
// on and above the diagonal are computed (1 / 3 / 6 / 10 of them at k <= 32 / 64 / 96 / 128, dealt round-robin to the waves); a * b
// and b * a are the same product, so the mirrored element has the same bits.
//
//   als_slab_kernel<KT>     one workgroup per slab of TKR_ALS_GRAM_SLAB listed rows -> an fp32 partial [k * k | k column sums | count]
//                           in the workspace.  Two uses: the slabs of tkr_als_gram's row list, and the slabs of the HEAVY rows of a
//                           solve (a row with heavy_from likes or more: several workgroups share it).
//   als_wide_slab_kernel    K24, tkr_als_gram_wide: the slab sum for k <= 512, the slab's rows staged as slab_sum stages them, the
//                           32 x 32 blocks on and above the diagonal dealt to passes of 12 (blockIdx.y), 3 per wave:
//                           the accumulators als_slab_kernel<4> holds.  An element is the same fp32 fma chain in list order whichever
//                           pass and wave has its block, so for k <= 128 the partials are K20's.  No column sums, no count.
//   als_gram_reduce_kernel  the one reduce of both Grams: adds the partials in ascending slab order in fp64, applies scale and ridge,
//                           rounds once (s * scale + ridge in this file's contraction mode, the default: that fixes its bits).
//   als_plan_kernel         (solve, only when a row can be heavy) one workgroup walks like_ptr, gives every heavy row its slabs of the
//                           workspace in row order (a block-wide scan) and writes heavy_base[row] (-1: the row sums its own likes)
//                           and slab_row[slab]; a row whose slabs do not fit the workspace sums its own likes.
//   als_solve_kernel<KT>    one workgroup per row.  A (k x k, and the right-hand side as row k) in LDS at a pitch of 16 mod 64 floats,
//                           so the 4 x 16 elements a wave touches at a time lie in 64 different banks.  Cholesky, right-looking, with
//                           the lower triangle in registers (thread (ty, tx) owns the elements (ty + 16 ii, tx + 16 cc)): per column
//                           its owners publish it through LDS, ONE barrier, every thread scales what it needs and updates its own
//                           elements; the right-hand side rides along, which IS the forward substitution.  Wave 0 substitutes back
//                           with the solution in registers.  The upper triangle of A is never written and the diagonal without the
//                           ridge is kept apart: the row's loss needs them after the factorisation.  Every barrier is in
//                           workgroup-uniform control flow: the loop bounds are k, the row's (checked) length and flags every
//                           thread reads from the same LDS word.
//
// K21 -- the same half-step with a prior on every row, every row solved (CER; tkr_als_solve_rows_prior):
//   als_solve_kernel<KT, kAlsPrior>   the per-row kernel with w_prior * prior[r] added to the right-hand side and 1/2 w_prior |x - prior[r]|^2
//                           to the loss; rows without likes are not its business.
//   als_solve_kernel<KT, kAlsFactor>  one workgroup: fp32(G + ridge I), the matrix every row without likes has, factorised ONCE per call
//                           by the per-row kernel's own Cholesky (a mode of the same template, not a copy); L goes to the workspace.
//   als_cold_kernel<KT>     a lane per row without likes: L in LDS, read wave-uniformly, z and x in registers, two triangular
//                           substitutions by dot products over contiguous rows (of L, then of L^T).
// No float atomics; the only atomic is the status word's minimum.  Nothing refused is used as an index.
#include "als_parts.h"

#include <math.h>

#include <algorithm>

namespace tkr {

constexpr int kAlsMaxSlabs = 1 << 20;                             // heavy slabs of one solve, at most (the plan kernel scans ints)

// floats between two rows of A: the smallest pitch >= k that is 16 mod 64
__host__ __device__ inline int als_a_pitch(int k) { return (k + 47) / 64 * 64 + 16; }
__host__ __device__ inline int64_t als_partial_stride(int k) { return (int64_t)k * k + k + 1; }

// like_ptr == nullptr: slab b of the list (rows, n_listed).  Otherwise slab b of the plan: row slab_row[b] (< 0: nothing to do), its
// likes first + s * SLAB .., s = b - heavy_base[row].
template <int KT>
__global__ __launch_bounds__(kAlsBlock) void als_slab_kernel(const float* __restrict__ Y, int n, int k, const int32_t* __restrict__ list,
                                                             long long n_listed, const int64_t* __restrict__ like_ptr,
                                                             const int32_t* __restrict__ slab_row, const int32_t* __restrict__ heavy_base,
                                                             float* __restrict__ partial, unsigned long long* __restrict__ status) {
    __shared__ float stage[kAlsTile * als_stage_pitch(KT)];
    __shared__ int cols_s[kAlsTile];
    const int tid = threadIdx.x;
    const long long b = blockIdx.x;
    long long first, word_row = -1;
    int count;
    if (like_ptr) {
        const int r = slab_row[b];
        if (r < 0) return;                                        // (uniform)
        const long long lo = like_ptr[r], hi = like_ptr[r + 1];   // checked by the plan kernel, which made r a heavy row
        first = lo + (b - heavy_base[r]) * (long long)kAlsSlab;
        count = (int)min((long long)kAlsSlab, hi - first);
        word_row = r;
    } else {
        first = b * (long long)kAlsSlab;
        count = (int)min((long long)kAlsSlab, n_listed - first);
    }
    als_f32x16 acc[als_tiles_per_wave(KT)];
    als_zero(acc);
    double col_sum = 0.0;
    int n_valid = 0;
    slab_sum<KT>(Y, n, k, list, first, count, stage, cols_s, acc, col_sum, n_valid, word_row, status);
    float* out = partial + (size_t)b * (size_t)als_partial_stride(k);
    als_emit<KT>(acc, k, [&](int p, int q, float v) { out[p * k + q] = v; });
    if (tid < k) out[k * k + tid] = (float)col_sum;
    if (tid == 0) out[k * k + k] = (float)n_valid;
}

// K24: the slab sum at any width up to 512: slab_sum's staging, product and emit with the blocks of the triangle dealt to passes, the
// stage in dynamic LDS (above 64 KB from k = 481), no column sums and no count.  It restates those three steps and does not call
// pieces of slab_sum: slab_sum and als_emit written over shared pieces are the same arithmetic, but the compiler gave als_slab_kernel
// and als_solve_kernel other instructions (other scalar registers at KT = 1 and 3, 6 waves per SIMD for 7 in als_solve_kernel<1>, and
// 1.3 % on the K20 iteration at k = 128).  A change to the staging is a change in both places; test_gram_wide_has_the_bits_of_gram
// holds them to the same bits.
constexpr int kWideTpw = als_tiles_per_wave(4);                   // blocks per wave and pass: als_slab_kernel<4>'s accumulators
constexpr int kWidePass = kWideTpw * kAlsWaves;

// grid (slabs, passes): the blocks 12 blockIdx.y .. of slab blockIdx.x -> partial [slab][k * k], both triangles
__global__ __launch_bounds__(kAlsBlock) void als_wide_slab_kernel(const float* __restrict__ Y, int n, int k, const int32_t* __restrict__ list,
                                                                 long long n_listed, float* __restrict__ partial,
                                                                 unsigned long long* __restrict__ status) {
    extern __shared__ __attribute__((aligned(16))) float als_lds[];
    const int KT = (k + 31) / 32, SP = als_stage_pitch(KT), NT = als_tiles(KT);
    float* stage = als_lds;                                         // [32][SP]
    int* cols_s = reinterpret_cast<int*>(als_lds + kAlsTile * SP);
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, l31 = lane & 31, h = lane >> 5;
    const long long first = (long long)blockIdx.x * kAlsSlab;
    const int count = (int)(n_listed - first < (long long)kAlsSlab ? n_listed - first : (long long)kAlsSlab);
    const int idx0 = blockIdx.y * kWidePass + wave;
    int bi[kWideTpw], bj[kWideTpw];
    als_f32x16 acc[kWideTpw];
#pragma unroll
    for (int s = 0; s < kWideTpw; ++s) {
        bi[s] = bj[s] = 0;
        if (idx0 + kAlsWaves * s < NT) als_tile_of(KT, idx0 + kAlsWaves * s, bi[s], bj[s]);
#pragma unroll
        for (int reg = 0; reg < 16; ++reg) acc[s][reg] = 0.f;
    }
    for (int base = 0; base < count; base += kAlsTile) {           // workgroup-uniform
        const int n_here = count - base < kAlsTile ? count - base : kAlsTile;
        if (tid < kAlsTile) {
            int c = -1;
            if (tid < n_here) {
                const long long t = first + base + tid;
                c = list ? list[t] : (int)t;
                if ((uint32_t)c >= (uint32_t)n) {
                    status_refuse(status, t, kAlsSkipped);
                    c = -1;
                }
            }
            cols_s[tid] = c;
        }
        __syncthreads();
        for (int q = tid >> 5; q < kAlsTile * KT; q += kAlsBlock / 32) {         // 32 lanes bring 32 consecutive floats of a row
            const int rr = q / KT, col = (q - rr * KT) * 32 + l31;
            const int c = cols_s[rr];
            stage[rr * SP + col] = (c >= 0 && col < k) ? Y[(size_t)c * k + col] : 0.f;
        }
        __syncthreads();
#pragma unroll
        for (int s = 0; s < kWideTpw; ++s) {
            if (idx0 + kAlsWaves * s < NT) {                       // wave-uniform
                const float* ap = stage + h * SP + bi[s] * 32 + l31;
                const float* bp = stage + h * SP + bj[s] * 32 + l31;
#pragma unroll 4
                for (int t = 0; t < kAlsTile; t += 2)
                    acc[s] = __builtin_amdgcn_mfma_f32_32x32x2f32(ap[t * SP], bp[t * SP], acc[s], 0, 0, 0);
            }
        }
        __syncthreads();
    }
    float* out = partial + (size_t)blockIdx.x * (size_t)k * (size_t)k;
#pragma unroll
    for (int s = 0; s < kWideTpw; ++s) {
        if (idx0 + kAlsWaves * s < NT) {
            const int q = bj[s] * 32 + l31;
#pragma unroll
            for (int reg = 0; reg < 16; ++reg) {
                const int p = bi[s] * 32 + (reg & 3) + 8 * (reg >> 2) + 4 * h;
                if (p < k && q < k) {
                    out[(size_t)p * k + q] = acc[s][reg];
                    if (bi[s] != bj[s]) out[(size_t)q * k + p] = acc[s][reg];
                }
            }
        }
    }
}

// partial: [n_slabs][stride] floats, the k * k sums in front (stride: als_partial_stride(k), or k * k for the wide slabs)
__global__ __launch_bounds__(kAlsBlock) void als_gram_reduce_kernel(const float* __restrict__ partial, long long n_slabs, size_t stride, int k,
                                                                    double scale, double ridge, float* __restrict__ G) {
    const int idx = blockIdx.x * kAlsBlock + threadIdx.x;
    if (idx >= k * k) return;
    double s = 0.0;
    for (long long b = 0; b < n_slabs; ++b) s += (double)partial[(size_t)b * stride + idx];
    const int p = idx / k, q = idx - p * k;
    G[idx] = (float)(s * scale + (p == q ? ridge : 0.0));
}

constexpr int kAlsPlanBlock = 1024;
__global__ __launch_bounds__(kAlsPlanBlock) void als_plan_kernel(const int64_t* __restrict__ like_ptr, long long n_likes, long long n_x,
                                                                 long long heavy_from, int cap, int32_t* __restrict__ heavy_base,
                                                                 int32_t* __restrict__ slab_row) {
    __shared__ int wave_sum_s[kAlsPlanBlock / TKR_WAVE];
    __shared__ long long running_s;
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    if (tid == 0) running_s = 0;
    __syncthreads();
    for (long long r0 = 0; r0 < n_x; r0 += kAlsPlanBlock) {       // workgroup-uniform
        const long long r = r0 + tid;
        long long ns = 0;
        if (r < n_x) {
            const long long lo = like_ptr[r], hi = like_ptr[r + 1];
            if (als_ptr_ok(lo, hi, n_likes, r) && hi - lo >= heavy_from && hi > lo) ns = (hi - lo + kAlsSlab - 1) / kAlsSlab;
        }
        const int counted = (int)min(ns, (long long)cap + 1);     // what does not fit is never placed: the sums stay inside an int
        int incl = counted;
#pragma unroll
        for (int d = 1; d < TKR_WAVE; d <<= 1) {
            const int up = __shfl_up(incl, d);
            if (lane >= d) incl += up;
        }
        if (lane == TKR_WAVE - 1) wave_sum_s[wave] = incl;
        __syncthreads();
        long long base = running_s;
        for (int w = 0; w < wave; ++w) base += wave_sum_s[w];
        base += incl - counted;
        if (r < n_x) {
            const bool fits = ns > 0 && base + ns <= (long long)cap;
            heavy_base[r] = fits ? (int32_t)base : -1;
            if (fits)
                for (long long s = 0; s < ns; ++s) slab_row[base + s] = (int32_t)r;
        }
        __syncthreads();                                          // everyone has read running_s and the wave sums
        if (tid == 0) {
            long long total = running_s;
            for (int w = 0; w < kAlsPlanBlock / TKR_WAVE; ++w) total += wave_sum_s[w];
            running_s = min(total, (long long)cap + 1);
        }
        __syncthreads();
    }
}

// dynamic LDS of the solve kernel, in floats from the start (every piece a multiple of 4 floats)
struct AlsSolveLds {
    int a, stage, diag, ldiag, raw, xs, cs, misc, floats;
    __host__ __device__ AlsSolveLds(int k, int KT) {
        const int tile_floats = kAlsTile * als_stage_pitch(KT);
        const int stage_floats = tile_floats > 2 * kAlsBlock ? tile_floats : 2 * kAlsBlock;       // later: the 256 doubles of the loss
        a = 0;
        stage = a + (k + 1) * als_a_pitch(k);
        diag = stage + stage_floats;
        ldiag = diag + 128;
        raw = ldiag + 128;
        xs = raw + 256;
        cs = xs + 128;                                            // 128 doubles
        misc = cs + 256;                                          // cols_s [32], n_valid, fail
        floats = misc + 36;
    }
};

// The one per-row solve, and the ONE factorisation of this file, in three modes (the factor of K21's cold rows is this code, not a copy:
// a wrapper around a shared device function gave K20 other register numbers and 0.9 % at k = 128, one template does not); everything that differs is behind `if constexpr`, so
// kAlsK20 is K20's kernel as it was:
//   kAlsK20     tkr_als_solve_rows
//   kAlsPrior   K21, tkr_als_solve_rows_prior: the right-hand side adds w_prior * prior[r] and the loss 1/2 w_prior |x - prior[r]|^2; a
//               row without likes is the cold kernel's
//   kAlsFactor  K21, one workgroup: the "row" has no likes and no right-hand side, A = fp32(G + ridge I) as a row's diagonal is
//               rounded; after the factorisation L goes to `factor` (als_factor_floats) in place of a back substitution
enum { kAlsK20 = 0, kAlsPrior = 1, kAlsFactor = 2 };
__host__ __device__ inline int64_t als_factor_floats(int k) { return (int64_t)k * k + 4; }      // L row-major [k][k], one int: 1 = factorised

template <int KT, int MODE>
__global__ __launch_bounds__(kAlsBlock) void als_solve_kernel(const float* __restrict__ Y, int n_y, int k, const float* __restrict__ G,
                                                              const int64_t* __restrict__ like_ptr, const int32_t* __restrict__ like_cols,
                                                              long long n_likes, double w_like, double w_rhs, double ridge,
                                                              const int32_t* __restrict__ heavy_base, const float* __restrict__ partial,
                                                              float* __restrict__ X, double* __restrict__ row_loss,
                                                              unsigned long long* __restrict__ status, const float* __restrict__ prior,
                                                              double w_prior, float* __restrict__ factor) {
    constexpr bool PRIOR = MODE == kAlsPrior;
    extern __shared__ __attribute__((aligned(16))) float als_lds[];
    const AlsSolveLds at(k, KT);
    const int AP = als_a_pitch(k);
    float* A = als_lds + at.a;                                     // [k + 1][AP]: row k is the right-hand side
    float* stage = als_lds + at.stage;
    float* diag = als_lds + at.diag;                               // A's diagonal without the ridge
    float* ldiag = als_lds + at.ldiag;                             // the factor's diagonal
    float* raw = als_lds + at.raw;                                 // the column of the current step as its owners hold it, [2][128]
    float* xs = als_lds + at.xs;
    float* zf = xs;                                                // L^-1 rhs, until wave 0 has it in registers
    double* cs = reinterpret_cast<double*>(als_lds + at.cs);       // column sums of the row's likes
    double* red = reinterpret_cast<double*>(stage);                // [256], after the sums
    int* cols_s = reinterpret_cast<int*>(als_lds + at.misc);
    int* n_valid_s = cols_s + 32;
    int* fail_s = cols_s + 33;
    const int tid = threadIdx.x;
    const long long r = blockIdx.x;
    const unsigned long long word = (unsigned long long)r * 4ull;  // status_refuse's packing by hand: the two exits share the word

    // the row's likes: the same two words in every thread, so every exit below is taken by the whole workgroup
    const long long lo = MODE == kAlsFactor ? 0 : like_ptr[r], hi = MODE == kAlsFactor ? 0 : like_ptr[r + 1];
    if (!als_ptr_ok(lo, hi, n_likes, r)) {
        if (tid == 0) {
            atomicMin(status, word + kAlsBadPtr);                 // the row is left as it is
            if (row_loss) row_loss[r] = 0.0;
        }
        return;
    }
    const int m = (int)(hi - lo);
    if constexpr (MODE != kAlsFactor) {
        if (m == 0) {
            if constexpr (!PRIOR)
                if (tid == 0 && row_loss) row_loss[r] = 0.0;
            return;
        }
    }
    const int hb = heavy_base ? heavy_base[r] : -1;
    double col_sum = 0.0;
    int n_valid = 0;
    auto put = [&](int p, int q, double s) {                      // A[p][q] = fp32(G + w_like * s); the ridge on the diagonal, in the same rounding
        const double v = (double)G[p * k + q] + w_like * s;
        if (p == q) {
            diag[p] = (float)v;
            A[p * AP + p] = (float)(v + ridge);
        } else {
            A[p * AP + q] = (float)v;
        }
    };
    if constexpr (MODE == kAlsFactor) {
        for (int idx = tid; idx < k * k; idx += kAlsBlock) {
            const int p = idx / k;
            put(p, idx - p * k, 0.0);
        }
    } else if (hb < 0) {                                          // (uniform) the row sums its own likes
        als_f32x16 acc[als_tiles_per_wave(KT)];
        als_zero(acc);
        slab_sum<KT>(Y, n_y, k, like_cols, lo, m, stage, cols_s, acc, col_sum, n_valid, r, status);
        als_emit<KT>(acc, k, [&](int p, int q, float v) { put(p, q, (double)v); });
    } else {                                                      // its slabs were summed by the launch before this one
        const size_t stride = (size_t)als_partial_stride(k);
        const int n_slabs = (m + kAlsSlab - 1) / kAlsSlab;
        const float* mine = partial + (size_t)hb * stride;
        for (int idx = tid; idx < k * k; idx += kAlsBlock) {
            double s = 0.0;
            for (int b = 0; b < n_slabs; ++b) s += (double)mine[(size_t)b * stride + idx];
            const int p = idx / k;
            put(p, idx - p * k, s);
        }
        if (tid < k) {
            for (int b = 0; b < n_slabs; ++b) {
                col_sum += (double)mine[(size_t)b * stride + k * k + tid];
                n_valid += (int)mine[(size_t)b * stride + k * k + k];
            }
        }
    }
    float pv = 0.f;                                               // (PRIOR) the prior's element tid, kept for the loss
    if (tid < k) {
        cs[tid] = col_sum;
        if constexpr (PRIOR) {
            pv = prior[(size_t)r * k + tid];
            A[k * AP + tid] = (float)(w_rhs * col_sum + w_prior * (double)pv);      // both terms in fp64, rounded once
        } else {
            A[k * AP + tid] = (float)(w_rhs * col_sum);
        }
    }
    if (tid == 0) {
        *n_valid_s = n_valid;
        *fail_s = 0;
    }
    __syncthreads();
    const int nv = MODE == kAlsFactor ? 1 : *n_valid_s;
    if (nv == 0) {                                                // (uniform) every like was refused: as a row without likes
        if (tid == 0 && row_loss) row_loss[r] = 0.0;
        return;
    }

    // Cholesky of A + ridge I, right-looking, the lower triangle in REGISTERS: thread (ty, tx) owns the elements (ty + 16 ii, tx + 16 cc)
    // for good.  Per column j one barrier: the owners of column j publish it (still unscaled, the pivot among it) in `raw`, two buffers
    // in turn, so that a column is published while the slowest thread still reads the one before; then every thread scales the 2 NB
    // entries it needs and updates its own elements.  The owners store the scaled column into A's lower triangle for the back
    // substitution; the right-hand side (row k of A, in LDS) takes part in the same updates, which IS the forward substitution.
    constexpr int NB = 2 * KT;
    const int tx = tid & 15, ty = tid >> 4;
    float a[NB][NB];
#pragma unroll
    for (int ii = 0; ii < NB; ++ii)
#pragma unroll
        for (int cc = 0; cc < NB; ++cc) {
            const int i = ty + 16 * ii, c = tx + 16 * cc;
            a[ii][cc] = (c <= i && i < k) ? A[i * AP + c] : 0.f;
        }
    float* zrow = A + k * AP;
    raw[tid] = 0.f;                                               // [2][128] = one word per thread
    __syncthreads();
    bool ok = true;
#pragma unroll
    for (int jb = 0; jb < NB; ++jb) {
        for (int jj = 0; ok && jj < 16; ++jj) {                   // (uniform: k, and a pivot every thread reads from the same word)
            const int j = jb * 16 + jj;
            if (j >= k) break;
            float* rb = raw + (j & 1) * 128;
            if (tx == jj) {
#pragma unroll
                for (int ii = jb; ii < NB; ++ii) {
                    const int i = ty + 16 * ii;
                    if (i < k) rb[i] = a[ii][jb];
                }
            }
            __syncthreads();
            const float d = rb[j];
            if (!(d > 0.f) || !(d < INFINITY)) {
                ok = false;
                break;
            }
            const float l = sqrtf(d), inv = 1.0f / l;              // one square root and one division per column; the column is
            if (tid == 0) ldiag[j] = l;                            // scaled by the reciprocal (a wave issues every instruction of
            float li[NB], lc[NB];                                  // this loop alone on its SIMD: their number is the time)
#pragma unroll
            for (int q = jb; q < NB; ++q) {                        // (entries at k and above are zero since the start: never published)
                const int i = ty + 16 * q, c = tx + 16 * q;
                li[q] = i > j ? rb[i] * inv : 0.f;
                lc[q] = c > j ? rb[c] * inv : 0.f;
            }
            // no predicate: a column at or before j has lc = 0; an element above the diagonal (c > i, where cc == ii) is never read
#pragma unroll
            for (int ii = jb; ii < NB; ++ii)
#pragma unroll
                for (int cc = jb; cc <= ii; ++cc) a[ii][cc] = fmaf(-li[ii], lc[cc], a[ii][cc]);
            if (tx == jj) {
#pragma unroll
                for (int ii = jb; ii < NB; ++ii) {
                    const int i = ty + 16 * ii;
                    if (i > j && i < k) A[i * AP + j] = li[ii];
                }
            }
            if (tid < k && tid >= j) {
                const float zj = zrow[j] * inv;
                if (tid == j) zf[j] = zj;
                else zrow[tid] = fmaf(-zj, rb[tid] * inv, zrow[tid]);
            }
        }
    }
    __syncthreads();
    if constexpr (MODE == kAlsFactor) {
        int* flag = reinterpret_cast<int*>(factor + (size_t)k * k);
        if (ok) {                                                 // (uniform)
            for (int idx = tid; idx < k * k; idx += kAlsBlock) {
                const int p = idx / k, q = idx - p * k;
                factor[idx] = q < p ? A[p * AP + q] : (q == p ? ldiag[p] : 0.f);
            }
        }
        if (tid == 0) *flag = ok ? 1 : 0;
        return;
    }
    if (ok && tid < TKR_WAVE) {                                   // wave 0: L^T x = z, z and x in registers (element i in lane i & 63)
        const int lane = tid;
        float z0 = lane < k ? zf[lane] : 0.f, z1 = lane + 64 < k ? zf[lane + 64] : 0.f;
        float x0 = 0.f, x1 = 0.f;
        for (int j = k - 1; j >= 0; --j) {
            const float zj = j < 64 ? bcast_f(z0, j) : bcast_f(z1, j - 64);
            const float xj = zj / ldiag[j];
            if (lane < j) z0 = fmaf(-A[j * AP + lane], xj, z0);
            if (lane + 64 < j) z1 = fmaf(-A[j * AP + lane + 64], xj, z1);
            if (lane == (j & 63)) {
                if (j < 64) x0 = xj; else x1 = xj;
            }
        }
        const bool finite = fabsf(x0) < INFINITY && fabsf(x1) < INFINITY;      // (false for a NaN)
        if (__ballot(!finite) != 0ull) {
            if (lane == 0) *fail_s = 1;
        } else {
            if (lane < k) xs[lane] = x0;
            if (lane + 64 < k) xs[lane + 64] = x1;
        }
    }
    __syncthreads();
    if (!ok || *fail_s) {                                         // (uniform) not positive definite in fp32; nothing is written
        if (tid == 0) {
            atomicMin(status, word + kAlsNotSolved);
            if (row_loss) row_loss[r] = 0.0;
        }
        return;
    }
    if (tid < k) X[(size_t)r * k + tid] = xs[tid];
    if (row_loss) {                                               // (uniform) 1/2 x^T A x - w_rhs (sum y) . x + 1/2 w_rhs m: fp32 products, fp64 sums
        double t = 0.0;
        for (int idx = tid; idx < k * k; idx += kAlsBlock) {
            const int p = idx / k, q = idx - p * k;
            const float a = p < q ? A[p * AP + q] : (p > q ? A[q * AP + p] : diag[p]);
            t += (double)(a * xs[q]) * (double)xs[p];
        }
        t *= 0.5;
        if (tid < k) t -= w_rhs * (cs[tid] * (double)xs[tid]);
        red[tid] = t;
        if constexpr (PRIOR) {
            if (tid < k) {                                        // (cs[tid] is this thread's own word: read above, free now)
                const double d = (double)xs[tid] - (double)pv;
                cs[tid] = d * d;
            }
        }
        __syncthreads();
        if (tid == 0) {
            double s = 0.0;
            for (int i = 0; i < kAlsBlock; ++i) s += red[i];
            if constexpr (PRIOR) {
                double q = 0.0;
                for (int j = 0; j < k; ++j) q += cs[j];
                row_loss[r] = (s + 0.5 * w_rhs * (double)nv) + 0.5 * w_prior * q;
            } else {
                row_loss[r] = s + 0.5 * w_rhs * (double)nv;
            }
        }
    }
}

static int64_t als_align(int64_t bytes) { return (bytes + 15) / 16 * 16; }

template <int KT>
static int launch_slabs(hipStream_t stream, long long n_slabs, const float* Y, int n, int k, const int32_t* list, long long n_listed,
                        const int64_t* like_ptr, const int32_t* slab_row, const int32_t* heavy_base, float* partial, unsigned long long* st) {
    hipLaunchKernelGGL(als_slab_kernel<KT>, dim3((unsigned)n_slabs), dim3(kAlsBlock), 0, stream, Y, n, k, list, n_listed, like_ptr, slab_row,
                       heavy_base, partial, st);
    TKR_LAUNCH_CHECK();
    return TKR_OK;
}

static int launch_slabs_kt(int KT, hipStream_t stream, long long n_slabs, const float* Y, int n, int k, const int32_t* list, long long n_listed,
                           const int64_t* like_ptr, const int32_t* slab_row, const int32_t* heavy_base, float* partial, unsigned long long* st) {
    switch (KT) {
        case 1: return launch_slabs<1>(stream, n_slabs, Y, n, k, list, n_listed, like_ptr, slab_row, heavy_base, partial, st);
        case 2: return launch_slabs<2>(stream, n_slabs, Y, n, k, list, n_listed, like_ptr, slab_row, heavy_base, partial, st);
        case 3: return launch_slabs<3>(stream, n_slabs, Y, n, k, list, n_listed, like_ptr, slab_row, heavy_base, partial, st);
        default: return launch_slabs<4>(stream, n_slabs, Y, n, k, list, n_listed, like_ptr, slab_row, heavy_base, partial, st);
    }
}

template <int KT, bool PRIOR>
static int launch_solve(hipStream_t stream, long long n_x, const float* Y, int n_y, int k, const float* G, const int64_t* like_ptr,
                        const int32_t* like_cols, long long n_likes, double w_like, double w_rhs, double ridge, const int32_t* heavy_base,
                        const float* partial, float* X, double* row_loss, unsigned long long* st, const float* prior, double w_prior) {
    const size_t lds = (size_t)AlsSolveLds(k, KT).floats * 4;
    auto kern = als_solve_kernel<KT, PRIOR ? kAlsPrior : kAlsK20>;
    if (lds > 64 * 1024) TKR_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    hipLaunchKernelGGL(kern, dim3((unsigned)n_x), dim3(kAlsBlock), lds, stream, Y, n_y, k, G, like_ptr, like_cols, n_likes, w_like, w_rhs, ridge,
                       heavy_base, partial, X, row_loss, st, prior, w_prior, (float*)nullptr);
    TKR_LAUNCH_CHECK();
    return TKR_OK;
}

// ---- K21: the rows without likes of tkr_als_solve_rows_prior ------------------------------------------------------------------------------
// Every such row has the same matrix, fp32(G + ridge I): it is factorised ONCE per call (one workgroup runs
// als_solve_kernel in its factor mode) and the rows are two triangular substitutions each (als_cold_kernel).
// A lane per row, 256 rows per workgroup; a workgroup without a cold row leaves at once.  The factor sits in LDS at a pitch of 32 KT
// floats: every lane of a wave reads the same entry at the same time (a broadcast), at an address the compiler knows, so a row
// comes four entries per LDS instruction.  z, then x in its place, stays in registers (the loops are unrolled over 32 KT; the guards
// on k are wave-uniform).  Both substitutions are DOT products over a contiguous row in LDS, summed apart from the element they are
// taken from -- four fp32 fma chains from +0.0 over the terms i = 0, 1, 2, 3 mod 4, added as (s0 + s1) + (s2 + s3) -- and then ONE
// subtraction and ONE division: z_j = (b_j - sum_{i<j} L_ji z_i) / l_jj over row j of L, and, after the workgroup has put L^T where L
// was, x_j = (z_j - sum_{i>j} L_ij x_i) / l_jj over row j of L^T.  (Updating z_i in place, term by term, rounds every term at the size
// of z_i: measured 6 x 2^-23 of the solution against 0.8 for fp32 LAPACK where the sums are small beside z.)  Every lane runs the same
// chain on its own row: a row's bits depend on the factor, w_prior and its prior, not on n_x, its neighbours or its lane.  Priors come
// in and rows go out through a [64][33] LDS tile per wave, 32 columns at a time, so that global memory sees 32 consecutive floats of
// a row per half-wave.
constexpr int kAlsColdPitch = 33;
__host__ __device__ constexpr int als_cold_lds_floats(int KT) { return KT * 32 * KT * 32 + kAlsWaves * TKR_WAVE * kAlsColdPitch; }

template <int KT>
__global__ __launch_bounds__(kAlsBlock) void als_cold_kernel(const float* __restrict__ factor, int k, const int64_t* __restrict__ like_ptr,
                                                             long long n_likes, long long n_x, const float* __restrict__ prior, double w_prior,
                                                             float* __restrict__ X, double* __restrict__ row_loss,
                                                             unsigned long long* __restrict__ status) {
    constexpr int LP = KT * 32;
    extern __shared__ __attribute__((aligned(16))) float als_lds[];
    float* L = als_lds;                                            // [k][LP]: L, the lower triangle with the diagonal; later L^T
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, l31 = lane & 31;
    float* st = L + LP * LP + wave * (TKR_WAVE * kAlsColdPitch);      // this wave's tile
    const long long r = (long long)blockIdx.x * kAlsBlock + tid;
    bool cold = false;
    if (r < n_x) {
        const long long lo = like_ptr[r], hi = like_ptr[r + 1];
        cold = lo == hi && als_ptr_ok(lo, hi, n_likes, r);         // (a row like_ptr is wrong at: kind 3, the per-row kernel's)
    }
    if (*reinterpret_cast<const int*>(factor + (size_t)k * k) == 0) {      // (the same word in every thread of the grid)
        if (cold) {                                               // on the shared factor: every cold row refused, none touched
            status_refuse(status, r, kAlsNotSolved);
            if (row_loss) row_loss[r] = 0.0;
        }
        return;
    }
    if (!__syncthreads_or(cold)) return;                          // (uniform)
    for (int idx = tid; idx < k * k; idx += kAlsBlock) {
        const int p = idx / k, q = idx - p * k;
        L[p * LP + q] = factor[idx];
    }
    const unsigned long long mask = __ballot(cold);               // the wave's rows r0 + rr, rr = the lane that holds the row
    const long long r0 = r - lane;
    auto stage_prior = [&](int c) {                               // the wave's 64 rows, columns 32 c .. 32 c + 31 (zeros beyond k, in rows not cold)
        const int col = c * 32 + l31;
        for (int rr = lane >> 5; rr < TKR_WAVE; rr += 2)
            st[rr * kAlsColdPitch + l31] = ((mask >> rr) & 1ull) && col < k ? prior[(size_t)(r0 + rr) * k + col] : 0.f;
    };
    float z[LP];
#pragma unroll
    for (int c = 0; c < KT; ++c) {
        stage_prior(c);
        __syncthreads();                                          // (also: the factor is in LDS)
#pragma unroll
        for (int i = 0; i < 32; ++i) z[c * 32 + i] = (float)(w_prior * (double)st[lane * kAlsColdPitch + i]);
        __syncthreads();
    }
    // (the empty asm keeps the scheduler from fetching rows far ahead of their use: the registers are z's)
    if (mask != 0ull) {                                           // (wave-uniform; no barrier inside)
#pragma unroll
        for (int j = 0; j < LP; ++j) {
            if (j < k) {
                float s[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
                for (int i = 0; i < j; ++i) s[i & 3] = fmaf(L[j * LP + i], z[i], s[i & 3]);
                z[j] = (z[j] - ((s[0] + s[1]) + (s[2] + s[3]))) / L[j * LP + j];
                asm volatile("" ::: "memory");
            }
        }
    }
    __syncthreads();                                              // every wave is done with L: L^T takes its place
    for (int idx = tid; idx < k * LP; idx += kAlsBlock) {         // row p of L^T = column p of L, zeros from column k on
        const int p = idx / LP, q = idx - p * LP;
        L[idx] = q < k ? factor[q * k + p] : 0.f;
    }
    __syncthreads();
    if (mask != 0ull) {
#pragma unroll
        for (int j = LP - 1; j >= 0; --j) {
            if (j < k) {                                          // (x_i = z_i = 0 at i >= k, and L^T is zero-filled there: the sum runs to LP)
                float s[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
                for (int i = j + 1; i < LP; ++i) s[i & 3] = fmaf(L[j * LP + i], z[i], s[i & 3]);
                z[j] = (z[j] - ((s[0] + s[1]) + (s[2] + s[3]))) / L[j * LP + j];
                asm volatile("" ::: "memory");
            }
        }
    }
    bool finite = true;
    double q = 0.0;                                               // sum (x_j - p_j)^2, j ascending, in fp64
#pragma unroll
    for (int c = 0; c < KT; ++c) {
        stage_prior(c);
        __syncthreads();
#pragma unroll
        for (int i = 0; i < 32; ++i) {
            if (c * 32 + i < k) {
                finite = finite && fabsf(z[c * 32 + i]) < INFINITY;            // (false for a NaN)
                const double d = (double)z[c * 32 + i] - (double)st[lane * kAlsColdPitch + i];
                q += d * d;
            }
        }
        __syncthreads();
    }
    const bool write = cold && finite;
    if (cold) {
        if (!finite) status_refuse(status, r, kAlsNotSolved);     // on this row's own solution: left as it is
        if (row_loss) row_loss[r] = finite ? 0.5 * w_prior * q : 0.0;
    }
    const unsigned long long wmask = __ballot(write);
#pragma unroll
    for (int c = 0; c < KT; ++c) {
#pragma unroll
        for (int i = 0; i < 32; ++i) st[lane * kAlsColdPitch + i] = z[c * 32 + i];
        __syncthreads();
        const int col = c * 32 + l31;
        for (int rr = lane >> 5; rr < TKR_WAVE; rr += 2)
            if (((wmask >> rr) & 1ull) && col < k) X[(size_t)(r0 + rr) * k + col] = st[rr * kAlsColdPitch + l31];
        __syncthreads();
    }
}

template <int KT>
static int launch_cold(hipStream_t stream, long long n_x, int k, const float* G, double ridge, float* factor, const int64_t* like_ptr,
                       long long n_likes, const float* prior, double w_prior, float* X, double* row_loss, unsigned long long* st) {
    const size_t lds_f = (size_t)AlsSolveLds(k, KT).floats * 4, lds_c = (size_t)als_cold_lds_floats(KT) * 4;
    auto fk = als_solve_kernel<KT, kAlsFactor>;
    auto ck = als_cold_kernel<KT>;
    if (lds_f > 64 * 1024) TKR_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(fk), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_f));
    if (lds_c > 64 * 1024) TKR_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(ck), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_c));
    hipLaunchKernelGGL(fk, dim3(1), dim3(kAlsBlock), lds_f, stream, (const float*)nullptr, 0, k, G, (const int64_t*)nullptr, (const int32_t*)nullptr, 0ll,
                       0.0, 0.0, ridge, (const int32_t*)nullptr, (const float*)nullptr, (float*)nullptr, (double*)nullptr,
                       (unsigned long long*)nullptr, (const float*)nullptr, 0.0, factor);
    TKR_LAUNCH_CHECK();
    hipLaunchKernelGGL(ck, dim3((unsigned)((n_x + kAlsBlock - 1) / kAlsBlock)), dim3(kAlsBlock), lds_c, stream, factor, k, like_ptr, n_likes, n_x, prior,
                       w_prior, X, row_loss, st);
    TKR_LAUNCH_CHECK();
    return TKR_OK;
}

// what tkr_als_solve_rows and tkr_als_solve_rows_prior share: the checks, the plan of the heavy rows, the per-row launch.  prior ==
// nullptr is K20: its kernel instantiation, its launches.
static int als_solve(const float* Y, int32_t n_y, int32_t k, const float* G, const int64_t* like_ptr, const int32_t* like_cols, int64_t n_likes,
                     int64_t n_x, double w_like, double w_rhs, double ridge, int64_t heavy_from, float* X, double* row_loss, void* workspace,
                     int64_t workspace_bytes, int64_t* status, void* stream_, const float* prior, double w_prior) {
    if (!Y || !G || !like_ptr || !X || !status || ((uintptr_t)status & 7) || ((uintptr_t)workspace & 15) || ((uintptr_t)row_loss & 7))
        return TKR_EINVAL;
    if (n_likes < 0 || (n_likes > 0 && !like_cols) || n_y < 1 || n_x < 1 || n_x > (int64_t)INT_MAX || heavy_from < 1 || workspace_bytes < 0)
        return TKR_EINVAL;
    if (!std::isfinite(w_like) || !std::isfinite(w_rhs) || !std::isfinite(ridge) || ridge < 0.0) return TKR_EINVAL;
    TKR_CHECK_RC(als_check_k(k, TKR_ALS_MAX_K));
    float* factor = nullptr;
    if (prior) {                                                  // the factor takes the front of the workspace, K20's part follows
        const int64_t front = als_align(als_factor_floats(k) * 4);
        if (!workspace || workspace_bytes < front) return TKR_EINVAL;
        factor = reinterpret_cast<float*>(workspace);
        workspace = reinterpret_cast<unsigned char*>(workspace) + front;
        workspace_bytes -= front;
    }
    // the heavy rows' part of the workspace: heavy_base [n_x], slab_row [cap], the partials [cap]
    const int64_t stride = als_partial_stride(k);
    int64_t cap = 0;
    if (heavy_from <= n_likes) {                                  // otherwise no row can be heavy
        if (!workspace || workspace_bytes < als_align(n_x * 4)) return TKR_EINVAL;
        const int64_t most = n_likes / kAlsSlab + n_likes / heavy_from + 1;       // slabs the heavy rows can have together
        const int64_t room = workspace_bytes - als_align(n_x * 4);
        cap = std::min<int64_t>(std::min<int64_t>(most, kAlsMaxSlabs), room / (stride * 4 + 4));
        while (cap > 0 && als_align(cap * 4) + als_align(cap * stride * 4) > room) --cap;
    }
    hipStream_t stream = (hipStream_t)stream_;
    unsigned long long* st = reinterpret_cast<unsigned long long*>(status);
    TKR_CHECK(hipMemsetAsync(st, 0xff, sizeof(unsigned long long), stream));          // -1: nothing refused
    const int KT = (k + 31) / 32;
    int32_t* heavy_base = nullptr;
    float* partial = nullptr;
    if (cap > 0) {
        unsigned char* ws = reinterpret_cast<unsigned char*>(workspace);
        heavy_base = reinterpret_cast<int32_t*>(ws);
        int32_t* slab_row = reinterpret_cast<int32_t*>(ws + als_align(n_x * 4));
        partial = reinterpret_cast<float*>(ws + als_align(n_x * 4) + als_align(cap * 4));
        TKR_CHECK(hipMemsetAsync(slab_row, 0xff, (size_t)cap * 4, stream));           // -1: a slab nobody has
        hipLaunchKernelGGL(als_plan_kernel, dim3(1), dim3(kAlsPlanBlock), 0, stream, like_ptr, (long long)n_likes, (long long)n_x,
                           (long long)heavy_from, (int)cap, heavy_base, slab_row);
        TKR_LAUNCH_CHECK();
        TKR_CHECK_RC(launch_slabs_kt(KT, stream, cap, Y, n_y, k, like_cols, n_likes, like_ptr, slab_row, heavy_base, partial, st));
    }
#define TKR_ALS_SOLVE(KTT)                                                                                                                      \
    if (!prior)                                                                                                                                 \
        return launch_solve<KTT, false>(stream, n_x, Y, n_y, k, G, like_ptr, like_cols, (long long)n_likes, w_like, w_rhs, ridge, heavy_base,   \
                                        partial, X, row_loss, st, nullptr, 0.0);                                                               \
    TKR_CHECK_RC((launch_solve<KTT, true>(stream, n_x, Y, n_y, k, G, like_ptr, like_cols, (long long)n_likes, w_like, w_rhs, ridge, heavy_base, \
                                          partial, X, row_loss, st, prior, w_prior)));                                                         \
    return launch_cold<KTT>(stream, n_x, k, G, ridge, factor, like_ptr, (long long)n_likes, prior, w_prior, X, row_loss, st)
    switch (KT) {
        case 1: TKR_ALS_SOLVE(1);
        case 2: TKR_ALS_SOLVE(2);
        case 3: TKR_ALS_SOLVE(3);
        default: TKR_ALS_SOLVE(4);
    }
#undef TKR_ALS_SOLVE
}

// what tkr_als_gram and tkr_als_gram_wide share: the checks, the status word, the slab sums -- launch_slabs(stream, n_slabs, n_listed,
// partial, st), the one thing that differs, with the bound on k and the floats between two partials -- and the reduce.
template <typename Launch>
static int als_gram(const float* Y, int32_t n, int32_t k, int32_t k_max, int64_t stride, const int32_t* rows, int64_t n_listed, double scale,
                    double ridge, float* G, void* workspace, int64_t workspace_bytes, int64_t* status, void* stream_, Launch launch_slabs) {
    if (!Y || !G || !status || ((uintptr_t)status & 7) || ((uintptr_t)workspace & 7)) return TKR_EINVAL;
    if (n < 1 || n_listed < 0 || workspace_bytes < 0 || !std::isfinite(scale) || !std::isfinite(ridge)) return TKR_EINVAL;
    TKR_CHECK_RC(als_check_k(k, k_max));
    if (!rows) n_listed = n;
    const long long n_slabs = (n_listed + kAlsSlab - 1) / kAlsSlab;
    if (n_slabs > (long long)INT_MAX) return TKR_EUNSUPPORTED;
    if (n_slabs > 0 && (!workspace || workspace_bytes < n_slabs * stride * 4)) return TKR_EINVAL;
    hipStream_t stream = (hipStream_t)stream_;
    unsigned long long* st = reinterpret_cast<unsigned long long*>(status);
    TKR_CHECK(hipMemsetAsync(st, 0xff, sizeof(unsigned long long), stream));          // -1: nothing refused
    float* partial = reinterpret_cast<float*>(workspace);
    if (n_slabs > 0) TKR_CHECK_RC(launch_slabs(stream, n_slabs, (long long)n_listed, partial, st));
    hipLaunchKernelGGL(als_gram_reduce_kernel, dim3((k * k + kAlsBlock - 1) / kAlsBlock), dim3(kAlsBlock), 0, stream, partial, n_slabs,
                       (size_t)stride, k, scale, ridge, G);
    TKR_LAUNCH_CHECK();
    return TKR_OK;
}

}  // namespace tkr

extern "C" int64_t tkr_als_workspace_bytes(int64_t n_x, int32_t k, int64_t n_slabs) {
    if (n_x < 0 || n_slabs < 0 || tkr::als_check_k(k, TKR_ALS_MAX_K) != TKR_OK) return TKR_EINVAL;
    return tkr::als_align(n_x * 4) + tkr::als_align(n_slabs * 4) + tkr::als_align(n_slabs * tkr::als_partial_stride(k) * 4);
}

extern "C" int tkr_als_gram(const float* Y, int32_t n, int32_t k, const int32_t* rows, int64_t n_listed, double scale, double ridge, float* G,
                            void* workspace, int64_t workspace_bytes, int64_t* status, void* stream_) {
    return tkr::als_gram(Y, n, k, TKR_ALS_MAX_K, tkr::als_partial_stride(k), rows, n_listed, scale, ridge, G, workspace, workspace_bytes, status, stream_,
                         [&](hipStream_t stream, long long n_slabs, long long listed, float* partial, unsigned long long* st) {
                             return tkr::launch_slabs_kt((k + 31) / 32, stream, n_slabs, Y, n, k, rows, listed, nullptr, nullptr, nullptr, partial, st);
                         });
}

extern "C" int64_t tkr_als_gram_wide_workspace_bytes(int32_t k, int64_t n_slabs) {
    if (n_slabs < 0) return TKR_EINVAL;
    const int rc = tkr::als_check_k(k, TKR_ALS_CG_MAX_K);
    if (rc != TKR_OK) return rc;
    return tkr::als_align(n_slabs * (int64_t)k * k * 4);
}

extern "C" int tkr_als_gram_wide(const float* Y, int32_t n, int32_t k, const int32_t* rows, int64_t n_listed, double scale, double ridge, float* G,
                                 void* workspace, int64_t workspace_bytes, int64_t* status, void* stream_) {
    return tkr::als_gram(Y, n, k, TKR_ALS_CG_MAX_K, (int64_t)k * k, rows, n_listed, scale, ridge, G, workspace, workspace_bytes, status, stream_,
                         [&](hipStream_t stream, long long n_slabs, long long listed, float* partial, unsigned long long* st) {
                             const int KT = (k + 31) / 32;
                             const size_t lds = (size_t)(tkr::kAlsTile * tkr::als_stage_pitch(KT) + tkr::kAlsTile) * 4;
                             const int passes = (tkr::als_tiles(KT) + tkr::kWidePass - 1) / tkr::kWidePass;
                             if (lds > 64 * 1024)
                                 TKR_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(tkr::als_wide_slab_kernel),
                                                               hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
                             hipLaunchKernelGGL(tkr::als_wide_slab_kernel, dim3((unsigned)n_slabs, (unsigned)passes), dim3(tkr::kAlsBlock), lds, stream, Y,
                                                n, k, rows, listed, partial, st);
                             TKR_LAUNCH_CHECK();
                             return (int)TKR_OK;
                         });
}

extern "C" int tkr_als_solve_rows(const float* Y, int32_t n_y, int32_t k, const float* G, const int64_t* like_ptr, const int32_t* like_cols,
                                  int64_t n_likes, int64_t n_x, double w_like, double w_rhs, double ridge, int64_t heavy_from, float* X,
                                  double* row_loss, void* workspace, int64_t workspace_bytes, int64_t* status, void* stream_) {
    return tkr::als_solve(Y, n_y, k, G, like_ptr, like_cols, n_likes, n_x, w_like, w_rhs, ridge, heavy_from, X, row_loss, workspace, workspace_bytes,
                          status, stream_, nullptr, 0.0);
}

extern "C" int64_t tkr_als_prior_workspace_bytes(int64_t n_x, int32_t k, int64_t n_slabs) {
    const int64_t base = tkr_als_workspace_bytes(n_x, k, n_slabs);
    return base < 0 ? base : base + tkr::als_align(tkr::als_factor_floats(k) * 4);
}

extern "C" int tkr_als_solve_rows_prior(const float* Y, int32_t n_y, int32_t k, const float* G, const int64_t* like_ptr, const int32_t* like_cols,
                                        int64_t n_likes, int64_t n_x, double w_like, double w_rhs, double ridge, int64_t heavy_from, float* X,
                                        double* row_loss, const float* prior, double w_prior, void* workspace, int64_t workspace_bytes,
                                        int64_t* status, void* stream_) {
    if (!prior || ((uintptr_t)prior & 3) || !std::isfinite(w_prior) || w_prior < 0.0) return TKR_EINVAL;
    return tkr::als_solve(Y, n_y, k, G, like_ptr, like_cols, n_likes, n_x, w_like, w_rhs, ridge, heavy_from, X, row_loss, workspace, workspace_bytes,
                          status, stream_, prior, w_prior);
}
