// K24 -- the ALS half-step by conjugate gradients (tkr_als_cg_rows): the second, opt-in solver of top-k-rec_amd/als.py.  Conjugate
// gradients only: the shared Gram at any width up to 512 (tkr_als_gram_wide) is csrc/als.hip's, beside K20's, and what both files use
// (the MFMA vector type, the stage pitch, als_ptr_ok, the check of k) is csrc/als_parts.h.
//
// The per-row matrix A_r = G + w_like * sum_{y in L_r} y y^T + ridge I is never formed.  A row takes `steps` steps of conjugate gradients
// from the value X[r] holds (Takacs, Pilaszy, Tikk 2011); a step needs q = A_r p, that is  p G  (shared by every row) and
// sum_y (y . p) y over the row's likes: O(k^2 + m k) per step where the factorisation is O(k^3 + m k^2), and a state of four vectors.
//
//   als_cg_kernel<KC>       a workgroup of 256 threads owns a tile of 32 consecutive rows of X; KC = the floats of a row a lane holds
//                           (lane l: the elements l, l + 64, ..), instantiated at 1, 2, 4, 8 (k <= 64 / 128 / 256 / 512).
//     cg_pg                 Q = P G for the tile on the exact-fp32 MFMA (v_mfma_f32_32x32x2_f32): G comes through LDS in panels of 8
//                           rows, so G is read once per 32 rows of X; wave w takes the 32-column blocks w, w + 4, ..  Every element of Q
//                           is ONE fp32 fma chain over j = 0 .. k - 1 from +0.0.  P and Q are [32][PP] floats in LDS, PP = the smallest
//                           pitch >= k that is 2 mod 64: the A operand of the MFMA is P[lane & 31][j + (lane >> 5)], 32 rows x 2
//                           adjacent columns, bank 2 (lane & 31) + (lane >> 5): 64 different banks.  (PP > k where k is odd; the
//                           column k is kept zero and pairs with a zero row of the panel.)  The panel's pitch is 32 mod 64, as
//                           als_stage_pitch: the two rows an MFMA reads start 32 banks apart.
//     cg_likes              the like part, a wave per row, the 8 rows of a wave in turn: p in registers, the rows of Y gathered whole
//                           through L2 (64 lanes x KC floats), t_y = y . p, s += t_y y as one fma chain per component in stored order;
//                           then q = fp32(Q + w_like s + ridge p), the three terms in fp64, rounded once.
//     the update            x and r stay in the registers of the wave that owns the row; p and q pass through LDS.
//                           alpha = rho / (p . q);  x = fma(alpha, p, x);  r = fma(-alpha, q, r);  rho' = r . r;  p = fma(rho' / rho, p, r)
//   Every dot product is ONE fixed tree: a lane's partial is an fma chain from +0.0 over its elements in ascending order, then
//   s += s(lane ^ 32), ^ 16, .. ^ 1.  Divisions are IEEE fp32 divisions.  The file is compiled with `#pragma clang fp contract(off)`:
//   every fused multiply-add is written as fmaf / the MFMA, everything else rounds on its own, so that tests/_cg_oracle.py can restate
//   the order operation by operation.
//   Every barrier is in workgroup-uniform control flow: the loops run over k and `steps`; a row that is done (rho < 1e-20), refused or
//   past n_x is frozen by its state word, which only the branches WITHOUT barriers read.  The bits of a row depend on G, the weights,
//   its own likes in stored order, its own X[r] and prior, and `steps`: its place in the tile picks a wave and a row of P, not an order.
// No float atomics; the only atomic is the status word's minimum.  Nothing refused is used as an index.
#include "als_parts.h"

#include <math.h>

#pragma clang fp contract(off)

namespace tkr {

constexpr int kCgBlock = 256;
constexpr int kCgWaves = kCgBlock / TKR_WAVE;
constexpr int kCgTile = 32;                                       // rows of X per workgroup = the MFMA's block edge
constexpr int kCgRows = kCgTile / kCgWaves;                       // rows a wave owns
constexpr int kCgPanel = 8;                                       // rows of G in LDS at a time
constexpr float kCgDone = 1e-20f;                                 // rho below this: the row is done

enum { kCgActive = 0, kCgFrozen = 1, kCgSkip = 2, kCgRefused = 3 };   // a row's state: 0, 1 are stored and have a loss; 2, 3 are untouched, loss 0
enum { kCgFirst = 0, kCgStep = 1, kCgLoss = 2 };

// floats between two rows of P / Q: the smallest pitch >= k that is 2 mod 64
__host__ __device__ inline int cg_p_pitch(int k) { return (k + 61) / 64 * 64 + 2; }
// (the panel of G has the Gram's stage pitch, als_stage_pitch)

// dynamic LDS of als_cg_kernel, in floats from the start (every piece an even number of floats)
struct CgLds {
    int p, q, g, lo, m, c, state, floats;
    __host__ __device__ CgLds(int k) {
        const int PP = cg_p_pitch(k), GP = als_stage_pitch((k + 31) / 32);
        p = 0;
        q = p + kCgTile * PP;
        g = q + kCgTile * PP;
        lo = g + kCgPanel * GP;                                   // 32 long long
        m = lo + 2 * kCgTile;
        c = m + kCgTile;
        state = c + kCgTile;
        floats = state + kCgTile;
    }
};

// the one dot product of this file: every lane returns the same bits
template <int KC>
__device__ __forceinline__ float cg_dot(const float (&a)[KC], const float (&b)[KC]) {
    float s = 0.f;
#pragma unroll
    for (int c = 0; c < KC; ++c) s = fmaf(a[c], b[c], s);
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) s = s + __shfl_xor(s, d);
    return s;
}

__device__ __forceinline__ double cg_tree(double s) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) s = s + __shfl_xor(s, d);
    return s;
}

// Q[row][col] = sum_j P[row][j] G[j][col], one fma chain over j ascending.  Called by the whole workgroup; starts and ends with a barrier.
template <int NBW>
__device__ __forceinline__ void cg_pg(const float* __restrict__ G, int k, int KT, const float* P, float* Q, float* Gs, int PP, int GP) {
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, l31 = lane & 31, h = lane >> 5;
    const int cols = KT * 32;
    als_f32x16 acc[NBW];
#pragma unroll
    for (int s = 0; s < NBW; ++s)
#pragma unroll
        for (int reg = 0; reg < 16; ++reg) acc[s][reg] = 0.f;
    for (int j0 = 0; j0 < k; j0 += kCgPanel) {                    // workgroup-uniform
        __syncthreads();                                          // P is complete / the panel before this one is done with
        for (int idx = tid; idx < kCgPanel * cols; idx += kCgBlock) {
            const int jr = idx / cols, col = idx - jr * cols, j = j0 + jr;
            Gs[jr * GP + col] = (j < k && col < k) ? G[(size_t)j * k + col] : 0.f;
        }
        __syncthreads();
        const int left = (k - j0 + 1) & ~1;                       // j0 + t + h <= k: the column k of P (k odd) is zero, < PP
        const int tn = left < kCgPanel ? left : kCgPanel;
        for (int t = 0; t < tn; t += 2) {
            const float a = P[l31 * PP + j0 + t + h];
#pragma unroll
            for (int s = 0; s < NBW; ++s) {
                const int nb = wave + kCgWaves * s;
                if (nb < KT) acc[s] = __builtin_amdgcn_mfma_f32_32x32x2f32(a, Gs[(t + h) * GP + nb * 32 + l31], acc[s], 0, 0, 0);      // (wave-uniform)
            }
        }
    }
#pragma unroll
    for (int s = 0; s < NBW; ++s) {
        const int nb = wave + kCgWaves * s, col = nb * 32 + l31;
        if (nb < KT && col < k) {
#pragma unroll
            for (int reg = 0; reg < 16; ++reg) Q[((reg & 3) + 8 * (reg >> 2) + 4 * h) * PP + col] = acc[s][reg];
        }
    }
    __syncthreads();
}

// the like part of one product for the 8 rows of this wave, v = the row of P:  s = sum_y (y . v) y,  then
//   kCgFirst  Q <- r = b - fp32(Q + w_like s + ridge v),  b = fp32(w_rhs sum y + w_prior prior);  counts the row's likes inside the table
//   kCgStep   Q <- fp32(Q + w_like s + ridge v)
//   kCgLoss   row_loss <- 1/2 v . fp32(Q + w_like s) - w_rhs sum_y t_y + 1/2 w_rhs c (+ 1/2 w_prior |v - prior|^2), sums in fp64
// No barrier inside.
template <int KC, int MODE>
__device__ __forceinline__ void cg_likes(const float* __restrict__ Y, int n_y, int k, const int32_t* __restrict__ like_cols,
                                         const float* __restrict__ prior, double w_like, double w_rhs, double w_prior, double ridge,
                                         long long row0, const float* P, float* Q, int PP, const long long* lo_s, const int* m_s, int* c_s,
                                         int* state_s, double* __restrict__ row_loss, unsigned long long* __restrict__ status) {
    constexpr int U = KC >= 8 ? 4 : (KC == 4 ? 8 : 32 / KC);       // rows of Y gathered at a time: 32 registers of them (16 at k > 256)
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    for (int i = 0; i < kCgRows; ++i) {
        const int lr = wave * kCgRows + i;
        const int state = __builtin_amdgcn_readfirstlane(state_s[lr]);
        if (MODE == kCgStep ? state != kCgActive : state >= kCgSkip) continue;       // (wave-uniform)
        const long long row = row0 + lr;
        const long long lo = lo_s[lr];
        const int m = __builtin_amdgcn_readfirstlane(m_s[lr]);
        float v[KC], s[KC];
        double cs[KC];
#pragma unroll
        for (int c = 0; c < KC; ++c) {
            const int col = lane + 64 * c;
            v[c] = col < k ? P[lr * PP + col] : 0.f;
            s[c] = 0.f;
            cs[c] = 0.0;
        }
        double lin = 0.0;
        int n_valid = 0;
        for (int base = 0; base < m; base += TKR_WAVE) {
            int mine = -1;
            if (base + lane < m) {
                mine = like_cols[lo + base + lane];
                if ((uint32_t)mine >= (uint32_t)n_y) {
                    if (MODE == kCgFirst) status_refuse(status, row, kAlsSkipped);
                    mine = -1;
                }
            }
            const int ne = m - base < TKR_WAVE ? m - base : TKR_WAVE;
            for (int e0 = 0; e0 < ne; e0 += U) {                  // U rows of Y in flight; the chains below still take them one by one
                int ys[U];
                float yv[U][KC], t[U];
#pragma unroll
                for (int u = 0; u < U; ++u) {
                    const int y = __builtin_amdgcn_readlane(mine, (e0 + u) & (TKR_WAVE - 1));
                    ys[u] = e0 + u < ne ? y : -1;
#pragma unroll
                    for (int c = 0; c < KC; ++c) {
                        const int col = lane + 64 * c;
                        yv[u][c] = (ys[u] >= 0 && col < k) ? Y[(size_t)ys[u] * k + col] : 0.f;
                    }
                }
#pragma unroll
                for (int u = 0; u < U; ++u) t[u] = cg_dot<KC>(yv[u], v);
#pragma unroll
                for (int u = 0; u < U; ++u) {
                    if (ys[u] < 0) continue;                      // (wave-uniform) refused, or past the row's end
#pragma unroll
                    for (int c = 0; c < KC; ++c) {
                        s[c] = fmaf(t[u], yv[u][c], s[c]);
                        if (MODE == kCgFirst) cs[c] = cs[c] + (double)yv[u][c];
                    }
                    if (MODE == kCgLoss) lin = lin + (double)t[u];
                    ++n_valid;
                }
            }
        }
        if (MODE == kCgFirst) {
            if (lane == 0) c_s[lr] = n_valid;
            if (n_valid == 0 && !(prior && m == 0)) {             // no like inside the table: untouched (with a prior: K21's rule)
                if (lane == 0) state_s[lr] = kCgSkip;
                continue;
            }
        }
        double quad = 0.0, dist = 0.0;
#pragma unroll
        for (int c = 0; c < KC; ++c) {
            const int col = lane + 64 * c;
            if (col < k) {
                const double gq = (double)Q[lr * PP + col];
                const float pv = prior ? prior[(size_t)row * k + col] : 0.f;
                if (MODE == kCgLoss) {
                    const float q = (float)(gq + w_like * (double)s[c]);
                    if (m > 0) quad = quad + (double)v[c] * (double)q;
                    const double d = (double)v[c] - (double)pv;
                    dist = dist + d * d;
                } else {
                    const float q = (float)((gq + w_like * (double)s[c]) + ridge * (double)v[c]);
                    if (MODE == kCgFirst) {
                        const float b = prior ? (float)(w_rhs * cs[c] + w_prior * (double)pv) : (float)(w_rhs * cs[c]);
                        Q[lr * PP + col] = b - q;
                    } else {
                        Q[lr * PP + col] = q;
                    }
                }
            }
        }
        if (MODE == kCgLoss) {
            quad = cg_tree(quad);
            dist = cg_tree(dist);
            double loss = m > 0 ? (0.5 * quad - w_rhs * lin) + 0.5 * w_rhs * (double)c_s[lr] : 0.0;
            if (prior) loss = loss + 0.5 * w_prior * dist;
            if (lane == 0) row_loss[row] = loss;
        }
    }
}

template <int KC>
__global__ __launch_bounds__(kCgBlock) void als_cg_kernel(const float* __restrict__ Y, int n_y, int k, const float* __restrict__ G,
                                                          const int64_t* __restrict__ like_ptr, const int32_t* __restrict__ like_cols,
                                                          long long n_likes, long long n_x, double w_like, double w_rhs, double ridge, int steps,
                                                          float* __restrict__ X, double* __restrict__ row_loss, const float* __restrict__ prior,
                                                          double w_prior, unsigned long long* __restrict__ status) {
    constexpr int NBW = KC >= 2 ? KC / 2 : 1;                     // 32-column blocks of Q per wave: ceil(ceil(k / 32) / 4)
    extern __shared__ __attribute__((aligned(16))) float cg_lds[];
    const CgLds at(k);
    const int KT = (k + 31) / 32, PP = cg_p_pitch(k), GP = als_stage_pitch(KT);
    float* P = cg_lds + at.p;
    float* Q = cg_lds + at.q;
    float* Gs = cg_lds + at.g;
    long long* lo_s = reinterpret_cast<long long*>(cg_lds + at.lo);
    int* m_s = reinterpret_cast<int*>(cg_lds + at.m);
    int* c_s = reinterpret_cast<int*>(cg_lds + at.c);
    int* state_s = reinterpret_cast<int*>(cg_lds + at.state);
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const long long row0 = (long long)blockIdx.x * kCgTile;

    if (tid < kCgTile) {                                          // the rows' likes and states
        const long long row = row0 + tid;
        long long lo = 0;
        int m = 0, state = kCgSkip;
        if (row < n_x) {
            const long long a = like_ptr[row], b = like_ptr[row + 1];
            if (!als_ptr_ok(a, b, n_likes, row)) {
                status_refuse(status, row, kAlsBadPtr);            // the row is left as it is
                state = kCgRefused;
            } else {
                lo = a;
                m = (int)(b - a);
                state = (m == 0 && !prior) ? kCgSkip : kCgActive;
            }
        }
        lo_s[tid] = lo;
        m_s[tid] = m;
        c_s[tid] = 0;
        state_s[tid] = state;
        for (int col = k; col < PP; ++col) P[tid * PP + col] = 0.f;            // the columns the MFMA may read beyond k
    }
    __syncthreads();

    float x[kCgRows][KC], r[kCgRows][KC], rho[kCgRows];
#pragma unroll
    for (int i = 0; i < kCgRows; ++i) {
        const int lr = wave * kCgRows + i;
        const bool live = state_s[lr] == kCgActive;
#pragma unroll
        for (int c = 0; c < KC; ++c) {
            const int col = lane + 64 * c;
            x[i][c] = (live && col < k) ? X[(size_t)(row0 + lr) * k + col] : 0.f;
            r[i][c] = 0.f;
            if (col < k) P[lr * PP + col] = x[i][c];
        }
        rho[i] = 0.f;
    }

    // r = b - A x;  p = r;  rho = r . r
    cg_pg<NBW>(G, k, KT, P, Q, Gs, PP, GP);
    cg_likes<KC, kCgFirst>(Y, n_y, k, like_cols, prior, w_like, w_rhs, w_prior, ridge, row0, P, Q, PP, lo_s, m_s, c_s, state_s, row_loss, status);
#pragma unroll
    for (int i = 0; i < kCgRows; ++i) {
        const int lr = wave * kCgRows + i;
        if (__builtin_amdgcn_readfirstlane(state_s[lr]) == kCgActive) {       // (wave-uniform, no barrier inside)
#pragma unroll
            for (int c = 0; c < KC; ++c) {
                const int col = lane + 64 * c;
                r[i][c] = col < k ? Q[lr * PP + col] : 0.f;
                if (col < k) P[lr * PP + col] = r[i][c];
            }
            rho[i] = cg_dot<KC>(r[i], r[i]);
            if (rho[i] < kCgDone && lane == 0) state_s[lr] = kCgFrozen;
        }
    }

    for (int step = 0; step < steps; ++step) {                    // workgroup-uniform
        cg_pg<NBW>(G, k, KT, P, Q, Gs, PP, GP);
        cg_likes<KC, kCgStep>(Y, n_y, k, like_cols, prior, w_like, w_rhs, w_prior, ridge, row0, P, Q, PP, lo_s, m_s, c_s, state_s, row_loss, status);
#pragma unroll
        for (int i = 0; i < kCgRows; ++i) {
            const int lr = wave * kCgRows + i;
            if (__builtin_amdgcn_readfirstlane(state_s[lr]) != kCgActive) continue;      // frozen: nothing of the row moves
            float p[KC], q[KC];
#pragma unroll
            for (int c = 0; c < KC; ++c) {
                const int col = lane + 64 * c;
                p[c] = col < k ? P[lr * PP + col] : 0.f;
                q[c] = col < k ? Q[lr * PP + col] : 0.f;
            }
            const float pq = cg_dot<KC>(p, q);
            if (!(pq > 0.f) || !(pq < INFINITY)) {                // not positive definite (or not finite) along p
                if (lane == 0) {
                    status_refuse(status, row0 + lr, kAlsNotSolved);
                    state_s[lr] = kCgRefused;
                }
                continue;
            }
            const float alpha = rho[i] / pq;
#pragma unroll
            for (int c = 0; c < KC; ++c) {
                x[i][c] = fmaf(alpha, p[c], x[i][c]);
                r[i][c] = fmaf(-alpha, q[c], r[i][c]);
            }
            const float rho2 = cg_dot<KC>(r[i], r[i]);
            const float beta = rho2 / rho[i];
#pragma unroll
            for (int c = 0; c < KC; ++c) {
                const int col = lane + 64 * c;
                if (col < k) P[lr * PP + col] = fmaf(beta, p[c], r[i][c]);
            }
            rho[i] = rho2;
            if (rho2 < kCgDone && lane == 0) state_s[lr] = kCgFrozen;
        }
    }

#pragma unroll
    for (int i = 0; i < kCgRows; ++i) {                           // a solution that is not finite is not stored
        const int lr = wave * kCgRows + i;
        if (__builtin_amdgcn_readfirstlane(state_s[lr]) >= kCgSkip) continue;
        bool finite = true;
#pragma unroll
        for (int c = 0; c < KC; ++c) finite = finite && fabsf(x[i][c]) < INFINITY;       // (false for a NaN)
        if (__ballot(!finite) != 0ull && lane == 0) {
            status_refuse(status, row0 + lr, kAlsNotSolved);
            state_s[lr] = kCgRefused;
        }
    }

    if (row_loss) {                                               // (uniform) ONE fresh product with the final x
#pragma unroll
        for (int i = 0; i < kCgRows; ++i) {
            const int lr = wave * kCgRows + i;
            const bool ok = __builtin_amdgcn_readfirstlane(state_s[lr]) < kCgSkip;
#pragma unroll
            for (int c = 0; c < KC; ++c) {
                const int col = lane + 64 * c;
                if (col < k) P[lr * PP + col] = ok ? x[i][c] : 0.f;
            }
            if (!ok && lane == 0 && row0 + lr < n_x) row_loss[row0 + lr] = 0.0;
        }
        cg_pg<NBW>(G, k, KT, P, Q, Gs, PP, GP);
        cg_likes<KC, kCgLoss>(Y, n_y, k, like_cols, prior, w_like, w_rhs, w_prior, ridge, row0, P, Q, PP, lo_s, m_s, c_s, state_s, row_loss, status);
    }
    if (steps > 0) {
#pragma unroll
        for (int i = 0; i < kCgRows; ++i) {
            const int lr = wave * kCgRows + i;
            if (__builtin_amdgcn_readfirstlane(state_s[lr]) >= kCgSkip) continue;
#pragma unroll
            for (int c = 0; c < KC; ++c) {
                const int col = lane + 64 * c;
                if (col < k) X[(size_t)(row0 + lr) * k + col] = x[i][c];
            }
        }
    }
}

template <int KC>
static int launch_cg(hipStream_t stream, const float* Y, int n_y, int k, const float* G, const int64_t* like_ptr, const int32_t* like_cols,
                     long long n_likes, long long n_x, double w_like, double w_rhs, double ridge, int steps, float* X, double* row_loss,
                     const float* prior, double w_prior, unsigned long long* st) {
    const size_t lds = (size_t)CgLds(k).floats * 4;
    auto kern = als_cg_kernel<KC>;
    if (lds > 64 * 1024) TKR_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    hipLaunchKernelGGL(kern, dim3((unsigned)((n_x + kCgTile - 1) / kCgTile)), dim3(kCgBlock), lds, stream, Y, n_y, k, G, like_ptr, like_cols, n_likes,
                       n_x, w_like, w_rhs, ridge, steps, X, row_loss, prior, w_prior, st);
    TKR_LAUNCH_CHECK();
    return TKR_OK;
}

}  // namespace tkr

extern "C" int64_t tkr_als_cg_workspace_bytes(int64_t n_x, int32_t k) {
    if (n_x < 0) return TKR_EINVAL;
    const int rc = tkr::als_check_k(k, TKR_ALS_CG_MAX_K);
    return rc != TKR_OK ? rc : 0;                                 // the state of a row is registers and LDS
}

extern "C" int tkr_als_cg_rows(const float* Y, int32_t n_y, int32_t k, const float* G, const int64_t* like_ptr, const int32_t* like_cols,
                               int64_t n_likes, int64_t n_x, double w_like, double w_rhs, double ridge, int32_t steps, float* X, double* row_loss,
                               const float* prior, double w_prior, void* workspace, int64_t workspace_bytes, int64_t* status, void* stream_) {
    if (!Y || !G || !like_ptr || !X || !status) return TKR_EINVAL;
    if (((uintptr_t)Y & 3) || ((uintptr_t)G & 3) || ((uintptr_t)X & 3) || ((uintptr_t)prior & 3) || ((uintptr_t)like_ptr & 7) ||
        ((uintptr_t)like_cols & 3) || ((uintptr_t)status & 7) || ((uintptr_t)row_loss & 7) || ((uintptr_t)workspace & 15))
        return TKR_EINVAL;
    if (n_likes < 0 || (n_likes > 0 && !like_cols) || n_y < 1 || n_x < 1 || n_x > (int64_t)INT_MAX || steps < 0 || workspace_bytes < 0)
        return TKR_EINVAL;
    if (!std::isfinite(w_like) || !std::isfinite(w_rhs) || !std::isfinite(ridge) || ridge < 0.0 || !std::isfinite(w_prior) || w_prior < 0.0)
        return TKR_EINVAL;
    TKR_CHECK_RC(tkr::als_check_k(k, TKR_ALS_CG_MAX_K));
    hipStream_t stream = (hipStream_t)stream_;
    unsigned long long* st = reinterpret_cast<unsigned long long*>(status);
    TKR_CHECK(hipMemsetAsync(st, 0xff, sizeof(unsigned long long), stream));          // -1: nothing refused
#define TKR_CG_LAUNCH(KC) \
    return tkr::launch_cg<KC>(stream, Y, n_y, k, G, like_ptr, like_cols, (long long)n_likes, (long long)n_x, w_like, w_rhs, ridge, steps, X, row_loss, prior, w_prior, st)
    if (k <= 64) TKR_CG_LAUNCH(1);
    if (k <= 128) TKR_CG_LAUNCH(2);
    if (k <= 256) TKR_CG_LAUNCH(4);
    TKR_CG_LAUNCH(8);
#undef TKR_CG_LAUNCH
}
