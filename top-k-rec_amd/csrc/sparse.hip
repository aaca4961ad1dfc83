// K26 -- a sparse x dense product (tkr_csr_spmm) and CER's E-step by conjugate gradients on top of it (tkr_estep_cg): the opt-in
// estep='cg' of top-k-rec_amd/als.py.  The content features F [n_items, d] stay a CSR; nothing of size d x d or n_items x d exists.
//
//   out[r] = fp32(alpha * sum_e val[e] * X[col[e]] + beta * Z[r])                       tkr_csr_spmm
//   (lv F^T F + le I) E = lv F^T V, `steps` steps of conjugate gradients from the E given, all k columns in step    tkr_estep_cg
//
//   spmm_kernel<G, KC>        a row is owned by a GROUP of G lanes (8, 16, 32 or 64), lane g of the group holds the components
//                             g, g + G, .. (KC of them): k <= 8 puts 8 rows on a wave, k <= 16 four, k <= 32 two, wider rows take a
//                             whole wave and 1, 2, 4 or 8 registers per lane.  The group reads G (col, val) pairs at a time, one per
//                             lane, and hands them round by a lane permute; the rows of X they name are gathered U at a time (U * KC
//                             <= 32 registers in flight) and THEN chained: s_c = fma(val[e], X[col[e]][c], s_c) from +0.0 in stored
//                             order, whatever U and G are.  A row with more than heavy_from nonzeros is put on a list instead.
//   spmm_heavy_kernel<G, KC>  one workgroup of 1024 threads (1024 / G groups) per listed row.  The row is cut into slabs of
//                             TKR_SPMM_SLAB nonzeros in stored order; a group sums a slab as the chain above; the slab sums pass through
//                             LDS and thread c adds them for component c in ASCENDING slab order in fp64.  Rounded once.
//   sp_chain<G, KC>           the one chain of this file, called by whole waves: both kernels above are this function.
//   es_*                      the vector part of the recurrence on [d, k] tables, a workgroup of 64 x 16 threads per slab of
//                             TKR_ESTEP_SLAB rows and block of 64 columns: thread (c, j) walks the rows 64 j .. 64 j + 63 of the slab
//                             for column c -- an fma chain from +0.0 for a dot product -- and the 16 run sums of a column are added in
//                             ascending order in fp32: that is a slab's partial.  es_alpha (one workgroup) adds the partials of a column
//                             in ascending slab order in fp64, rounds once, and forms alpha; es_p does the same for beta.
// The file is compiled with `#pragma clang fp contract(off)`: every fused multiply-add is written as fmaf, everything else rounds on its
// own, so that tests/_estep_oracle.py can restate the order operation by operation.
// No float atomics; the atomics are the status word's minimum and the integer counter of the heavy list, whose order changes no result.
// Nothing refused is used as an index.  Every barrier is in workgroup-uniform control flow.
#include "als_parts.h"

#include <math.h>

#include <algorithm>

#pragma clang fp contract(off)

namespace tkr {

constexpr int kSpBlock = 256;
constexpr int kSpHeavyBlock = 1024;
constexpr int kSpSlab = TKR_SPMM_SLAB;
constexpr int kEsSlab = TKR_ESTEP_SLAB, kEsRuns = 16, kEsRun = kEsSlab / kEsRuns, kEsCols = 64;
constexpr float kEsDone = 1e-20f;                                 // rho below this: the column is done
static_assert(kEsRun == 64 && kSpSlab % 64 == 0, "a run is 64 rows; a slab of nonzeros is whole reads of every group width");

// the kinds of K26: a column index outside [0, n_cols); a value that is not finite; p . q of a column not positive and finite;
// ptr wrong at the row
enum { kSpBadCol = 0, kSpNotFinite = 1, kSpNotSolved = 2, kSpBadPtr = 3 };
enum { kSpFlagCol = 1, kSpFlagVal = 2 };

__device__ __forceinline__ bool sp_finite(float v) { return fabsf(v) < INFINITY; }       // (false for a NaN)

// s_c = the chain over the nonzeros [first, first + count) of THIS GROUP's row, components c = g + G * 0 .. g + G * (KC - 1).
// Called by every lane of a wave (count may be 0); -> the flags of what the group met, the same in each of its lanes.
template <int G, int KC>
__device__ __forceinline__ int sp_chain(const int32_t* __restrict__ col, const float* __restrict__ val, const float* __restrict__ X, int n_cols,
                                        int k, long long first, int count, float (&s)[KC]) {
    constexpr int U = KC >= 8 ? 4 : (KC == 4 || G < 16 ? 8 : 16);  // rows of X gathered at a time: up to 32 registers of them
    static_assert(G % U == 0, "a read of G pairs is whole gathers");
    const int lane = threadIdx.x & 63, g = lane & (G - 1);
#pragma unroll
    for (int c = 0; c < KC; ++c) s[c] = 0.f;
    int most = count;                                             // the longest count among the wave's groups
    if (G < 64) {
#pragma unroll
        for (int d = 32; d >= G; d >>= 1) most = max(most, __shfl_xor(most, d));
    }
    int flags = 0;
    for (int base = 0; base < most; base += G) {                  // wave-uniform
        int mine_c = -1;
        float mine_v = 0.f;
        if (base + g < count) {
            mine_c = col[first + base + g];
            mine_v = val[first + base + g];
            if ((uint32_t)mine_c >= (uint32_t)n_cols) {
                flags |= kSpFlagCol;
                mine_c = -1;                                      // never an index
            }
            if (!sp_finite(mine_v)) flags |= kSpFlagVal;
        }
        const int n_here = min(G, most - base);
        for (int e0 = 0; e0 < n_here; e0 += U) {                  // U gathers in flight; the chain below still takes them one by one
            int cs[U];
            float vs[U], xv[U][KC];
#pragma unroll
            for (int u = 0; u < U; ++u) {
                if (G == 64) {
                    cs[u] = __builtin_amdgcn_readlane(mine_c, e0 + u);
                    vs[u] = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(mine_v), e0 + u));
                } else {
                    cs[u] = __shfl(mine_c, e0 + u, G);
                    vs[u] = __shfl(mine_v, e0 + u, G);
                }
#pragma unroll
                for (int c = 0; c < KC; ++c) {
                    const int comp = g + G * c;
                    xv[u][c] = (cs[u] >= 0 && comp < k) ? X[(size_t)cs[u] * k + comp] : 0.f;
                }
            }
#pragma unroll
            for (int u = 0; u < U; ++u) {
#pragma unroll
                for (int c = 0; c < KC; ++c) s[c] = cs[u] >= 0 ? fmaf(vs[u], xv[u][c], s[c]) : s[c];
            }
        }
    }
    const unsigned long long met_c = __ballot(flags & kSpFlagCol), met_v = __ballot(flags & kSpFlagVal);
    const unsigned long long mine = (G == 64 ? ~0ull : ((1ull << G) - 1ull) << (lane & ~(G - 1)));
    return ((met_c & mine) ? kSpFlagCol : 0) | ((met_v & mine) ? kSpFlagVal : 0);
}

__device__ __forceinline__ void sp_refuse(unsigned long long* status, long long where, int flags) {
    if (flags & kSpFlagCol) status_refuse(status, where, kSpBadCol);
    if (flags & kSpFlagVal) status_refuse(status, where, kSpNotFinite);
}

__device__ __forceinline__ float sp_round(double alpha, double s, double beta, const float* Z, size_t at) {
    return Z ? (float)(alpha * s + beta * (double)Z[at]) : (float)(alpha * s);
}

template <int G, int KC>
__global__ __launch_bounds__(kSpBlock) void spmm_kernel(const int64_t* __restrict__ ptr, const int32_t* __restrict__ col,
                                                        const float* __restrict__ val, long long nnz, long long n_rows, int n_cols,
                                                        const float* __restrict__ X, int k, double alpha, const float* __restrict__ Z, double beta,
                                                        float* __restrict__ out, long long heavy_from, long long row_base,
                                                        unsigned long long* __restrict__ status, int32_t* __restrict__ heavy_count,
                                                        int32_t* __restrict__ heavy_list) {
    constexpr int kRows = kSpBlock / G;
    const int g = threadIdx.x & (G - 1);
    const long long r = (long long)blockIdx.x * kRows + threadIdx.x / G;
    long long lo = 0;
    int count = 0;
    bool live = false;
    if (r < n_rows) {
        lo = ptr[r];
        const long long hi = ptr[r + 1];
        if (!als_ptr_ok(lo, hi, nnz, r)) {
            if (g == 0) status_refuse(status, row_base + r, kSpBadPtr);        // the row is not written
        } else if (hi - lo > heavy_from && heavy_list) {
            if (g == 0) heavy_list[atomicAdd(heavy_count, 1)] = (int32_t)r;
        } else {
            live = true;
            count = (int)(hi - lo);
        }
    }
    float s[KC];
    const int flags = sp_chain<G, KC>(col, val, X, n_cols, k, lo, count, s);   // (every lane of the wave: no exit above)
    if (!live) return;
    if (flags) {
        if (g == 0) sp_refuse(status, row_base + r, flags);                    // the row is not written
        return;
    }
#pragma unroll
    for (int c = 0; c < KC; ++c) {
        const int comp = g + G * c;
        if (comp < k) {
            const size_t at = (size_t)r * k + comp;
            out[at] = sp_round(alpha, (double)s[c], beta, Z, at);
        }
    }
}

template <int G, int KC>
__global__ __launch_bounds__(kSpHeavyBlock) void spmm_heavy_kernel(const int64_t* __restrict__ ptr, const int32_t* __restrict__ col,
                                                                   const float* __restrict__ val, int n_cols, const float* __restrict__ X, int k,
                                                                   double alpha, const float* __restrict__ Z, double beta, float* __restrict__ out,
                                                                   long long row_base, unsigned long long* __restrict__ status,
                                                                   const int32_t* __restrict__ heavy_count, const int32_t* __restrict__ heavy_list) {
    constexpr int kUnits = kSpHeavyBlock / G, GK = G * KC;
    __shared__ float part[kUnits * GK];
    if ((int)blockIdx.x >= *heavy_count) return;                  // (the same word in every thread)
    const int tid = threadIdx.x, unit = tid / G, g = tid & (G - 1);
    const long long r = heavy_list[blockIdx.x];
    const long long lo = ptr[r], hi = ptr[r + 1];                 // checked by spmm_kernel, which listed the row
    const long long n_slabs = (hi - lo + kSpSlab - 1) / kSpSlab;
    double acc = 0.0;
    int flags = 0;
    for (long long b0 = 0; b0 < n_slabs; b0 += kUnits) {          // workgroup-uniform
        const long long b = b0 + unit, first = lo + b * kSpSlab;
        const int count = b < n_slabs ? (int)min((long long)kSpSlab, hi - first) : 0;
        float s[KC];
        flags |= sp_chain<G, KC>(col, val, X, n_cols, k, first, count, s);
#pragma unroll
        for (int c = 0; c < KC; ++c) part[unit * GK + g + G * c] = s[c];
        __syncthreads();
        const int n_here = (int)min((long long)kUnits, n_slabs - b0);
        if (tid < k)
            for (int u = 0; u < n_here; ++u) acc = acc + (double)part[u * GK + tid];
        __syncthreads();
    }
    flags = (__syncthreads_or(flags & kSpFlagCol) ? kSpFlagCol : 0) | (__syncthreads_or(flags & kSpFlagVal) ? kSpFlagVal : 0);
    if (flags) {
        if (tid == 0) sp_refuse(status, row_base + r, flags);     // the row is not written
        return;
    }
    if (tid < k) {
        const size_t at = (size_t)r * k + tid;
        out[at] = sp_round(alpha, acc, beta, Z, at);
    }
}

struct SpmmArgs {
    const int64_t* ptr;
    const int32_t* col;
    const float* val;
    long long nnz, n_rows;
    int n_cols;
};

template <int G, int KC>
static int launch_spmm(hipStream_t stream, const SpmmArgs& A, const float* X, int k, double alpha, const float* Z, double beta, float* out,
                       long long heavy_from, long long row_base, unsigned long long* st, int32_t* heavy_count, int32_t* heavy_list, long long cap) {
    constexpr int kRows = kSpBlock / G;
    hipLaunchKernelGGL((spmm_kernel<G, KC>), dim3((unsigned)((A.n_rows + kRows - 1) / kRows)), dim3(kSpBlock), 0, stream, A.ptr, A.col, A.val, A.nnz,
                       A.n_rows, A.n_cols, X, k, alpha, Z, beta, out, heavy_from, row_base, st, heavy_count, heavy_list);
    TKR_LAUNCH_CHECK();
    if (cap > 0) {
        hipLaunchKernelGGL((spmm_heavy_kernel<G, KC>), dim3((unsigned)cap), dim3(kSpHeavyBlock), 0, stream, A.ptr, A.col, A.val, A.n_cols, X, k, alpha,
                           Z, beta, out, row_base, st, heavy_count, heavy_list);
        TKR_LAUNCH_CHECK();
    }
    return TKR_OK;
}

static int64_t sp_align(int64_t bytes) { return (bytes + 15) / 16 * 16; }
static int64_t sp_list_bytes(int64_t n_rows) { return sp_align(16 + n_rows * 4); }       // the counter, then the rows

// the listed rows a product can have, at most: each has more than heavy_from nonzeros
static long long sp_cap(const SpmmArgs& A, long long heavy_from) {
    return heavy_from < A.nnz ? std::min<long long>(A.n_rows, A.nnz / (heavy_from + 1)) : 0;
}

// one product on the stream; list: sp_list_bytes(n_rows) bytes where sp_cap > 0.  The status word is the caller's to reset.
static int spmm(hipStream_t stream, const SpmmArgs& A, const float* X, int k, double alpha, const float* Z, double beta, float* out,
                long long heavy_from, long long row_base, unsigned long long* st, void* list) {
    const long long cap = sp_cap(A, heavy_from);
    int32_t* heavy_count = nullptr;
    int32_t* heavy_list = nullptr;
    if (cap > 0) {
        heavy_count = reinterpret_cast<int32_t*>(list);
        heavy_list = heavy_count + 4;
        TKR_CHECK(hipMemsetAsync(heavy_count, 0, 16, stream));
    }
#define TKR_SPMM(G, KC) return launch_spmm<G, KC>(stream, A, X, k, alpha, Z, beta, out, heavy_from, row_base, st, heavy_count, heavy_list, cap)
    if (k <= 8) TKR_SPMM(8, 1);
    if (k <= 16) TKR_SPMM(16, 1);
    if (k <= 32) TKR_SPMM(32, 1);
    if (k <= 64) TKR_SPMM(64, 1);
    if (k <= 128) TKR_SPMM(64, 2);
    if (k <= 256) TKR_SPMM(64, 4);
    TKR_SPMM(64, 8);
#undef TKR_SPMM
}

// ---- the vector part of the E-step ------------------------------------------------------------------------------------------------------
// what every es_ kernel of block (64, 16) and grid (slabs, column blocks) starts from
struct EsAt {
    int c, run;
    long long row0;                                               // the first row of this thread's run
    __device__ EsAt() : c(blockIdx.y * kEsCols + threadIdx.x), run(threadIdx.y), row0((long long)blockIdx.x * kEsSlab + (long long)threadIdx.y * kEsRun) {}
};

// the 16 run sums of a column, added in ascending order in fp32 -> the slab's partial, in the threads of run 0.  A barrier inside.
__device__ __forceinline__ float es_join(float s, float (*runs)[kEsCols]) {
    runs[threadIdx.y][threadIdx.x] = s;
    __syncthreads();
    float t = runs[0][threadIdx.x];
#pragma unroll
    for (int j = 1; j < kEsRuns; ++j) t = t + runs[j][threadIdx.x];
    return t;
}

// the partials of a column in ascending slab order in fp64, rounded once
__device__ __forceinline__ float es_total(const float* __restrict__ part, int n_slabs, int k, int c) {
    double s = 0.0;
    for (int b = 0; b < n_slabs; ++b) s = s + (double)part[(size_t)b * k + c];
    return (float)s;
}

// a value of V that is not finite: 4 * its row + 1
__global__ __launch_bounds__(256) void es_finite_kernel(const float* __restrict__ V, size_t n, int k, unsigned long long* __restrict__ status) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n && !sp_finite(V[i])) status_refuse(status, (long long)(i / k), kSpNotFinite);
}

// x = E;  r = b - w;  p = r;  the partials of r . r
__global__ __launch_bounds__(kEsCols * kEsRuns) void es_init_kernel(const float* __restrict__ E, const float* __restrict__ B, const float* __restrict__ W,
                                                                    long long d, int k, float* __restrict__ Xw, float* __restrict__ R,
                                                                    float* __restrict__ P, float* __restrict__ rr_part) {
    __shared__ float runs[kEsRuns][kEsCols];
    const EsAt at;
    float s = 0.f;
    if (at.c < k) {
#pragma unroll 8
        for (int i = 0; i < kEsRun; ++i) {
            const long long row = at.row0 + i;
            if (row < d) {
                const size_t j = (size_t)row * k + at.c;
                const float r = B[j] - W[j];
                Xw[j] = E[j];
                R[j] = r;
                P[j] = r;
                s = fmaf(r, r, s);
            }
        }
    }
    s = es_join(s, runs);
    if (at.run == 0 && at.c < k) rr_part[(size_t)blockIdx.x * k + at.c] = s;
}

// the partials of p . q
__global__ __launch_bounds__(kEsCols * kEsRuns) void es_dot_kernel(const float* __restrict__ P, const float* __restrict__ Q, long long d, int k,
                                                                   const int* __restrict__ halt, float* __restrict__ pq_part) {
    __shared__ float runs[kEsRuns][kEsCols];
    if (*halt) return;                                            // (the same word in every thread)
    const EsAt at;
    float s = 0.f;
    if (at.c < k) {
#pragma unroll 8
        for (int i = 0; i < kEsRun; ++i) {
            const long long row = at.row0 + i;
            if (row < d) {
                const size_t j = (size_t)row * k + at.c;
                s = fmaf(P[j], Q[j], s);
            }
        }
    }
    s = es_join(s, runs);
    if (at.run == 0 && at.c < k) pq_part[(size_t)blockIdx.x * k + at.c] = s;
}

// one workgroup, behind the products and the scan that read all of the input: what they refused halts the call
__global__ __launch_bounds__(TKR_ALS_CG_MAX_K) void es_begin_kernel(const unsigned long long* __restrict__ status, int k, int* __restrict__ halt,
                                                                    int* __restrict__ refused) {
    if (threadIdx.x == 0) *halt = *status != ~0ull;
    if ((int)threadIdx.x < k) refused[threadIdx.x] = 0;
}

// one workgroup, thread c: rho = r . r and p . q of column c from their partials; the column goes on where it is not refused, rho >=
// 1e-20 and p . q is positive and finite (else: refused, 4 * c + 2)
__global__ __launch_bounds__(TKR_ALS_CG_MAX_K) void es_alpha_kernel(const float* __restrict__ rr_part, const float* __restrict__ pq_part, int n_slabs, int k,
                                                                    const int* __restrict__ halt, int* __restrict__ refused, int* __restrict__ go,
                                                                    float* __restrict__ rho, float* __restrict__ alpha,
                                                                    unsigned long long* __restrict__ status) {
    const int c = threadIdx.x;
    if (*halt || c >= k) return;
    const float rh = es_total(rr_part, n_slabs, k, c), pq = es_total(pq_part, n_slabs, k, c);
    bool on = !refused[c] && rh >= kEsDone;
    if (on && !(pq > 0.f && pq < INFINITY)) {
        status_refuse(status, c, kSpNotSolved);
        refused[c] = 1;
        on = false;
    }
    go[c] = on;
    rho[c] = rh;
    alpha[c] = on ? rh / pq : 0.f;
}

// x = fma(alpha, p, x);  r = fma(-alpha, q, r);  the partials of the new r . r
__global__ __launch_bounds__(kEsCols * kEsRuns) void es_update_kernel(const float* __restrict__ P, const float* __restrict__ Q, long long d, int k,
                                                                      const int* __restrict__ halt, const int* __restrict__ go,
                                                                      const float* __restrict__ alpha, float* __restrict__ Xw, float* __restrict__ R,
                                                                      float* __restrict__ rr_part) {
    __shared__ float runs[kEsRuns][kEsCols];
    if (*halt) return;
    const EsAt at;
    const bool on = at.c < k && go[at.c];
    float s = 0.f;
    if (on) {
        const float a = alpha[at.c];
#pragma unroll 8
        for (int i = 0; i < kEsRun; ++i) {
            const long long row = at.row0 + i;
            if (row < d) {
                const size_t j = (size_t)row * k + at.c;
                Xw[j] = fmaf(a, P[j], Xw[j]);
                const float r = fmaf(-a, Q[j], R[j]);
                R[j] = r;
                s = fmaf(r, r, s);
            }
        }
    }
    s = es_join(s, runs);
    if (at.run == 0 && on) rr_part[(size_t)blockIdx.x * k + at.c] = s;       // a column that does not move keeps its rho
}

// p = fma(rho' / rho, p, r)
__global__ __launch_bounds__(kEsCols * kEsRuns) void es_p_kernel(const float* __restrict__ R, long long d, int k, const int* __restrict__ halt,
                                                                 const int* __restrict__ go, const float* __restrict__ rho,
                                                                 const float* __restrict__ rr_part, int n_slabs, float* __restrict__ P) {
    __shared__ float beta_s[kEsCols];
    if (*halt) return;
    const EsAt at;
    const bool on = at.c < k && go[at.c];
    if (at.run == 0 && on) beta_s[threadIdx.x] = es_total(rr_part, n_slabs, k, at.c) / rho[at.c];
    __syncthreads();
    if (!on) return;
    const float beta = beta_s[threadIdx.x];
#pragma unroll 8
    for (int i = 0; i < kEsRun; ++i) {
        const long long row = at.row0 + i;
        if (row < d) {
            const size_t j = (size_t)row * k + at.c;
            P[j] = fmaf(beta, P[j], R[j]);
        }
    }
}

// E = x in the columns that were not refused
__global__ __launch_bounds__(256) void es_final_kernel(const float* __restrict__ Xw, size_t n, int k, const int* __restrict__ halt,
                                                       const int* __restrict__ refused, float* __restrict__ E) {
    if (*halt) return;
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n && !refused[i % k]) E[i] = Xw[i];
}

// the workspace of tkr_estep_cg, in bytes from its start (every piece a multiple of 16)
struct EsRoom {
    int64_t list, T, B, R, P, Q, X, rr, pq, rho, alpha, go, refused, halt, bytes;
    EsRoom(int64_t n_items, int64_t d, int64_t k) {
        const int64_t table = sp_align(d * k * 4), slabs = (d + kEsSlab - 1) / kEsSlab, col = sp_align(k * 4);
        list = 0;
        T = list + sp_list_bytes(std::max(n_items, d));
        B = T + sp_align(n_items * k * 4);
        R = B + table;
        P = R + table;
        Q = P + table;
        X = Q + table;
        rr = X + table;
        pq = rr + sp_align(slabs * k * 4);
        rho = pq + sp_align(slabs * k * 4);
        alpha = rho + col;
        go = alpha + col;
        refused = go + col;
        halt = refused + col;
        bytes = halt + 16;
    }
};

// the flat launches of the E-step (a thread per element of a [rows, k] table, 256 per workgroup) fit the grid's first dimension
static bool es_flat_ok(int64_t rows, int64_t k) { return (rows * k + 255) / 256 <= (int64_t)INT_MAX; }

static bool sp_csr_args_ok(const int64_t* ptr, const int32_t* col, const float* val, int64_t nnz, int64_t n_rows, int64_t n_cols) {
    if (!ptr || ((uintptr_t)ptr & 7) || ((uintptr_t)col & 3) || ((uintptr_t)val & 3)) return false;
    if (nnz < 0 || (nnz > 0 && (!col || !val))) return false;
    return n_rows >= 1 && n_rows <= (int64_t)INT_MAX && n_cols >= 1 && n_cols <= (int64_t)INT_MAX;
}

}  // namespace tkr

extern "C" int64_t tkr_csr_spmm_workspace_bytes(int64_t n_rows) {
    if (n_rows < 1 || n_rows > (int64_t)INT_MAX) return TKR_EINVAL;
    return tkr::sp_list_bytes(n_rows);
}

extern "C" int tkr_csr_spmm(const int64_t* ptr, const int32_t* col, const float* val, int64_t nnz, int64_t n_rows, int32_t n_cols, const float* X,
                            int32_t k, double alpha, const float* Z, double beta, float* out, int64_t heavy_from, void* workspace,
                            int64_t workspace_bytes, int64_t* status, void* stream_) {
    using namespace tkr;
    if (!X || !out || !status || ((uintptr_t)X & 3) || ((uintptr_t)Z & 3) || ((uintptr_t)out & 3) || ((uintptr_t)status & 7) ||
        ((uintptr_t)workspace & 15))
        return TKR_EINVAL;
    if (!sp_csr_args_ok(ptr, col, val, nnz, n_rows, n_cols) || heavy_from < 1 || workspace_bytes < 0) return TKR_EINVAL;
    if (!std::isfinite(alpha) || !std::isfinite(beta)) return TKR_EINVAL;
    TKR_CHECK_RC(als_check_k(k, TKR_ALS_CG_MAX_K));
    const SpmmArgs A{ptr, col, val, (long long)nnz, (long long)n_rows, n_cols};
    if (sp_cap(A, heavy_from) > 0 && (!workspace || workspace_bytes < sp_list_bytes(n_rows))) return TKR_EINVAL;
    hipStream_t stream = (hipStream_t)stream_;
    unsigned long long* st = reinterpret_cast<unsigned long long*>(status);
    TKR_CHECK(hipMemsetAsync(st, 0xff, sizeof(unsigned long long), stream));          // -1: nothing refused
    return spmm(stream, A, X, k, alpha, Z, beta, out, heavy_from, 0, st, workspace);
}

extern "C" int64_t tkr_estep_cg_workspace_bytes(int64_t n_items, int64_t d, int32_t k) {
    if (n_items < 1 || d < 1 || n_items > (int64_t)INT_MAX || d > (int64_t)INT_MAX) return TKR_EINVAL;
    const int rc = tkr::als_check_k(k, TKR_ALS_CG_MAX_K);
    if (rc != TKR_OK) return rc;
    if (!tkr::es_flat_ok(n_items, k) || !tkr::es_flat_ok(d, k)) return TKR_EUNSUPPORTED;
    return tkr::EsRoom(n_items, d, k).bytes;
}

extern "C" int tkr_estep_cg(const int64_t* f_ptr, const int32_t* f_col, const float* f_val, const int64_t* t_ptr, const int32_t* t_col,
                            const float* t_val, int64_t nnz, int64_t n_items, int64_t d, const float* V, int32_t k, float* E, double lv, double le,
                            int32_t steps, int64_t heavy_from, void* workspace, int64_t workspace_bytes, int64_t* status, void* stream_) {
    using namespace tkr;
    if (!V || !E || !status || !workspace || ((uintptr_t)V & 3) || ((uintptr_t)E & 3) || ((uintptr_t)status & 7) || ((uintptr_t)workspace & 15))
        return TKR_EINVAL;
    if (!sp_csr_args_ok(f_ptr, f_col, f_val, nnz, n_items, d) || !sp_csr_args_ok(t_ptr, t_col, t_val, nnz, d, n_items)) return TKR_EINVAL;
    if (steps < 1 || heavy_from < 1 || !std::isfinite(lv) || !std::isfinite(le) || !(lv > 0.0) || !(le > 0.0)) return TKR_EINVAL;
    TKR_CHECK_RC(als_check_k(k, TKR_ALS_CG_MAX_K));
    if (!es_flat_ok(n_items, k) || !es_flat_ok(d, k)) return TKR_EUNSUPPORTED;
    const EsRoom at(n_items, d, k);
    if (workspace_bytes < at.bytes) return TKR_EINVAL;
    hipStream_t stream = (hipStream_t)stream_;
    unsigned long long* st = reinterpret_cast<unsigned long long*>(status);
    unsigned char* ws = reinterpret_cast<unsigned char*>(workspace);
    auto f32 = [&](int64_t off) { return reinterpret_cast<float*>(ws + off); };
    auto i32 = [&](int64_t off) { return reinterpret_cast<int*>(ws + off); };
    float *T = f32(at.T), *B = f32(at.B), *R = f32(at.R), *P = f32(at.P), *Q = f32(at.Q), *Xw = f32(at.X), *rr = f32(at.rr), *pq = f32(at.pq);
    int* halt = i32(at.halt);
    const SpmmArgs F{f_ptr, f_col, f_val, (long long)nnz, (long long)n_items, (int)d}, Ft{t_ptr, t_col, t_val, (long long)nnz, (long long)d, (int)n_items};
    const int n_slabs = (int)((d + kEsSlab - 1) / kEsSlab);
    const size_t n = (size_t)d * k;
    const dim3 grid((unsigned)n_slabs, (unsigned)((k + kEsCols - 1) / kEsCols)), block(kEsCols, kEsRuns);
    const unsigned flat = (unsigned)((n + 255) / 256);

    TKR_CHECK(hipMemsetAsync(st, 0xff, sizeof(unsigned long long), stream));          // -1: nothing refused
    // what may be refused of the input is refused by the three products and the scan of V, all before E is written
    hipLaunchKernelGGL(es_finite_kernel, dim3((unsigned)(((size_t)n_items * k + 255) / 256)), dim3(256), 0, stream, V, (size_t)n_items * k, k, st);
    TKR_LAUNCH_CHECK();
    TKR_CHECK_RC(spmm(stream, F, E, k, 1.0, nullptr, 0.0, T, heavy_from, 0, st, ws + at.list));                    // T = F E
    TKR_CHECK_RC(spmm(stream, Ft, T, k, lv, E, le, Q, heavy_from, n_items, st, ws + at.list));                     // W = lv F^T T + le E (in Q)
    TKR_CHECK_RC(spmm(stream, Ft, V, k, lv, nullptr, 0.0, B, heavy_from, n_items, st, ws + at.list));              // B = lv F^T V
    hipLaunchKernelGGL(es_init_kernel, grid, block, 0, stream, E, B, Q, (long long)d, k, Xw, R, P, rr);
    TKR_LAUNCH_CHECK();
    hipLaunchKernelGGL(es_begin_kernel, dim3(1), dim3(TKR_ALS_CG_MAX_K), 0, stream, st, k, halt, i32(at.refused));
    TKR_LAUNCH_CHECK();
    for (int step = 0; step < steps; ++step) {
        // (the products do not read `halt`: in a halted call they walk the same CSRs against whatever the workspace holds, refuse
        // the same rows again, and nothing they write leaves the workspace)
        TKR_CHECK_RC(spmm(stream, F, P, k, 1.0, nullptr, 0.0, T, heavy_from, 0, st, ws + at.list));                // T = F P
        TKR_CHECK_RC(spmm(stream, Ft, T, k, lv, P, le, Q, heavy_from, n_items, st, ws + at.list));                 // Q = lv F^T T + le P
        hipLaunchKernelGGL(es_dot_kernel, grid, block, 0, stream, P, Q, (long long)d, k, halt, pq);
        TKR_LAUNCH_CHECK();
        hipLaunchKernelGGL(es_alpha_kernel, dim3(1), dim3(TKR_ALS_CG_MAX_K), 0, stream, rr, pq, n_slabs, k, halt, i32(at.refused), i32(at.go),
                           f32(at.rho), f32(at.alpha), st);
        TKR_LAUNCH_CHECK();
        hipLaunchKernelGGL(es_update_kernel, grid, block, 0, stream, P, Q, (long long)d, k, halt, i32(at.go), f32(at.alpha), Xw, R, rr);
        TKR_LAUNCH_CHECK();
        hipLaunchKernelGGL(es_p_kernel, grid, block, 0, stream, R, (long long)d, k, halt, i32(at.go), f32(at.rho), rr, n_slabs, P);
        TKR_LAUNCH_CHECK();
    }
    hipLaunchKernelGGL(es_final_kernel, dim3(flat), dim3(256), 0, stream, Xw, n, k, halt, i32(at.refused), E);
    TKR_LAUNCH_CHECK();
    return TKR_OK;
}
