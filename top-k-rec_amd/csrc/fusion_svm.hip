// K23 -- the sums of one Newton pass of the SVM fusion (the reference's old/methods/sfusion.py: LinearSVC(C) on the score differences of
// sampled triplets; top-k-rec_amd/svmfusion.py runs the Newton iteration on the host in fp64).  The rows are K16's features
// (tkr_fusion_features: D[t, m] = fl(s_m(u, i) - s_m(u, j))); row g = first_row + t carries the label y = +1 (g even) or -1 (g odd) and,
// in the space of margins, is x~ = (d, y):  z = sum_m W[m] d[m] + y W[M].  Over the ACTIVE rows (1 - z > 0, strictly) a pass needs
//   S = sum x~ x~^T (upper triangle),   r = sum (1 - z) x~,   q = sum (1 - z)^2,   and their number.
//
//   fusion_svm_sums_kernel     one workgroup per slab of TKR_FUSION_SVM_SLAB rows; slabs are cut at multiples of the slab in g, so which
//                              thread takes a row and at which turn depends on g alone: thread (g % slab) % 256, turn (g % slab) / 256.
//                              A thread keeps W, the row and its (M + 1)(M + 2) / 2 + M + 3 sums in registers (M is a template
//                              argument), everything in fp64, every product-and-add one fma.  Lanes are combined by one fixed tree (DPP, the
//                              tree of wave_sum in tkr_common.h on both halves of a double), the four waves in wave order through LDS.
//   fusion_svm_reduce_kernel   one workgroup: entry e of the result is the slabs' entries e added in ascending slab order.
//
// No float atomics: the only atomic is the status word's minimum.  A row with an entry that is not finite is never summed.
#include "tkr_common.h"
#include "../../include/tkr.h"

#pragma clang fp contract(off)   // every rounding below is written out: fma where one is meant

namespace tkr {

constexpr int kSvmThreads = 256, kSvmWaves = kSvmThreads / TKR_WAVE;
constexpr int kSvmSlab = TKR_FUSION_SVM_SLAB;
constexpr int kSvmReduceAhead = 32;
static_assert(kSvmSlab % kSvmThreads == 0, "a slab is a whole number of turns of the workgroup");

// the words of one slab's partial and of the result: S | r | q | count
__host__ __device__ constexpr int svm_words(int M) { return (M + 1) * (M + 2) / 2 + M + 3; }
static_assert(svm_words(TKR_FUSION_MAX_MODELS) <= kSvmThreads, "the reduce kernel gives every word a thread");

template <int CTRL, int ROW_MASK = 0xf>
__device__ __forceinline__ double dpp_add_d(double v) {          // dpp_add of tkr_common.h on a double: lanes masked off add +0.0
    const long long b = __double_as_longlong(v);
    const int lo = __builtin_amdgcn_update_dpp(0, (int)b, CTRL, ROW_MASK, 0xf, false);
    const int hi = __builtin_amdgcn_update_dpp(0, (int)(b >> 32), CTRL, ROW_MASK, 0xf, false);
    return v + __longlong_as_double(((long long)hi << 32) | (long long)(unsigned)lo);
}

// the sum over the 64 lanes, in lane 63 (the tree of wave_sum)
__device__ __forceinline__ double wave_sum_d63(double v) {
    v = dpp_add_d<0xb1>(v);
    v = dpp_add_d<0x4e>(v);
    v = dpp_add_d<0x124>(v);
    v = dpp_add_d<0x128>(v);
    v = dpp_add_d<0x142, 0xa>(v);
    v = dpp_add_d<0x143, 0xc>(v);
    return v;
}

// M: the number of models; VEC: the rows of D are 16-byte aligned and come in float4 loads (fusion_sgd_kernel, csrc/fusion.hip: a row
// per thread walks every cache line M times with dword loads).
template <int M, bool VEC>
__global__ __launch_bounds__(kSvmThreads) void fusion_svm_sums_kernel(const float* __restrict__ D, int64_t n_rows, int64_t first_row,
                                                                     const double* __restrict__ W, double* __restrict__ partial,
                                                                     unsigned long long* __restrict__ status) {
    constexpr int X = M + 1, NS = X * (X + 1) / 2, WORDS = svm_words(M);
    __shared__ double red[kSvmWaves][WORDS];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    double w[X];
#pragma unroll
    for (int m = 0; m < X; ++m) w[m] = W[m];
    double S[NS], r[X], q = 0.0, cnt = 0.0;
#pragma unroll
    for (int e = 0; e < NS; ++e) S[e] = 0.0;
#pragma unroll
    for (int m = 0; m < X; ++m) r[m] = 0.0;
    const int64_t g0 = (first_row / kSvmSlab + (int64_t)blockIdx.x) * kSvmSlab, g_end = first_row + n_rows;
    // Rows in flight: a turn's loads do not depend on the turn before, but nothing can be loaded ahead of a bounds check -- so a turn
    // outside the call (the first and the last slab may be cut) loads row 0, which every call has, and is dropped afterwards.
    constexpr int kTurnsInFlight = M <= 4 ? 4 : M <= 8 ? 2 : 1;
#pragma unroll kTurnsInFlight
    for (int turn = 0; turn < kSvmSlab / kSvmThreads; ++turn) {
        const int64_t g = g0 + turn * kSvmThreads + tid;
        const bool inside = g >= first_row && g < g_end;
        const float* row = D + (size_t)(inside ? g - first_row : 0) * M;
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
        bool finite = true;
#pragma unroll
        for (int m = 0; m < M; ++m) finite = finite && (__float_as_uint(d[m]) & 0x7f800000u) != 0x7f800000u;
        if (!inside) continue;
        if (!finite) {                                            // refused: the smallest such row is what the caller hears of
            atomicMin(status, (unsigned long long)g);
            continue;
        }
        double x[X];
#pragma unroll
        for (int m = 0; m < M; ++m) x[m] = (double)d[m];
        x[M] = (g & 1) ? -1.0 : 1.0;
        double z = 0.0;
#pragma unroll
        for (int m = 0; m < X; ++m) z = fma(w[m], x[m], z);
        const double a = 1.0 - z;
        if (a > 0.0) {
            int e = 0;
#pragma unroll
            for (int i = 0; i < X; ++i) {
#pragma unroll
                for (int j = i; j < X; ++j, ++e) S[e] = fma(x[i], x[j], S[e]);
            }
#pragma unroll
            for (int m = 0; m < X; ++m) r[m] = fma(a, x[m], r[m]);
            q = fma(a, a, q);
            cnt = cnt + 1.0;
        }
    }
    // lanes: the fixed tree; lane 63 holds the wave's sums
#pragma unroll
    for (int e = 0; e < NS; ++e) {
        const double s = wave_sum_d63(S[e]);
        if (lane == 63) red[wave][e] = s;
    }
#pragma unroll
    for (int m = 0; m < X; ++m) {
        const double s = wave_sum_d63(r[m]);
        if (lane == 63) red[wave][NS + m] = s;
    }
    q = wave_sum_d63(q);
    cnt = wave_sum_d63(cnt);
    if (lane == 63) {
        red[wave][NS + X] = q;
        red[wave][NS + X + 1] = cnt;
    }
    __syncthreads();
    if (tid < WORDS) {                                            // the waves in wave order
        double s = red[0][tid];
#pragma unroll
        for (int v = 1; v < kSvmWaves; ++v) s = s + red[v][tid];
        partial[(size_t)blockIdx.x * WORDS + tid] = s;
    }
}

// out[e] = sum over the slabs, ascending, of partial[slab, e]; the count (whole numbers below 2^53 in fp64: exact) leaves as int64.
// A refusal leaves out as it is.
__global__ __launch_bounds__(kSvmThreads) void fusion_svm_reduce_kernel(const double* __restrict__ partial, int64_t n_slabs, int words,
                                                                       double* __restrict__ out, const unsigned long long* __restrict__ status) {
    if (*status != ~0ull) return;
    const int e = threadIdx.x;
    if (e >= words) return;
    double s = 0.0;
    for (int64_t b0 = 0; b0 < n_slabs; b0 += kSvmReduceAhead) {   // the loads of kSvmReduceAhead slabs at once, the additions one by one
        double v[kSvmReduceAhead];
#pragma unroll
        for (int i = 0; i < kSvmReduceAhead; ++i) v[i] = b0 + i < n_slabs ? partial[(size_t)(b0 + i) * words + e] : 0.0;
#pragma unroll
        for (int i = 0; i < kSvmReduceAhead; ++i)
            if (b0 + i < n_slabs) s = s + v[i];
    }
    if (e == words - 1) reinterpret_cast<long long*>(out)[e] = (long long)s;
    else out[e] = s;
}

template <int M>
static void launch_svm_sums(const float* D, int64_t n_rows, int64_t first_row, const double* W, double* partial, unsigned long long* status,
                            unsigned n_slabs, hipStream_t stream) {
    if constexpr (M % 4 == 0) {
        if (((uintptr_t)D & 15) == 0) {
            hipLaunchKernelGGL((fusion_svm_sums_kernel<M, true>), dim3(n_slabs), dim3(kSvmThreads), 0, stream, D, n_rows, first_row, W, partial, status);
            return;
        }
    }
    hipLaunchKernelGGL((fusion_svm_sums_kernel<M, false>), dim3(n_slabs), dim3(kSvmThreads), 0, stream, D, n_rows, first_row, W, partial, status);
}

// the slabs that rows [first_row, first_row + n_rows) touch
static int64_t svm_slabs(int64_t n_rows, int64_t first_row) {
    return (first_row + n_rows - 1) / kSvmSlab - first_row / kSvmSlab + 1;
}

static bool svm_range_ok(int64_t n_rows, int32_t n_models, int64_t first_row) {
    return n_models >= 1 && n_models <= TKR_FUSION_MAX_MODELS && n_rows >= 1 && first_row >= 0 && n_rows <= ((int64_t)1 << 42) &&
           first_row <= ((int64_t)1 << 42);                       // at most 2^31 slabs in a call, and g stays far below 2^53
}

}  // namespace tkr

extern "C" int64_t tkr_fusion_svm_partial_bytes(int64_t n_rows, int32_t n_models, int64_t first_row) {
    if (!tkr::svm_range_ok(n_rows, n_models, first_row)) return TKR_EINVAL;
    return tkr::svm_slabs(n_rows, first_row) * tkr::svm_words(n_models) * (int64_t)sizeof(double);
}

extern "C" int tkr_fusion_svm_sums(const float* D, int64_t n_rows, int32_t n_models, int64_t first_row, const double* W, double* partial,
                                   int64_t partial_bytes, int64_t slab_offset, double* out, int64_t* status, void* stream_) {
    if (!D || !W || !partial || !status || !tkr::svm_range_ok(n_rows, n_models, first_row)) return TKR_EINVAL;
    if (((uintptr_t)D & 3) || ((uintptr_t)W & 7) || ((uintptr_t)partial & 7) || ((uintptr_t)out & 7) || ((uintptr_t)status & 7)) return TKR_EINVAL;
    const int words = tkr::svm_words(n_models);
    const int64_t n_slabs = tkr::svm_slabs(n_rows, first_row);
    if (slab_offset < 0 || slab_offset > ((int64_t)1 << 31) || partial_bytes < 0 ||
        (slab_offset + n_slabs) > partial_bytes / (words * (int64_t)sizeof(double)))
        return TKR_EINVAL;
    hipStream_t stream = (hipStream_t)stream_;
    unsigned long long* st = reinterpret_cast<unsigned long long*>(status);
    if (slab_offset == 0) TKR_CHECK(hipMemsetAsync(st, 0xff, sizeof(unsigned long long), stream));          // -1: nothing refused
    double* mine = partial + (size_t)slab_offset * words;
    switch (n_models) {
#define TKR_SVM_CASE(M) case M: tkr::launch_svm_sums<M>(D, n_rows, first_row, W, mine, st, (unsigned)n_slabs, stream); break;
        TKR_SVM_CASE(1) TKR_SVM_CASE(2) TKR_SVM_CASE(3) TKR_SVM_CASE(4) TKR_SVM_CASE(5) TKR_SVM_CASE(6) TKR_SVM_CASE(7) TKR_SVM_CASE(8)
        TKR_SVM_CASE(9) TKR_SVM_CASE(10) TKR_SVM_CASE(11) TKR_SVM_CASE(12) TKR_SVM_CASE(13) TKR_SVM_CASE(14) TKR_SVM_CASE(15) TKR_SVM_CASE(16)
#undef TKR_SVM_CASE
    }
    TKR_LAUNCH_CHECK();
    if (out) {
        hipLaunchKernelGGL(tkr::fusion_svm_reduce_kernel, dim3(1), dim3(tkr::kSvmThreads), 0, stream, partial, slab_offset + n_slabs, words, out, st);
        TKR_LAUNCH_CHECK();
    }
    return TKR_OK;
}
