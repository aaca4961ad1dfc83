// K17 -- look at a finished top-k list as a whole: greedy Maximal Marginal Relevance (Carbonell & Goldstein) over a pool per row, and
// the pairwise dissimilarity sums the list metrics (intra-list diversity) are prefix sums of.  Both are built on one primitive, the
// similarity of two pool entries of a row,
//
//   sim(a, b) = chain(S[id_a], S[id_b])          S: dense fp32 [n_items, k], whatever the caller measures similarity in
//
// with chain = exact_score (csrc/score_chain.h) without bias: the fma chain of K4 / K8 / K12 with the two k-halves interleaved, the one
// fp32 order of the library (oracle/ref_np.py mfma_chain_scores).  Products commute and the order is fixed: sim(a, b) == sim(b, a) bit
// for bit.
//
//   mmr_kernel<STAGED>   one workgroup per row, a thread per pool entry (64 .. 1024 threads: one wave up to 64 entries).  The valid
//                        prefix of the pool is found first (a ballot per wave, a minimum over the waves); an id outside [0, n_items)
//                        ends the row and is never used as an index.  STAGED: the valid entries' rows of S are brought into LDS once,
//                        all threads together (coalesced over k), at a pitch that makes the lane-per-row reads of the chain
//                        conflict-free (k % 8 == 0: b128 reads, pitch / 4 odd; other k: b32 reads, pitch odd); every pick then costs
//                        one chain per thread, own row against the picked row (the same address in every lane: a broadcast), all out
//                        of LDS.  Not STAGED (the rows do not fit): the same loop with both rows read through L2 at every step.
//                        The argmax of a step is a 64-bit maximum of (ordered objective bits, inverted position): a butterfly inside the
//                        wave (DPP / ds_swizzle, csrc/topk_parts.h lane_xor), one LDS word per wave and one barrier across the waves
//                        (the words are double-buffered by the parity of the step).  No atomics but the status word's minimum.
//   pair_sums_kernel     one workgroup per list, thread b sums 1 - sim(a, b) over a < b in float64, a ascending (the lists are short:
//                        their rows stay in L1 / L2).
#include "tkr_common.h"
#include "topk_parts.h"
#include "../../include/tkr.h"

#include <math.h>

namespace tkr {

constexpr int kDivMaxPool = TKR_MMR_MAX_POOL;                    // entries of a row: a thread each
constexpr int kDivMaxWaves = kDivMaxPool / TKR_WAVE;
constexpr int kDivHeadBytes = 2 * kDivMaxWaves * 8 + kDivMaxWaves * 4;       // the waves' argmax words (two parities), their prefix ends
constexpr size_t kDivLdsBudget = 160 * 1024;                     // what one CU holds
static_assert(kDivMaxPool % TKR_WAVE == 0 && kDivHeadBytes % 16 == 0, "whole waves, an aligned image");
enum { kDivBadId = 1 };                                          // the one kind of K17's status word: an id outside the table ends row `where`

// floats between the staged rows: lane l reads row l, so the rows of 16 (b128) resp. 32 (b32) consecutive lanes must start in
// different 16-byte slots resp. banks
__host__ __device__ inline int div_pitch(int k) {
    if ((k & 7) == 0) return ((k >> 2) & 1) ? k : k + 4;
    return (k & 1) ? k : k + 1;
}

__device__ __forceinline__ uint64_t wave_max_key(uint64_t key) {
    uint32_t hi = (uint32_t)(key >> 32), lo = (uint32_t)key;
    auto step = [&](uint32_t ohi, uint32_t olo) {
        const bool other_gt = (ohi > hi) || (ohi == hi && olo > lo);
        hi = other_gt ? ohi : hi;
        lo = other_gt ? olo : lo;
    };
    step(lane_xor<1>(hi), lane_xor<1>(lo));
    step(lane_xor<2>(hi), lane_xor<2>(lo));
    step(lane_xor<4>(hi), lane_xor<4>(lo));
    step(lane_xor<8>(hi), lane_xor<8>(lo));
    step(lane_xor<16>(hi), lane_xor<16>(lo));
    step(lane_xor<32>(hi), lane_xor<32>(lo));
    return ((uint64_t)hi << 32) | lo;
}

// the valid prefix of a row's ids (thread e holds entry e, -1 behind the row's end): its length, the same in every thread.  The entry
// that ends it, when it is an id >= n_items, is reported (status_refuse, tkr_common.h).  One barrier.
__device__ __forceinline__ int valid_prefix(int id, int n, int n_items, int row, int* ends, unsigned long long* status) {
    const int tid = threadIdx.x, wave = tid >> 6, n_waves = blockDim.x >> 6;
    const bool bad = tid < n && (uint32_t)id >= (uint32_t)n_items;
    const unsigned long long b = __ballot(bad);
    if ((tid & 63) == 0) ends[wave] = b ? wave * TKR_WAVE + __ffsll(b) - 1 : n;
    __syncthreads();
    int n_valid = n;
    for (int w = 0; w < n_waves; ++w) n_valid = min(n_valid, ends[w]);
    if (tid == n_valid && bad && id >= 0) status_refuse(status, row, kDivBadId);
    return n_valid;
}

template <bool STAGED>
__global__ __launch_bounds__(kDivMaxPool) void mmr_kernel(const float* __restrict__ S, int n_items, int k, const int32_t* __restrict__ ids,
                                                          const float* __restrict__ rel, int N, float lam32, float mu32, int t, int pitch,
                                                          int32_t* __restrict__ sel_pos, unsigned long long* __restrict__ status) {
    extern __shared__ __attribute__((aligned(16))) unsigned char div_lds[];
    uint64_t* wkey = reinterpret_cast<uint64_t*>(div_lds);                                     // [2][kDivMaxWaves]
    int* ends = reinterpret_cast<int*>(div_lds + 2 * kDivMaxWaves * 8);                        // [kDivMaxWaves]
    int* ids_s = reinterpret_cast<int*>(div_lds + kDivHeadBytes);                              // [blockDim.x]
    float* img = reinterpret_cast<float*>(div_lds + kDivHeadBytes + (size_t)blockDim.x * 4);   // STAGED: [n_valid][pitch]
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, n_waves = blockDim.x >> 6;
    const int row = blockIdx.x;
    const int id = tid < N ? ids[(size_t)row * N + tid] : -1;
    ids_s[tid] = id;
    const int n_valid = valid_prefix(id, N, n_items, row, ends, status);      // (its barrier: ids_s is written for every thread)
    const bool live = tid < n_valid;
    if (STAGED) {
        if ((k & 7) == 0) {                                       // the pitch is a multiple of four floats: 16-byte stores
            const int k4 = k >> 2;
            for (int i = tid; i < n_valid * k4; i += blockDim.x) {
                const int e = i / k4, j = (i - e * k4) * 4;
                *reinterpret_cast<float4*>(img + (size_t)e * pitch + j) = *reinterpret_cast<const float4*>(S + (size_t)ids_s[e] * k + j);
            }
        } else {
            for (int i = tid; i < n_valid * k; i += blockDim.x) {
                const int e = i / k, j = i - e * k;
                img[(size_t)e * pitch + j] = S[(size_t)ids_s[e] * k + j];
            }
        }
        __syncthreads();
    }
    const float* mine = STAGED ? img + (size_t)tid * pitch : S + (size_t)(live ? id : 0) * k;
    const float a = live ? __fmul_rn(lam32, rel[(size_t)row * N + tid]) : 0.f;
    float pen = -INFINITY;
    bool picked = false;
    const int picks = min(t, n_valid);
    for (int r = 0; r < picks; ++r) {                             // workgroup-uniform: every thread takes every barrier
        const float obj = (r == 0 ? a : fmaf(-mu32, pen, a)) + 0.0f;        // -0.0 -> +0.0: equal objectives have equal keys
        uint64_t key = (live && !picked) ? (((uint64_t)ordered_bits(obj) << 32) | (uint32_t)~tid) : 0ull;
        key = wave_max_key(key);
        uint64_t* slot = wkey + (r & 1) * kDivMaxWaves;
        if (lane == 0) slot[wave] = key;
        __syncthreads();
        uint64_t best = slot[0];
        for (int w = 1; w < n_waves; ++w) best = slot[w] > best ? slot[w] : best;
        const int p = (int)~(uint32_t)best;                       // r < n_valid: an unpicked valid entry exists, p < n_valid
        if (tid == 0) sel_pos[(size_t)row * t + r] = p;
        if (tid == p) picked = true;
        if (r + 1 < picks && live && !picked) {
            const float* other = STAGED ? img + (size_t)p * pitch : S + (size_t)ids_s[p] * k;
            pen = fmaxf(pen, exact_score(other, mine, k, nullptr, 0));
        }
    }
    for (int r = picks + tid; r < t; r += blockDim.x) sel_pos[(size_t)row * t + r] = -1;
}

__global__ __launch_bounds__(kDivMaxPool) void pair_sums_kernel(const float* __restrict__ S, int n_items, int k, const int32_t* __restrict__ ids,
                                                                int t, double* __restrict__ pair_sum, unsigned long long* __restrict__ status) {
    __shared__ int ends[kDivMaxWaves];
    __shared__ int ids_s[kDivMaxPool];
    const int tid = threadIdx.x, row = blockIdx.x;
    const int id = tid < t ? ids[(size_t)row * t + tid] : -1;
    ids_s[tid] = id;
    const int n_valid = valid_prefix(id, t, n_items, row, ends, status);
    if (tid >= t) return;
    double sum = 0.0;
    if (tid < n_valid) {
        const float* mine = S + (size_t)id * k;
        for (int a = 0; a < tid; ++a) sum += 1.0 - (double)exact_score(S + (size_t)ids_s[a] * k, mine, k, nullptr, 0);
    }
    pair_sum[(size_t)row * t + tid] = sum;
}

}  // namespace tkr

extern "C" int tkr_mmr_select(const float* S, int32_t n_items, int32_t k, const int32_t* ids, const float* rel, int32_t n_rows, int32_t N,
                              double lam, int32_t t, int32_t* sel_pos, int64_t* status, void* stream_) {
    if (!S || !ids || !rel || !sel_pos || !status || ((uintptr_t)status & 7)) return TKR_EINVAL;
    if (n_items < 1 || k < 1 || n_rows < 1 || N < 1 || t < 1 || t > N) return TKR_EINVAL;
    if (!isfinite(lam) || lam < 0.0 || lam > 1.0) return TKR_EINVAL;
    if (N > tkr::kDivMaxPool) return TKR_EUNSUPPORTED;
    hipStream_t stream = (hipStream_t)stream_;
    unsigned long long* st = reinterpret_cast<unsigned long long*>(status);
    TKR_CHECK(hipMemsetAsync(st, 0xff, sizeof(unsigned long long), stream));          // -1: nothing refused
    const float lam32 = (float)lam, mu32 = 1.0f - lam32;
    const int block = (N + TKR_WAVE - 1) / TKR_WAVE * TKR_WAVE, pitch = tkr::div_pitch(k);
    const size_t head = (size_t)tkr::kDivHeadBytes + (size_t)block * 4, rows = (size_t)N * pitch * 4;
    const bool staged = head + rows <= tkr::kDivLdsBudget;
    const size_t lds = staged ? head + rows : head;
    auto kern = staged ? tkr::mmr_kernel<true> : tkr::mmr_kernel<false>;
    if (lds > 64 * 1024)
        TKR_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)tkr::kDivLdsBudget));
    hipLaunchKernelGGL(kern, dim3(n_rows), dim3(block), lds, stream, S, n_items, k, ids, rel, N, lam32, mu32, t, pitch, sel_pos, st);
    TKR_LAUNCH_CHECK();
    return TKR_OK;
}

extern "C" int tkr_list_pair_sums(const float* S, int32_t n_items, int32_t k, const int32_t* ids, int32_t n_rows, int32_t t, double* pair_sum,
                                  int64_t* status, void* stream_) {
    if (!S || !ids || !pair_sum || !status || ((uintptr_t)status & 7) || ((uintptr_t)pair_sum & 7)) return TKR_EINVAL;
    if (n_items < 1 || k < 1 || n_rows < 1 || t < 1) return TKR_EINVAL;
    if (t > tkr::kDivMaxPool) return TKR_EUNSUPPORTED;
    hipStream_t stream = (hipStream_t)stream_;
    unsigned long long* st = reinterpret_cast<unsigned long long*>(status);
    TKR_CHECK(hipMemsetAsync(st, 0xff, sizeof(unsigned long long), stream));
    const int block = (t + TKR_WAVE - 1) / TKR_WAVE * TKR_WAVE;
    hipLaunchKernelGGL(tkr::pair_sums_kernel, dim3(n_rows), dim3(block), 0, stream, S, n_items, k, ids, t, pair_sum, st);
    TKR_LAUNCH_CHECK();
    return TKR_OK;
}
