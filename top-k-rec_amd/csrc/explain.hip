// K19 -- for every entry of a row's list, the e most similar items of a second, per-row set (the ANCHORS: the user's likes when a
// list is explained, the user's history when unexpectedness is measured).  The similarity is K17's,
//
//   sim(a, b) = chain(S[a], S[b])          S: dense fp32 [n_items, k], whatever the caller measures similarity in
//
// with chain = exact_score (csrc/score_chain.h) without bias: one fma chain per (entry, anchor) pair, kept in ONE lane from the first
// product to the last -- a chain is never reduced across lanes, which would change its bits.
//
//   nearest_anchors_kernel<STAGED, E, BLOCK>
//       one workgroup of BLOCK threads per row (256 up to t = 256 entries, 1024 above).  The valid prefix of the list is found as in
//       K17 (a ballot per wave, a minimum over the waves); an id outside [0, n_items) ends the row and is never used as an index.
//       The threads are cut into G = min(BLOCK / t, tile) groups of t: thread (g, p) owns entry p for good and takes the anchors
//       g, g + G, ... of every tile, so at t = 30 a wave works on (entry, anchor) pairs with 60 of 64 lanes instead of 30.
//       The anchors are streamed through the workgroup once, in tiles of at most kAncTile positions: their columns are checked
//       (one outside the table is skipped, reported and never used as an index) and kept in LDS, so a history may be of any length.
//       STAGED: the list's rows of S are brought into LDS once and every tile's rows behind them, all threads together (coalesced
//       over k), at K17's pitch: lanes that read different rows read conflict-free, lanes that read the same row get a broadcast.
//       Not STAGED (t + 8 rows do not fit the 160 KB of a CU): the same loop with both rows read through L2 at every chain.
//       A thread runs its chains of a tile four at a time on one read of its entry's row (chains<N>; two in the 1024-thread workgroup).
//       A thread keeps the E best (ordered similarity bits, inverted position) of its entry as packed 64-bit keys, sorted, in
//       registers; the keys of an entry are distinct, so the G lists of an entry merge into one result whatever the order: thread
//       (0, p) reads the others' from LDS in group order (the region of the staged rows, which are done with by then).
//       No atomics but the status word's minimum.
#include "tkr_common.h"
#include "topk_parts.h"
#include "../../include/tkr.h"

#include <limits.h>

#include <algorithm>

namespace tkr {

constexpr int kAncMaxT = TKR_ANCHOR_MAX_T;
constexpr int kAncMaxWaves = kAncMaxT / TKR_WAVE;
constexpr int kAncTile = 32;                                     // anchor positions of a tile, at most
constexpr int kAncMinTile = 8;                                   // STAGED needs room for this many
constexpr int kAncChains = 4;                                    // chains a thread runs side by side on one read of its entry's row (two in
                                                                 // the 1024-thread workgroup, whose threads have 128 registers)
constexpr int kAncHeadBytes = kAncMaxWaves * 4 + kAncTile * 4;   // the waves' prefix ends, the tile's checked columns
constexpr size_t kAncLdsBudget = 160 * 1024;                     // what one CU holds
static_assert(kAncMaxT % TKR_WAVE == 0 && kAncHeadBytes % 16 == 0 && kAncMaxT == TKR_MMR_MAX_POOL, "whole waves, an aligned image");
// K19's kinds (no kind 2): a list id outside the table ends the row; an anchor outside it was skipped; a bad anchor_ptr, padding only
enum { kAncBadId = 0, kAncSkipped = 1, kAncBadPtr = 3 };

// floats between two staged rows: K17's pitch (csrc/diversity.hip div_pitch) -- the rows of 16 (b128) resp. 32 (b32) consecutive
// lanes start in different 16-byte slots resp. banks
__host__ __device__ inline int anc_pitch(int k) {
    if ((k & 7) == 0) return ((k >> 2) & 1) ? k : k + 4;
    return (k & 1) ? k : k + 1;
}

__device__ __forceinline__ float key_sim(uint32_t ob) {          // the inverse of ordered_bits, for every bit pattern
    return __uint_as_float((ob & 0x80000000u) ? (ob & 0x7fffffffu) : ~ob);
}

// keys[0] > keys[1] > ... (0: an empty slot, below every key).  x goes in where it belongs, the last one drops out
template <int E>
__device__ __forceinline__ void keep_best(uint64_t (&keys)[E], uint64_t x) {
    if (x <= keys[E - 1]) return;
#pragma unroll
    for (int i = 0; i < E; ++i) {
        const bool gt = x > keys[i];
        const uint64_t up = gt ? x : keys[i];
        x = gt ? keys[i] : x;
        keys[i] = up;
    }
}

// N chains of one entry at once: exact_score(other[j], mine) for every j with the entry's row read ONCE per N chains -- the kernel is
// bound by its LDS reads, and this takes them from 2 to 1 + 1 / N rows per chain
template <int N>
__device__ __forceinline__ void chains(const float* __restrict__ mine, const float* const (&other)[N], int k, float (&out)[N]) {
    chain_rows<N, 2, 1, false>(mine, other, k, out);
#pragma unroll
    for (int j = 0; j < N; ++j) out[j] = chain_pos_zero(out[j]);     // no bias
}

// rows cols[0 .. n) of S -> dst[a][pitch], all threads together, coalesced over k; a row whose column is negative is left out.  With
// k % 8 == 0 a thread has four 16-byte loads in flight before it stores the first (a tile of 32 rows at k = 128 is one such batch)
template <int BLOCK>
__device__ __forceinline__ void stage_rows(float* __restrict__ dst, int pitch, const float* __restrict__ S, int k, const int* cols, int n) {
    const int tid = threadIdx.x;
    if ((k & 7) == 0) {                                           // the pitch is a multiple of four floats: 16-byte stores
        const int k4 = k >> 2, total = n * k4;
        for (int i0 = tid; i0 < total; i0 += 4 * BLOCK) {
            float4 v[4];
            int at[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) {                         // (a piece that is not wanted reads row 0 of S: a valid address, not stored)
                const int i = i0 + u * BLOCK < total ? i0 + u * BLOCK : 0;
                const int a = i / k4, j = (i - a * k4) * 4, c = cols[a];
                at[u] = (i0 + u * BLOCK < total && c >= 0) ? a * pitch + j : -1;
                v[u] = *reinterpret_cast<const float4*>(S + (size_t)max(c, 0) * k + j);
            }
#pragma unroll
            for (int u = 0; u < 4; ++u)
                if (at[u] >= 0) *reinterpret_cast<float4*>(dst + at[u]) = v[u];
        }
    } else {
        for (int i = tid; i < n * k; i += BLOCK) {
            const int a = i / k, j = i - a * k, c = cols[a];
            if (c >= 0) dst[(size_t)a * pitch + j] = S[(size_t)c * k + j];
        }
    }
}

template <bool STAGED, int E, int BLOCK>
__global__ __launch_bounds__(BLOCK) void nearest_anchors_kernel(const float* __restrict__ S, int n_items, int k, const int32_t* __restrict__ ids,
                                                                int t, const int64_t* __restrict__ anchor_ptr,
                                                                const int32_t* __restrict__ anchor_cols, long long n_anchors, int e, int pitch,
                                                                int tile, int32_t* __restrict__ best_pos, float* __restrict__ best_sim,
                                                                unsigned long long* __restrict__ status) {
    extern __shared__ __attribute__((aligned(16))) unsigned char anc_lds[];
    int* ends = reinterpret_cast<int*>(anc_lds);                                               // [kAncMaxWaves]
    int* acol_s = reinterpret_cast<int*>(anc_lds + kAncMaxWaves * 4);                          // [kAncTile]: -1 = skipped
    int* ids_s = reinterpret_cast<int*>(anc_lds + kAncHeadBytes);                              // [BLOCK]
    unsigned char* region = anc_lds + kAncHeadBytes + (size_t)BLOCK * 4;
    float* img = reinterpret_cast<float*>(region);                                             // STAGED: [t][pitch], the list's rows
    float* timg = img + (size_t)t * pitch;                                                     // STAGED: [tile][pitch], the tile's rows
    uint64_t* merge = reinterpret_cast<uint64_t*>(region);                                     // [t][G][E], after the last tile
    constexpr int NC = BLOCK <= 256 ? kAncChains : kAncChains / 2;
    const int tid = threadIdx.x, wave = tid >> 6;
    const int row = blockIdx.x;
    const unsigned long long word = (unsigned long long)row * 4ull;  // status_refuse's packing by hand: the three sites share the word

    // the valid prefix (thread p < t holds entry p)
    const int id = tid < t ? ids[(size_t)row * t + tid] : -1;
    ids_s[tid] = id;
    const bool bad = tid < t && (uint32_t)id >= (uint32_t)n_items;
    const unsigned long long b = __ballot(bad);
    if ((tid & 63) == 0) ends[wave] = b ? wave * TKR_WAVE + __ffsll(b) - 1 : t;
    __syncthreads();
    int n_valid = t;
    for (int w = 0; w < BLOCK / TKR_WAVE; ++w) n_valid = min(n_valid, ends[w]);
    if (tid == n_valid && bad && id >= 0) atomicMin(status, word + kAncBadId);

    // the row's anchors: the same two words in every thread
    const long long lo = anchor_ptr[row], hi = anchor_ptr[row + 1];
    const bool ptr_ok = lo >= 0 && lo <= hi && hi <= n_anchors && (row != 0 || lo == 0) && hi - lo <= (long long)INT_MAX;
    if (!ptr_ok && tid == 0) atomicMin(status, word + kAncBadPtr);
    const int n_anc = ptr_ok ? (int)(hi - lo) : 0;

    const int G = min(BLOCK / t, tile);
    const int g = tid / t, p = tid - g * t;
    const bool active = g < G && p < n_valid;
    const int my_id = active ? ids_s[p] : -1;
    if (STAGED) stage_rows<BLOCK>(img, pitch, S, k, ids_s, n_valid);
    const float* mine = STAGED ? img + (size_t)p * pitch : S + (size_t)(active ? my_id : 0) * k;
    uint64_t keys[E];
#pragma unroll
    for (int i = 0; i < E; ++i) keys[i] = 0ull;
    bool told = false;
    for (int base = 0; base < n_anc; base += tile) {              // workgroup-uniform: every thread takes every barrier
        const int n_here = min(tile, n_anc - base);
        if (tid < n_here) {
            const int c = anchor_cols[lo + base + tid];
            const bool ok = (uint32_t)c < (uint32_t)n_items;
            if (!ok && !told) {
                atomicMin(status, word + kAncSkipped);
                told = true;
            }
            acol_s[tid] = ok ? c : -1;
        }
        __syncthreads();                                          // (also: the list's rows are staged)
        if (n_valid > 0) {
            if (STAGED) {
                stage_rows<BLOCK>(timg, pitch, S, k, acol_s, n_here);
                __syncthreads();
            }
            if (active) {
                for (int a0 = g; a0 < n_here; a0 += NC * G) {         // the anchors a0, a0 + G, ... of this thread, NC at a time
                    const float* other[NC];
                    bool ok[NC];
                    int n_ok = 0;
#pragma unroll
                    for (int j = 0; j < NC; ++j) {
                        const int a = a0 + j * G;
                        const int c = a < n_here ? acol_s[a] : -1;
                        ok[j] = c >= 0 && c != my_id;                 // an item does not explain itself
                        n_ok += ok[j];
                        // (a chain that is not wanted runs on the thread's first anchor of the group: a valid address, the result unused)
                        other[j] = STAGED ? timg + (size_t)(ok[j] ? a : a0) * pitch : S + (size_t)(ok[j] ? c : 0) * k;
                    }
                    if (n_ok == 0) continue;
                    float sim[NC];
                    if (n_ok == 1) {                                  // short rows: one chain, not NC
                        const float* one = other[0];
#pragma unroll
                        for (int j = 1; j < NC; ++j) one = ok[j] ? other[j] : one;
                        const float s = exact_score(one, mine, k, nullptr, 0);
#pragma unroll
                        for (int j = 0; j < NC; ++j) sim[j] = s;
                    } else {
                        chains<NC>(mine, other, k, sim);
                    }
#pragma unroll
                    for (int j = 0; j < NC; ++j)
                        if (ok[j]) keep_best<E>(keys, ((uint64_t)ordered_bits(sim[j]) << 32) | (uint32_t)~(uint32_t)(base + a0 + j * G));
                }
            }
        }
        __syncthreads();                                          // the tile is done with
    }
    if (G > 1) {                                                  // (uniform) the G lists of an entry -> thread (0, p)
        __syncthreads();                                          // n_anc = 0: the staged rows may still be written
        if (g > 0 && g < G) {
#pragma unroll
            for (int i = 0; i < E; ++i) merge[((size_t)p * G + g) * E + i] = keys[i];
        }
        __syncthreads();
        if (g == 0 && p < n_valid) {
            for (int gg = 1; gg < G; ++gg) {
                for (int i = 0; i < E; ++i) {
                    const uint64_t x = merge[((size_t)p * G + gg) * E + i];
                    if (x <= keys[E - 1]) break;                  // sorted: what follows is smaller still
                    keep_best<E>(keys, x);
                }
            }
        }
    }
    if (tid < t) {                                                // g = 0, p = tid
        int32_t* op = best_pos + ((size_t)row * t + tid) * e;
        float* os = best_sim + ((size_t)row * t + tid) * e;
#pragma unroll
        for (int i = 0; i < E; ++i) {
            if (i < e) {
                const bool have = tid < n_valid && keys[i] != 0ull;
                op[i] = have ? (int32_t)~(uint32_t)keys[i] : -1;
                os[i] = have ? key_sim((uint32_t)(keys[i] >> 32)) : -INFINITY;
            }
        }
    }
}

template <bool STAGED, int E, int BLOCK>
static int launch_nearest_anchors(size_t lds, hipStream_t stream, int n_rows, const float* S, int n_items, int k, const int32_t* ids, int t,
                                  const int64_t* anchor_ptr, const int32_t* anchor_cols, long long n_anchors, int e, int pitch, int tile,
                                  int32_t* best_pos, float* best_sim, unsigned long long* status) {
    auto kern = nearest_anchors_kernel<STAGED, E, BLOCK>;
    if (lds > 64 * 1024)
        TKR_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)kAncLdsBudget));
    hipLaunchKernelGGL(kern, dim3(n_rows), dim3(BLOCK), lds, stream, S, n_items, k, ids, t, anchor_ptr, anchor_cols, n_anchors, e, pitch, tile,
                       best_pos, best_sim, status);
    TKR_LAUNCH_CHECK();
    return TKR_OK;
}

}  // namespace tkr

extern "C" int tkr_nearest_anchors(const float* S, int32_t n_items, int32_t k, const int32_t* ids, int32_t n_rows, int32_t t,
                                   const int64_t* anchor_ptr, const int32_t* anchor_cols, int64_t n_anchors, int32_t e, int32_t* best_pos,
                                   float* best_sim, int64_t* status, void* stream_) {
    if (!S || !ids || !anchor_ptr || !best_pos || !best_sim || !status || ((uintptr_t)status & 7)) return TKR_EINVAL;
    if (n_anchors < 0 || (n_anchors > 0 && !anchor_cols)) return TKR_EINVAL;
    if (n_items < 1 || k < 1 || n_rows < 1 || t < 1 || e < 1) return TKR_EINVAL;
    if (t > TKR_ANCHOR_MAX_T || e > TKR_ANCHOR_MAX_E) return TKR_EUNSUPPORTED;
    hipStream_t stream = (hipStream_t)stream_;
    unsigned long long* st = reinterpret_cast<unsigned long long*>(status);
    TKR_CHECK(hipMemsetAsync(st, 0xff, sizeof(unsigned long long), stream));          // -1: nothing refused
    const int block = t <= 256 ? 256 : 1024, E = e <= 4 ? 4 : 8, pitch = tkr::anc_pitch(k);
    const size_t head = (size_t)tkr::kAncHeadBytes + (size_t)block * 4, row_bytes = (size_t)pitch * 4;
    const bool staged = head + (size_t)(t + tkr::kAncMinTile) * row_bytes <= tkr::kAncLdsBudget;
    int tile = tkr::kAncTile;
    if (staged) tile = (int)std::min<size_t>(tkr::kAncTile, (tkr::kAncLdsBudget - head) / row_bytes - (size_t)t);
    const int G = std::min(block / t, tile);
    const size_t merge = G > 1 ? (size_t)t * G * E * 8 : 0, rows = staged ? (size_t)(t + tile) * row_bytes : 0;
    const size_t lds = head + std::max(rows, merge);              // merge <= 64 KB: inside the budget with any head
#define TKR_ANC_LAUNCH(ST, EE, BL)                                                                                                   \
    return tkr::launch_nearest_anchors<ST, EE, BL>(lds, stream, n_rows, S, n_items, k, ids, t, anchor_ptr, anchor_cols, (long long)n_anchors, \
                                                   e, pitch, tile, best_pos, best_sim, st)
    if (staged) {
        if (block == 256) { if (E == 4) TKR_ANC_LAUNCH(true, 4, 256); else TKR_ANC_LAUNCH(true, 8, 256); }
        if (E == 4) TKR_ANC_LAUNCH(true, 4, 1024); else TKR_ANC_LAUNCH(true, 8, 1024);
    }
    if (block == 256) { if (E == 4) TKR_ANC_LAUNCH(false, 4, 256); else TKR_ANC_LAUNCH(false, 8, 256); }
    if (E == 4) TKR_ANC_LAUNCH(false, 4, 1024); else TKR_ANC_LAUNCH(false, 8, 1024);
#undef TKR_ANC_LAUNCH
}
