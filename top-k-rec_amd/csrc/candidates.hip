// K12 -- score and rank per-user candidate lists: many rows, a short list of candidate columns each (re-ranking a first-stage
// shortlist; evaluation against sampled negatives).  For entry e of row r with column c = cand_cols[e]:
//
//   score_out[e] = s(r, c)                       the one fp32 score of K4 / K8: exact_score (csrc/score_chain.h), masked entries too
//   rank_out[e]  = -1                            when c is masked for the row, else
//                  #{e' of the row, unmasked, e' != e : s(r, c_e') > s(r, c_e) or (equal and c_e' > c_e)}
//
// -- K4's canonical order restricted to the list.  The columns of a row are strictly ascending, so "c_e' > c_e" is "e' > e": the list
// is held as one 32-bit key per entry (rank_bits of the score: every NaN one key above +inf; 0 = masked, below every score), and with t = key - 1 for the entries behind
// the own one and t = key for those in front of it the rank is #{e' : key_e' > t_e'}: one compare and one add per pair.
//
// Two launches, no atomics, no workspace:
//   cand_rows_kernel   a wave per row of at most kCandResident entries, from first score to last rank.  Lane l scores entries l, l + 64,
//                      ...: the user row is uniform over the wave, the chain is sequential in k -- no reduction across lanes.  The item
//                      rows of the wave's 64 candidates come through LDS in slabs of the k dimension, loaded by all lanes together
//                      (staged_score below; k % 8 == 0 -- other widths: every lane gathers its own row, exact_score as it stands).
//                      The score is stored and its key put into the wave's kCandResident x 4 B of LDS.  Then lane l counts, for each
//                      of its entries, the keys ahead of it: b128 broadcast reads of the list, in three stretches (in front of the
//                      wave's 64 entries: t = key; among them: the full rule; behind them: t = key - 1).  Rows are dealt to waves in
//                      index order by the hardware's workgroup dispatcher, ~70 workgroups per CU at the design point, so a list of
//                      2,048 (the longest here) is no tail.
//   cand_long_kernel   rows longer than kCandResident, a whole workgroup per row: every thread scores entries tid, tid + 256, ... into
//                      score_out, then the row's keys are rebuilt from score_out and the mask in tiles of kCandResident in LDS and every
//                      thread counts its entries against each tile.  Quadratic in the length of the list (40,000 entries: ~40 ms):
//                      correct at any length up to n_cols, meant as the exception -- a caller that ranks most of the catalogue wants K4.
//                      Workgroup b looks at rows [256 b, 256 b + 256) and leaves at once when none of them is long.
// Out-of-contract columns (outside [0, n_cols)) are never dereferenced: score -inf, rank -1.
#include "tkr_common.h"
#include "topk_parts.h"
#include "../../include/tkr.h"

namespace tkr {

constexpr int kCandResident = TKR_CANDIDATES_RESIDENT;          // entries of a row whose keys stay in LDS (a multiple of 64)
constexpr int kCandWaves = 4;
static_assert(kCandResident % 64 == 0, "whole wave batches");

struct CandEntry { float score; uint32_t key; };

// score and key of entry `e`: the key is 0 when the column is masked for `row` (or no column at all)
__device__ __forceinline__ CandEntry cand_entry(const float* __restrict__ up, const float* __restrict__ Vt, const float* __restrict__ bias,
                                                int n_cols, int k, const uint32_t* __restrict__ mask, int pitch, int row, int c) {
    CandEntry r;
    if ((uint32_t)c >= (uint32_t)n_cols) { r.score = -INFINITY; r.key = 0u; return r; }
    r.score = exact_score(up, Vt + (size_t)c * k, k, bias, c);
    const bool masked = mask && col_masked(mask, pitch, row, c);
    r.key = masked ? 0u : rank_bits(r.score);
    return r;
}

__device__ __forceinline__ int count4_gt(uint4 o, uint32_t t) {
    return (o.x > t ? 1 : 0) + (o.y > t ? 1 : 0) + (o.z > t ? 1 : 0) + (o.w > t ? 1 : 0);
}
// the full rule for keys at list positions j .. j + 3 against the own key at position i
__device__ __forceinline__ int count4_rule(uint4 o, int j, uint32_t mine, int i) {
    return ((o.x > mine || (o.x == mine && j + 0 > i)) ? 1 : 0) + ((o.y > mine || (o.y == mine && j + 1 > i)) ? 1 : 0) +
           ((o.z > mine || (o.z == mine && j + 2 > i)) ? 1 : 0) + ((o.w > mine || (o.w == mine && j + 3 > i)) ? 1 : 0);
}

// ---- the item rows of the wave's 64 candidates staged through LDS (k % 8 == 0) ---------------------------------------------------
// A slab is kStageS factors of each k-half of every row: 8 consecutive lanes bring one row's slab (2 x 64 B) with one float4 load
// each, 8 loads per lane and slab, held in registers while the previous slab is consumed (the double buffer: registers + one LDS
// image), then written to the wave's image [64][2 kStageS + 4] (pitch 36 floats: conflict-free b128 reads); every lane runs the chain
// (csrc/score_chain.h chain_step4, chain_finish) over its own row out of LDS (measured against the form in which every lane gathers
// its own row with exact_score, bitwise equal on 120 M scores and 7-8 % faster: DESIGN.md section 4 K12).
constexpr int kStageS = 16, kStagePitch = 2 * kStageS + 4;

__device__ __forceinline__ float staged_score(const float* __restrict__ up, const float* __restrict__ Vt, const float* __restrict__ bias,
                                              int k, int c_own, bool live, float* __restrict__ img, int lane) {
    const int KH = k >> 1;
    const int piece = lane & 7, half = piece >> 2, f4 = piece & 3;
    const float* src[8];
#pragma unroll
    for (int q = 0; q < 8; ++q) src[q] = Vt + (size_t)__shfl(c_own, q * 8 + (lane >> 3), 64) * k + half * KH + f4 * 4;
    float* dst = img + (lane >> 3) * kStagePitch + half * kStageS + f4 * 4;
    const float* mine = img + lane * kStagePitch;
    float4 stg[8];
    auto fetch = [&](int s0) {
        const bool in = s0 + f4 * 4 < KH;                        // the last slab of a half may be short (KH % 4 == 0)
#pragma unroll
        for (int q = 0; q < 8; ++q) stg[q] = in ? *reinterpret_cast<const float4*>(src[q] + s0) : make_float4(0.f, 0.f, 0.f, 0.f);
    };
    float acc = 0.f;
    fetch(0);
    for (int s0 = 0; s0 < KH; s0 += kStageS) {
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");   // the previous slab is consumed
        __builtin_amdgcn_wave_barrier();
#pragma unroll
        for (int q = 0; q < 8; ++q) *reinterpret_cast<float4*>(dst + q * 8 * kStagePitch) = stg[q];
        if (s0 + kStageS < KH) fetch(s0 + kStageS);
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        __builtin_amdgcn_wave_barrier();
        const int n = min(kStageS, KH - s0);
        for (int kk = 0; kk < n; kk += 4) {
            const float4 a0 = *reinterpret_cast<const float4*>(mine + kk), a1 = *reinterpret_cast<const float4*>(mine + kStageS + kk);
            const float4 b0 = *reinterpret_cast<const float4*>(up + s0 + kk), b1 = *reinterpret_cast<const float4*>(up + KH + s0 + kk);
            chain_step4(acc, a0, a1, b0, b1);
        }
    }
    return chain_finish(acc, live ? bias : nullptr, c_own);
}

__global__ __launch_bounds__(kCandWaves * TKR_WAVE) void cand_rows_kernel(
    const float* __restrict__ U, const int32_t* __restrict__ uidx, int n_rows, const float* __restrict__ Vt,
    const float* __restrict__ bias, int n_cols, int k, const int64_t* __restrict__ cand_ptr, const int32_t* __restrict__ cand_cols,
    const uint32_t* __restrict__ mask, int pitch, float* __restrict__ score_out, int32_t* __restrict__ rank_out) {
    __shared__ __attribute__((aligned(16))) uint32_t keys_all[kCandWaves][kCandResident];
    __shared__ __attribute__((aligned(16))) float img_all[kCandWaves][64 * kStagePitch];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int row = blockIdx.x * kCandWaves + wave;
    if (row >= n_rows) return;
    const int64_t e0 = cand_ptr[row], len = cand_ptr[row + 1] - e0;
    if (len <= 0 || len > kCandResident) return;                 // empty; long rows: cand_long_kernel
    const int L = (int)len, Lp = (L + 63) & ~63;
    uint32_t* keys = keys_all[wave];
    const float* up = U + (size_t)(uidx ? uidx[row] : row) * k;
    if ((k & 7) == 0) {
        for (int i = lane; i < Lp; i += 64) {                    // wave-uniform trip count: every lane stages
            const int c = i < L ? cand_cols[e0 + i] : 0;
            const bool live = i < L && (uint32_t)c < (uint32_t)n_cols;
            float sc = staged_score(up, Vt, bias, k, live ? c : 0, live, img_all[wave], lane);
            uint32_t key = 0u;
            if (i < L) {
                if (!live) sc = -INFINITY;
                score_out[e0 + i] = sc;
                const bool masked = !live || (mask && col_masked(mask, pitch, row, c));
                key = masked ? 0u : rank_bits(sc);
            }
            keys[i] = key;
        }
    } else {                                                     // rows that are not 16-byte aligned: every lane gathers its own
        for (int i = lane; i < Lp; i += 64) {
            uint32_t key = 0u;                                   // the padding of the last batch: below everything
            if (i < L) {
                const CandEntry en = cand_entry(up, Vt, bias, n_cols, k, mask, pitch, row, cand_cols[e0 + i]);
                score_out[e0 + i] = en.score;
                key = en.key;
            }
            keys[i] = key;
        }
    }
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");       // the wave's own LDS writes, read back by its other lanes
    __builtin_amdgcn_wave_barrier();
    for (int c0 = 0; c0 < L; c0 += 64) {
        const int i = c0 + lane;
        const uint32_t mine = keys[i];                           // i < Lp
        int cnt = 0;
        for (int j = 0; j < c0; j += 4) cnt += count4_gt(*reinterpret_cast<const uint4*>(keys + j), mine);
#pragma unroll
        for (int j = 0; j < 64; j += 4) cnt += count4_rule(*reinterpret_cast<const uint4*>(keys + c0 + j), c0 + j, mine, i);
        const uint32_t below = mine - 1u;                        // mine = 0 (masked): nothing is counted, the rank is -1 anyway
        for (int j = c0 + 64; j < Lp; j += 4) cnt += count4_gt(*reinterpret_cast<const uint4*>(keys + j), below);
        if (i < L) rank_out[e0 + i] = mine ? cnt : -1;
    }
}

__global__ __launch_bounds__(256) void cand_long_kernel(
    const float* __restrict__ U, const int32_t* __restrict__ uidx, int n_rows, const float* __restrict__ Vt,
    const float* __restrict__ bias, int n_cols, int k, const int64_t* __restrict__ cand_ptr, const int32_t* __restrict__ cand_cols,
    const uint32_t* __restrict__ mask, int pitch, float* __restrict__ score_out, int32_t* __restrict__ rank_out) {
    __shared__ __attribute__((aligned(16))) uint32_t tile[kCandResident];
    const int tid = threadIdx.x;
    const int row_end = min(n_rows, (int)(blockIdx.x + 1) * 256);
    for (int row = blockIdx.x * 256; row < row_end; ++row) {     // workgroup-uniform: every thread walks the same rows
        const int64_t e0 = cand_ptr[row], len = cand_ptr[row + 1] - e0;
        if (len <= kCandResident || len > (int64_t)n_cols) continue;     // (longer than the catalogue: not strictly ascending columns)
        const int L = (int)len;
        const float* up = U + (size_t)(uidx ? uidx[row] : row) * k;
        for (int i = tid; i < L; i += 256)
            score_out[e0 + i] = cand_entry(up, Vt, bias, n_cols, k, mask, pitch, row, cand_cols[e0 + i]).score;
        __syncthreads();                                         // the row's scores are in score_out for every thread of the workgroup
        auto key_of = [&](int i) -> uint32_t {
            const int c = cand_cols[e0 + i];
            if ((uint32_t)c >= (uint32_t)n_cols) return 0u;
            const bool masked = mask && col_masked(mask, pitch, row, c);
            return masked ? 0u : rank_bits(score_out[e0 + i]);
        };
        for (int b0 = 0; b0 < L; b0 += 256) {
            const int i = b0 + tid;
            const uint32_t mine = i < L ? key_of(i) : 0u;
            int cnt = 0;
            for (int t0 = 0; t0 < L; t0 += kCandResident) {
                const int T = min(kCandResident, L - t0), Tp = (T + 3) & ~3;
                __syncthreads();                                 // the previous tile is counted
                for (int j = tid; j < Tp; j += 256) tile[j] = j < T ? key_of(t0 + j) : 0u;
                __syncthreads();
                for (int j = 0; j < Tp; j += 4) cnt += count4_rule(*reinterpret_cast<const uint4*>(tile + j), t0 + j, mine, i);
            }
            if (i < L) rank_out[e0 + i] = mine ? cnt : -1;
        }
        __syncthreads();                                         // the next long row of this block refills the tile
    }
}

}  // namespace tkr

extern "C" int tkr_rank_candidates(const float* U, const int32_t* user_idx, int32_t n_rows, const float* Vt, const float* bias,
                                   int32_t n_cols, int32_t k, const int64_t* cand_ptr, const int32_t* cand_cols, const uint32_t* mask,
                                   int32_t mask_pitch, float* score_out, int32_t* rank_out, void* stream_) {
    if (!U || !Vt || !cand_ptr || !cand_cols || !score_out || !rank_out) return TKR_EINVAL;
    if (n_rows <= 0 || n_cols <= 0 || k <= 0) return TKR_EINVAL;
    if (mask && mask_pitch < n_rows) return TKR_EINVAL;
    hipStream_t stream = (hipStream_t)stream_;
    hipLaunchKernelGGL(tkr::cand_long_kernel, dim3((n_rows + 255) / 256), dim3(256), 0, stream, U, user_idx, n_rows, Vt, bias, n_cols, k,
                       cand_ptr, cand_cols, mask, mask_pitch, score_out, rank_out);
    TKR_LAUNCH_CHECK();
    hipLaunchKernelGGL(tkr::cand_rows_kernel, dim3((n_rows + tkr::kCandWaves - 1) / tkr::kCandWaves), dim3(tkr::kCandWaves * TKR_WAVE), 0,
                       stream, U, user_idx, n_rows, Vt, bias, n_cols, k, cand_ptr, cand_cols, mask, mask_pitch, score_out, rank_out);
    TKR_LAUNCH_CHECK();
    return TKR_OK;
}
