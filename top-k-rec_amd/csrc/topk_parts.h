// Device helpers of K4 and K8 (csrc/topk.hip, csrc/topk_refine.hip, csrc/like_ranks.hip): ordered keys, the wave-wide bitonic sorts,
// the bounds the item ranges of a user block tell each other, the fp32 MFMA tile, the prologue of the fp16 bound-and-refine kernels.
// The fp32 score of one (user, item) pair is csrc/score_chain.h, included here for every file that scores pairs.
#pragma once
#include "tkr_common.h"
#include "score_chain.h"

namespace tkr {

typedef float f32x16 __attribute__((ext_vector_type(16)));

constexpr int kTopkMaxWaves = 8;
constexpr int kCap = 64;                 // candidate slots per user (= wave width: one entry per lane in a trim)
constexpr int kMaxK = 32;                // K + 32 (largest per-tile inflow) <= kCap
constexpr int TKR_EAGAIN_EXACT = -100;   // internal: the bound-and-refine launch cannot run here (no workspace for its flags)

__device__ __forceinline__ uint32_t ordered_bits(float s) {      // monotone float -> uint
    const uint32_t f = __float_as_uint(s);
    return (f & 0x80000000u) ? ~f : (f | 0x80000000u);
}

// The canonical order covers every fp32 value (include/tkr.h, K4): NaN > +inf > finite > -inf, and every NaN, whatever its sign and
// payload, is the same score.  rank_score is that one NaN (the positive quiet one) for a NaN, s itself otherwise; rank_bits its
// ordered bits, 0xffc00000 for a NaN: above +inf, never 0 and never 0xffffffff (the "absent" and "no rank" words of the keys).
// bound_score turns a K-th best score into a filter threshold: +inf for a NaN -- thresholds are never NaN, and what reaches a
// threshold t is !(s < t), which a NaN score always does.
constexpr uint32_t kNanBits = 0x7fc00000u;
__device__ __forceinline__ float rank_score(float s) { return (s != s) ? __uint_as_float(kNanBits) : s; }
__device__ __forceinline__ uint32_t rank_bits(float s) { return (s != s) ? (kNanBits | 0x80000000u) : ordered_bits(s); }
__device__ __forceinline__ float bound_score(float s) { return fminf(s, INFINITY); }

// value of lane (lane ^ STRIDE).  Strides 1..8 stay in the VALU (DPP), 16 uses the LDS crossbar without
// an address (ds_swizzle), only 32 needs a bpermute.
__device__ __forceinline__ float unordered_bits(uint32_t ob) {    // inverse of ordered_bits; 0 -> below every float
    if (ob == 0u) return -INFINITY;
    return __uint_as_float((ob & 0x80000000u) ? (ob & 0x7fffffffu) : ~ob);
}

// Item-range splits of one user block cooperate through thr_shared[row]: the K-th best score inside ANY subset of
// the catalogue is a lower bound of the K-th best overall, so every range may filter with the largest bound any
// range has published.  Ranges are dispatched range-major (blockIdx.x fastest), so later ranges start with the
// thresholds of earlier ones instead of -inf and skip the expensive low-threshold phase.  Results do not depend on
// the timing: a column of the global top K passes every such bound, and the final order comes from the exact sorts.
__device__ __forceinline__ float share_threshold(uint32_t* thr_shared, int row, bool publish, float thr) {
    if (!thr_shared) return thr;
    uint32_t seen = 0u;
    if (publish && thr > -INFINITY) seen = atomicMax(&thr_shared[row], ordered_bits(thr));
    seen = max(seen, (uint32_t)__shfl_xor((int)seen, 32, 64));  // the h = 1 lane of the user gets it too
    return fmaxf(thr, unordered_bits(seen));
}
// Bound-and-refine arithmetic: the filter runs on approximate scores with `thr` = (lower bound of the K-th best EXACT score)
// - margin; what the item ranges of a block tell each other is the bound itself.
// thr and margin are in the user's scaled units (scale = a power of two), the shared word is not.
__device__ __forceinline__ float share_bound(uint32_t* thr_shared, int row, bool publish, float thr, float margin, float scale,
                                             float inv_scale) {
    if (!thr_shared) return thr;
    uint32_t seen = 0u;
    if (publish && thr > -INFINITY) seen = atomicMax(&thr_shared[row], ordered_bits((thr + margin) * inv_scale));
    seen = max(seen, (uint32_t)__shfl_xor((int)seen, 32, 64));
    return fmaxf(thr, unordered_bits(seen) * scale - margin);
}

// 2^e with amax * 2^e in [2^13, 2^14) (|e| <= 60; 1 for amax = 0): the power-of-two scaling of the fp16 pass
__device__ __forceinline__ float pow2_scale(float amax) {
    if (!(amax > 0.f)) return 1.f;
    const int e = (int)((__float_as_uint(amax) >> 23) & 0xffu) - 127;
    const int sft = max(-60, min(60, 13 - e));
    return __uint_as_float((uint32_t)(127 + sft) << 23);
}

template <int STRIDE>
__device__ __forceinline__ uint32_t lane_xor(uint32_t v) {
    if constexpr (STRIDE == 1) return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0xB1, 0xf, 0xf, true);   // quad_perm [1,0,3,2]
    else if constexpr (STRIDE == 2) return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x4E, 0xf, 0xf, true);   // [2,3,0,1]
    else if constexpr (STRIDE == 4) {   // half_mirror (i ^ 7) then quad reverse (i ^ 3)
        const int t = __builtin_amdgcn_update_dpp(0, (int)v, 0x141, 0xf, 0xf, true);
        return (uint32_t)__builtin_amdgcn_update_dpp(0, t, 0x1B, 0xf, 0xf, true);
    } else if constexpr (STRIDE == 8) return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x128, 0xf, 0xf, true);   // row_ror:8
    else if constexpr (STRIDE == 16) return (uint32_t)__builtin_amdgcn_ds_swizzle((int)v, 0x401F);   // xor 16 inside each 32 lanes
    else return (uint32_t)__shfl_xor((int)v, 32, 64);
}

template <int SIZE, int STRIDE>
__device__ __forceinline__ void cmpx(uint32_t& hi, uint32_t& lo, int lane) {
    const uint32_t ohi = lane_xor<STRIDE>(hi), olo = lane_xor<STRIDE>(lo);
    const bool other_gt = (ohi > hi) || (ohi == hi && olo > lo);
    const bool upper = (lane & STRIDE) != 0;                 // I am the higher lane of the pair
    const bool desc = (lane & SIZE) == 0;                    // this block sorts descending
    const bool take_max = (upper != desc);                   // lower lane of a descending block keeps the max
    const bool take_other = (take_max == other_gt);
    hi = take_other ? ohi : hi;
    lo = take_other ? olo : lo;
}

// descending bitonic sort of one 64-bit key per lane across the wave (keys are distinct)
__device__ __forceinline__ uint64_t wave_sort_desc(uint64_t key, int lane) {
    uint32_t hi = (uint32_t)(key >> 32), lo = (uint32_t)key;
    cmpx<2, 1>(hi, lo, lane);
    cmpx<4, 2>(hi, lo, lane); cmpx<4, 1>(hi, lo, lane);
    cmpx<8, 4>(hi, lo, lane); cmpx<8, 2>(hi, lo, lane); cmpx<8, 1>(hi, lo, lane);
    cmpx<16, 8>(hi, lo, lane); cmpx<16, 4>(hi, lo, lane); cmpx<16, 2>(hi, lo, lane); cmpx<16, 1>(hi, lo, lane);
    cmpx<32, 16>(hi, lo, lane); cmpx<32, 8>(hi, lo, lane); cmpx<32, 4>(hi, lo, lane); cmpx<32, 2>(hi, lo, lane);
    cmpx<32, 1>(hi, lo, lane);
    cmpx<64, 32>(hi, lo, lane); cmpx<64, 16>(hi, lo, lane); cmpx<64, 8>(hi, lo, lane); cmpx<64, 4>(hi, lo, lane);
    cmpx<64, 2>(hi, lo, lane); cmpx<64, 1>(hi, lo, lane);
    return ((uint64_t)hi << 32) | lo;
}

// the first 15 stages of the network: lanes 0-31 end up sorted descending, lanes 32-63 ASCENDING (two independent
// 32-key sorts, no exchange across the halves)
__device__ __forceinline__ uint64_t wave_sort_halves(uint64_t key, int lane) {
    uint32_t hi = (uint32_t)(key >> 32), lo = (uint32_t)key;
    cmpx<2, 1>(hi, lo, lane);
    cmpx<4, 2>(hi, lo, lane); cmpx<4, 1>(hi, lo, lane);
    cmpx<8, 4>(hi, lo, lane); cmpx<8, 2>(hi, lo, lane); cmpx<8, 1>(hi, lo, lane);
    cmpx<16, 8>(hi, lo, lane); cmpx<16, 4>(hi, lo, lane); cmpx<16, 2>(hi, lo, lane); cmpx<16, 1>(hi, lo, lane);
    cmpx<32, 16>(hi, lo, lane); cmpx<32, 8>(hi, lo, lane); cmpx<32, 4>(hi, lo, lane); cmpx<32, 2>(hi, lo, lane);
    cmpx<32, 1>(hi, lo, lane);
    return ((uint64_t)hi << 32) | lo;
}


typedef unsigned short u16x2 __attribute__((ext_vector_type(2)));

// wave-wide OR, returned to every lane (uniform)
template <int CTRL, int ROW_MASK = 0xf>
__device__ __forceinline__ uint32_t dpp_or(uint32_t v) {
    return v | (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, CTRL, ROW_MASK, 0xf, false);
}
__device__ __forceinline__ uint32_t wave_or(uint32_t v) {
    v = dpp_or<0xb1>(v); v = dpp_or<0x4e>(v); v = dpp_or<0x124>(v); v = dpp_or<0x128>(v);
    v = dpp_or<0x142, 0xa>(v); v = dpp_or<0x143, 0xc>(v);
    return (uint32_t)__builtin_amdgcn_readlane((int)v, 63);
}

// how many of the two 15-bit keys packed in xo (each with bit 15 set on top) reach cand: (key | 0x8000) - cand keeps bit 15
// exactly when key >= cand and never borrows from the neighbouring field; the answers are added up as two 16-bit counters
__device__ __forceinline__ u16x2 count_ge2(uint32_t xo, uint32_t cand2, u16x2 acc) {
    return acc + (__builtin_bit_cast(u16x2, xo - cand2) >> (unsigned short)15);
}


// A compiler hole, ROCm 7.2 / gfx950 (found in round 5; tests/test_gpu_topk.py test_exact_arithmetic_lists caught it): the wait states
// between a 16-pass MFMA and the first VALU read of its result (19 on this chip; the hardware does NOT interlock them) are counted by
// hipcc along the LAYOUT of the code, not along the control flow.  On a workgroup's LAST tile the staging code between the chain and
// the filter is skipped by two scalar branches, the `s_nop 2` hipcc had placed in front of `v_accvgpr_read a15` is all that is left,
// and the lane reads register 15 -- the last the matrix pipe writes -- one MFMA early: scores of tile rows 27 and 31 came out short
// of their last two products, depending on how the rest of the file happened to be laid out.  The wait goes in by hand, right behind
// the chain: 20 states of ~6,400 per tile.
// (`acc` is an operand of the statement: it cannot move above the chain or below the first read; where the accumulators live in
// AGPRs hipcc copies them out in front of it -- in line with the chain, where its own count is right)
__device__ __forceinline__ void mfma_result_guard(f32x16& acc) {            // behind a chain of 16-pass MFMAs (v_mfma_f32_32x32x2_f32)
    asm volatile("s_nop 15\n\ts_nop 3" : "+v"(acc));
}
__device__ __forceinline__ void mfma_result_guard_8pass(f32x16& acc) {      // behind 8-pass MFMAs (v_mfma_f32_32x32x16_f16): 11 states
    asm volatile("s_nop 10" : "+v"(acc));
}

// ---- the fp32 MFMA tile of K4 and K8: 32 items x 32 users x k -----------------------------------------------------------------------
// KHP MFMAs on top of `acc`: arow = the lane's half of its item's LDS row (ScoreTile: [h * KHP + kk]), breg = the lane's half of its
// user's row.  The guard comes with the chain; a caller whose accumulator runs over several groups (the slabs of a wide row) asks for it
// behind the last one only.
template <int KHP>
__device__ __forceinline__ void mfma_f32_group(f32x16& acc, const float* arow, const float* breg, bool guard = true) {
#pragma unroll
    for (int kk = 0; kk < KHP; kk += 4) {
        const float4 a = *reinterpret_cast<const float4*>(arow + kk);
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.x, breg[kk + 0], acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.y, breg[kk + 1], acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.z, breg[kk + 2], acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.w, breg[kk + 3], acc, 0, 0, 0);
    }
    if (guard) mfma_result_guard(acc);
}

// The item tiles of a workgroup of at most NT threads (`nthreads` of them at run time), double-buffered in LDS: tile [2][32][KP] with
// half hh of an item's factors at [hh * KHP + kk], zero beyond the half, and the tile's biases tbias [2][32].  Tile t goes global ->
// registers (stage_load, issued early) -> LDS (stage_store, written after the MFMA chain).  float4 path when every k-half starts
// 16-byte aligned (k % 8 == 0); scalar path otherwise.
template <int KHP, int NT>
struct ScoreTile {
    static constexpr int KP = 2 * KHP + 4;                       // padded LDS row (floats): conflict-free b128 reads
    static constexpr int NC = (32 * 2 * KHP / 4 + NT - 1) / NT;  // float4 chunks per thread
    float* tile;
    float* tbias;
    const float* Vt;
    const float* bias;
    int n_cols, k, KH, tid, nthreads;
    bool vec;                                                    // then KH % 4 == 0: no chunk straddles the halves
    int src_off[NC], dst_off[NC], item_of[NC];                   // per-chunk offsets, fixed for the whole kernel
    float4 stg[NC];
    float stg_bias;

    __device__ __forceinline__ ScoreTile(float* tile_, float* tbias_, const float* Vt_, const float* bias_, int n_cols_, int k_, int nthreads_)
        : tile(tile_), tbias(tbias_), Vt(Vt_), bias(bias_), n_cols(n_cols_), k(k_), KH((k_ + 1) >> 1), tid(threadIdx.x),
          nthreads(nthreads_), vec((k_ & 7) == 0), stg_bias(0.f) {
        const int k4 = k >> 2;
#pragma unroll
        for (int q = 0; q < NC; ++q) {
            const int c = tid + q * nthreads;
            const int item = vec ? c / k4 : 0, e = vec ? (c % k4) * 4 : 0;
            const bool live = vec && c < 32 * k4;
            src_off[q] = live ? item * k + e : -1;
            dst_off[q] = item * KP + (e / KH) * KHP + (e % KH);
            item_of[q] = item;
        }
    }

    // B operand: half h of the factor row of this lane's user (k-range [h * KH, min(k, (h + 1) * KH))), resident for the whole kernel
    static __device__ __forceinline__ void load_user(float (&breg)[KHP], const float* U, const int32_t* uidx,
                                                     int row, bool user_ok, int k, int h) {
        const int KH = (k + 1) >> 1;
        const int urow = user_ok ? (uidx ? uidx[row] : row) : 0;
        const float* up = U + (size_t)urow * k + h * KH;
#pragma unroll
        for (int kk = 0; kk < KHP; ++kk) {
            const int e = h * KH + kk;
            breg[kk] = (user_ok && kk < KH && e < k) ? up[kk] : 0.f;
        }
    }

    __device__ __forceinline__ void stage_load(int t) {          // tile t -> registers
        if (vec) {
#pragma unroll
            for (int q = 0; q < NC; ++q) {
                stg[q] = make_float4(0.f, 0.f, 0.f, 0.f);
                if (src_off[q] >= 0 && t * 32 + item_of[q] < n_cols)
                    stg[q] = *reinterpret_cast<const float4*>(Vt + (size_t)t * 32 * k + src_off[q]);
            }
        }
        if (tid < 32) {
            const int col = t * 32 + tid;
            stg_bias = (bias && col < n_cols) ? bias[col] : 0.f;
        }
    }

    __device__ __forceinline__ void stage_store(int t, int buf) {   // registers (or, scalar path, global) -> LDS
        float* dst = tile + buf * 32 * KP;
        if (vec) {
#pragma unroll
            for (int q = 0; q < NC; ++q)
                if (src_off[q] >= 0) *reinterpret_cast<float4*>(dst + dst_off[q]) = stg[q];
        } else {
            for (int c = tid; c < 32 * 2 * KHP; c += nthreads) {
                const int item = c / (2 * KHP), p = c % (2 * KHP);
                const int hh = p / KHP, kk = p % KHP;
                const int e = hh * KH + kk, col = t * 32 + item;
                float v = 0.f;
                if (kk < KH && e < k && col < n_cols) v = Vt[(size_t)col * k + e];
                dst[item * KP + p] = v;
            }
        }
        if (tid < 32) tbias[buf * 32 + tid] = stg_bias;
    }

    __device__ __forceinline__ void zero_padding() {             // what the vector path never writes
        for (int c = tid; c < 2 * 32 * KP; c += nthreads) tile[c] = 0.f;
    }

    __device__ __forceinline__ const float* arow(int buf, int ul, int h) const { return tile + buf * 32 * KP + ul * KP + h * KHP; }
};


typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef _Float16 f16x4 __attribute__((ext_vector_type(4)));

// ---- the fp16 bound-and-refine kernels (csrc/topk.hip score_topk_bf16_kernel, csrc/topk_refine.hip): what a lane sets up once ---------
// B operand: lane (user ul, k-group h) holds elements 16s + 8h .. +7 of its user's row, scaled by the user's own power of two su to
// fp16 (hreg); the item factors are scaled by sv, scores live in units of bscale = su * sv.  `margin`: how far the approximate score
// may be from the exact fp32 score in those units -- what makes the filter's lists supersets of the exact top K; derived in
// csrc/topk.hip above score_topk_bf16_kernel.  extra: bits of [0] max |v_i|, [1] max |bias|, [2] max |V element|.
// `sane`: the margin means what it says for this user.  It does not when the row or the item table holds a NaN or an infinity, when
// |u| * max |v_i| + max |bias| comes near fp32's range (a score, or the bound the item ranges share, could overflow), or when
// pow2_scale had to clamp (|13 - e| > 60: the scaled factors leave fp16's range, and sum u^2 its own -- it overflows above 2^64 and
// loses the reach term below 2^-63; kept to largest elements in [2^-47, 2^60)), or when max |bias| in the user's scaled units leaves
// fp32's range.  A user that is not sane flags its user block, which the fp32 kernel then ranks on its own (the list-overflow path,
// without the thresholds this pass published: csrc/topk.hip redo_plan), so NaN and infinite scores are ranked by the fp32 kernel alone.
// The user still goes through the fp16 pass, like its neighbours -- `sane` feeds the block flag and nothing inside the tile loop --
// and what the pass makes of it (lists of valid columns, thresholds of its own row) is thrown away with the block.
// topk_bounds_kernel reports a non-finite item table or bias as max |v_i| = +inf: then no user is sane.
__device__ __forceinline__ bool pow2_scale_exact(float amax) {  // amax = 0, or pow2_scale(amax) is the unclamped power of two
    const int e = (int)((__float_as_uint(amax) >> 23) & 0xffu) - 127;
    return amax == 0.f || (e >= -47 && e < 60);
}

template <int KS>
__device__ __forceinline__ void refine_prologue(const float* up, int k, bool user_ok, int h, const uint32_t* extra,
                                                f16x8 (&hreg)[KS], float& margin, float& bscale, float& sv, bool& sane) {
    constexpr int KPAD = KS * 16;
    float uv[KS][8];
    if ((k & 3) == 0) {                                          // two 16-byte loads per 16-wide k step, all issued before use
#pragma unroll
        for (int s = 0; s < KS; ++s)
#pragma unroll
            for (int q = 0; q < 2; ++q) {
                const int e = 16 * s + 8 * h + 4 * q;
                float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
                if (user_ok && e < k) v = *reinterpret_cast<const float4*>(up + e);
                uv[s][4 * q + 0] = v.x; uv[s][4 * q + 1] = v.y; uv[s][4 * q + 2] = v.z; uv[s][4 * q + 3] = v.w;
            }
    } else {
#pragma unroll
        for (int s = 0; s < KS; ++s)
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                const int e = 16 * s + 8 * h + i;
                const float v = up[min(e, k - 1)];
                uv[s][i] = (user_ok && e < k) ? v : 0.f;
            }
    }
    float nu = 0.f, amax = 0.f;
#pragma unroll
    for (int s = 0; s < KS; ++s)
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            nu = fmaf(uv[s][i], uv[s][i], nu);
            amax = fmaxf(amax, fabsf(uv[s][i]));
        }
    nu += __shfl_xor(nu, 32, 64);                                // the other k-group of the same user
    amax = fmaxf(amax, __shfl_xor(amax, 32, 64));
    const float su = pow2_scale(amax);
    sv = pow2_scale(__uint_as_float(extra[2]));
    bscale = su * sv;
#pragma unroll
    for (int s = 0; s < KS; ++s)
#pragma unroll
        for (int i = 0; i < 8; ++i) hreg[s][i] = (_Float16)(uv[s][i] * su);
    const float reach = sqrtf(nu) * 1.001f * __uint_as_float(extra[0]);      // >= |u| * max |v_i|
    margin = (fmaf(1.05f * 0.0009765625f, reach, 3.8146973e-6f * (reach + __uint_as_float(extra[1]))) + 7.7e-34f) * bscale +
             2.01f * (float)KPAD;
    // (a NaN in the row: nu and the margin are NaN, fmaxf left it out of amax; an infinity: amax)
    sane = reach + __uint_as_float(extra[1]) < 1e38f && margin < 1e38f && __uint_as_float(extra[1]) * bscale < 1e38f &&
           pow2_scale_exact(amax) && pow2_scale_exact(__uint_as_float(extra[2]));
}

// acc <- fma(bias, bscale, acc) in the accumulator's own registers: the biases of a tile in the user's scaled units
__device__ __forceinline__ void add_scaled_bias_inplace(f32x16& acc, const float* tbias, int h, float bscale) {
#pragma unroll
    for (int g = 0; g < 4; ++g) {
        const float4 bq = *reinterpret_cast<const float4*>(tbias + 8 * g + 4 * h);
        acc[4 * g + 0] = fmaf(bq.x, bscale, acc[4 * g + 0]); acc[4 * g + 1] = fmaf(bq.y, bscale, acc[4 * g + 1]);
        acc[4 * g + 2] = fmaf(bq.z, bscale, acc[4 * g + 2]); acc[4 * g + 3] = fmaf(bq.w, bscale, acc[4 * g + 3]);
    }
}


template <int KS>
__device__ __forceinline__ int tile_swizzle(int r) {             // KS in {1, 2, 4, 8}: CR = 2 * KS chunks per row, 16 / CR rows per 256 B
    constexpr int CR = 2 * KS;
    return (r / (16 / CR)) & (CR - 1);
}


}  // namespace tkr
