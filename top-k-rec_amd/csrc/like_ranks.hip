// K8 -- filtered rank of every liked test column: the one integer per like from which AUC, NDCG, MRR, MAP and the reference's
// accuracy@k (evaluate.py:96-112, any step / total) all follow.
//
//   rank_out[e] = #{unrated columns c != l ahead of l = like_cols[e] in the canonical order of its row}
//               = #{c unmasked : key(c) > key(l)},   key = rank_bits(score) << 32 | column
// (K4's canonical order over every fp32 value, include/tkr.h: descending score, every NaN one score above +inf, ties -> higher
// column first; -0.0 ties with 0.0), or -1 when l itself is rated: the reference walk never
// reaches a rated like.  The scores are K4's mode-1 bits (fp32 MFMA chain, fl(acc + bias)): exact_score for the likes, the
// tile loop of score_topk_kernel for the catalogue -- same products, counting in place of selection.
//
// Three launches:
//   like_keys_kernel   a wave per row: the key of every like (exact_score), rank_out <- 0 / -1
//   like_sort_kernel   a wave per row: the row's keys in ascending order (rank sort: position = keys below; rows of any length)
//   like_ranks_kernel  W x 32 users per workgroup as the B operand of v_mfma_f32_32x32x2_f32, 32-item tiles double-buffered in
//                      LDS.  The user block's sorted keys t_0 < t_1 < ... sit in LDS beside one counter per key.  A column with
//                      key x is ahead of exactly the likes q < m, m = #{t_q < x}: a lane finds m for its 16 scores of the tile
//                      by 16 interleaved binary searches (the step loop outside, so 16 LDS reads are in flight) and bumps
//                      counter[m - 1]; m = 0 (masked, tail, behind every like of the user) bumps nothing.  At the end
//                      rank(q) = sum of counter[j], j >= q: one suffix walk per user, added to rank_out with integer atomics
//                      -- item ranges of one user block (the grid's y dimension, so the CUs fill in whole rounds) just add up.
//   LDS: tiles 2 x 32 x (2 KHP + 4) x 4 B (66.6 KB at k = 256) + 64 biases + kLikeCap x (8 B key + 4 B counter) = 72 KB:
//   139 KB at k = 256, 106 KB at k = 128.  A user block with more than kLikeCap likes is counted in chunks of the sorted key
//   array (cut anywhere, inside a user's list too: the likes of a chunk are a contiguous piece of every user's sorted list, and
//   m counted against that piece ranks exactly its likes); each chunk runs the tile loop again.
// k > 256: like_ranks_wide_kernel, a wave per row with a lane per column on exact_score.
#include <algorithm>

#include "tkr_common.h"
#include "topk_parts.h"
#include "../../include/tkr.h"

namespace tkr {

constexpr int kLikeCap = 6144;                    // likes of a user block resident in LDS at a time
constexpr uint32_t kNoRank = 0xffffffffu;         // high word of the key of a like that gets no rank (rated / not a column)
constexpr int kLikeMaxSplits = 64;

struct LikeWs {                                   // carve of the caller's workspace for `cap` likes
    uint64_t* ukey;                               // [cap] keys in CSR order
    uint64_t* skey;                               // [cap] keys of every row ascending
    int32_t* sperm;                               // [cap] index inside its row of the like behind skey[i]
    int64_t cap;
};

// v - origin clamped into [0, n]: where a CSR bound falls inside a chunk of n keys
__device__ __forceinline__ int chunk_pos(int64_t v, int64_t origin, int n) {
    const int64_t d = v - origin;
    return d < 0 ? 0 : (d > n ? n : (int)d);
}

__device__ __forceinline__ uint64_t like_key(float s, int col) { return ((uint64_t)rank_bits(s) << 32) | (uint32_t)col; }

// the CSR is usable: starts at 0 and fits the workspace (a workspace sized for fewer likes: every rank_out <- -2, nothing else runs)
__device__ __forceinline__ bool like_csr_ok(const int64_t* __restrict__ like_ptr, int n_rows, int64_t cap) {
    return like_ptr[0] == 0 && like_ptr[n_rows] <= cap;
}

__global__ __launch_bounds__(256) void like_keys_kernel(const float* __restrict__ U, const int32_t* __restrict__ uidx, int n_rows,
                                                        const float* __restrict__ Vt, const float* __restrict__ bias, int n_cols, int k,
                                                        const uint32_t* __restrict__ mask, int pitch, const int64_t* __restrict__ like_ptr,
                                                        const int32_t* __restrict__ like_cols, int32_t* __restrict__ rank_out, LikeWs ws) {
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (row >= n_rows) return;
    const int64_t e0 = like_ptr[row], e1 = like_ptr[row + 1];
    if (!like_csr_ok(like_ptr, n_rows, ws.cap)) {
        if (like_ptr[0] == 0)
            for (int64_t e = e0 + lane; e < e1; e += 64) rank_out[e] = -2;
        return;
    }
    const float* up = U + (size_t)(uidx ? uidx[row] : row) * k;
    for (int64_t e = e0 + lane; e < e1; e += 64) {
        const int c = like_cols[e];
        bool ranked = c >= 0 && c < n_cols;
        if (ranked && mask) ranked = !col_masked(mask, pitch, row, c);
        ws.ukey[e] = ranked ? like_key(exact_score(up, Vt + (size_t)c * k, k, bias, c), c) : (((uint64_t)kNoRank << 32) | (uint32_t)c);
        rank_out[e] = ranked ? 0 : -1;
    }
}

__global__ __launch_bounds__(256) void like_sort_kernel(int n_rows, const int64_t* __restrict__ like_ptr, LikeWs ws) {
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (row >= n_rows || !like_csr_ok(like_ptr, n_rows, ws.cap)) return;
    const int64_t e0 = like_ptr[row];
    const int P = (int)(like_ptr[row + 1] - e0);
    for (int q = lane; q < P; q += 64) {
        const uint64_t key = ws.ukey[e0 + q];
        int pos = 0;                                             // equal keys (a column listed twice) keep their order: always a permutation
        for (int j = 0; j < P; ++j) {
            const uint64_t o = ws.ukey[e0 + j];
            pos += (o < key || (o == key && j < q)) ? 1 : 0;
        }
        ws.skey[e0 + pos] = key;
        ws.sperm[e0 + pos] = q;
    }
}

template <int KHP>
constexpr int like_waves() { return KHP > 64 ? 4 : kTopkMaxWaves; }

template <int KHP>
__global__ __launch_bounds__((like_waves<KHP>() * TKR_WAVE)) void like_ranks_kernel(
    const float* __restrict__ U, const int32_t* __restrict__ uidx, int n_rows, const float* __restrict__ Vt,
    const float* __restrict__ bias, int n_cols, int k, const uint32_t* __restrict__ mask, int mask_pitch,
    const int64_t* __restrict__ like_ptr, int32_t* __restrict__ rank_out, LikeWs ws, int tiles_per_split) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    constexpr int WAVES = like_waves<KHP>();
    constexpr int users = WAVES * 32, NT_ = WAVES * 64;
    using Tile = ScoreTile<KHP, NT_>;
    constexpr int KP = Tile::KP;
    float* tile = reinterpret_cast<float*>(smem_raw);            // [2][32][KP]
    float* tbias = tile + 2 * 32 * KP;                           // [2][32]
    uint64_t* keys = reinterpret_cast<uint64_t*>(tbias + 64);    // [kLikeCap]
    uint32_t* cnt = reinterpret_cast<uint32_t*>(keys + kLikeCap);   // [kLikeCap]

    if (!like_csr_ok(like_ptr, n_rows, ws.cap)) return;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int ul = lane & 31, h = lane >> 5;
    const int block = blockIdx.x;
    const int row = block * users + wave * 32 + ul;
    const bool user_ok = row < n_rows;
    const int64_t seg0 = like_ptr[block * users], seg1 = like_ptr[min(n_rows, (block + 1) * users)];
    if (seg1 <= seg0) return;                                    // no likes in this user block (workgroup-uniform)
    const int64_t my0 = user_ok ? like_ptr[row] : seg1, my1 = user_ok ? like_ptr[row + 1] : seg1;

    float breg[KHP];
    Tile::load_user(breg, U, uidx, row, user_ok, k, h);
    const int n_tiles_all = (n_cols + 31) >> 5;
    const int t_begin = blockIdx.y * tiles_per_split;
    const int n_tiles = min(n_tiles_all, t_begin + tiles_per_split);
    if (t_begin >= n_tiles) return;

    Tile tl(tile, tbias, Vt, bias, n_cols, k, NT_);
    if (tl.vec) tl.zero_padding();
    const uint32_t tail_mask = (n_cols & 31) ? (0xffffffffu << (n_cols & 31)) : 0u;

    for (int64_t cs = seg0; cs < seg1; cs += kLikeCap) {         // chunks of the block's sorted keys (one, as a rule)
        const int n_chunk = chunk_pos(seg1, cs, kLikeCap);
        __syncthreads();                                         // the previous chunk's walk is done with keys / cnt
        for (int i = tid; i < n_chunk; i += NT_) { keys[i] = ws.skey[cs + i]; cnt[i] = 0u; }
        // this lane's user: its piece [base, base + P) of the chunk
        const int base = chunk_pos(my0, cs, n_chunk);
        const int P = chunk_pos(my1, cs, n_chunk) - base;
        int pmax = P;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) pmax = max(pmax, __shfl_xor(pmax, o, 64));
        const bool wave_counts = pmax > 0;                       // wave-uniform: no like of these 32 users in this chunk
        const int top = __builtin_amdgcn_readfirstlane(wave_counts ? 1 << (31 - __clz(pmax)) : 0);
        tl.stage_load(t_begin);
        tl.stage_store(t_begin, t_begin & 1);
        __syncthreads();
        const uint64_t lowest = P > 0 ? keys[base] : ~0ull;
        if (t_begin + 1 < n_tiles) tl.stage_load(t_begin + 1);

        for (int t = t_begin; t < n_tiles; ++t) {
            const int buf = t & 1;
            uint32_t maskw = (mask && user_ok) ? mask[(size_t)t * mask_pitch + row] : 0u;
            f32x16 acc = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
            if (wave_counts) {
                // ---- 32 items x 32 users x k: exact fp32 MFMA
                mfma_f32_group<KHP>(acc, tl.arow(buf, ul, h), breg);
            }
            if (t + 1 < n_tiles) tl.stage_store(t + 1, buf ^ 1);
            if (t + 2 < n_tiles) tl.stage_load(t + 2);
            if (wave_counts) {
                // ---- epilogue: register r of lane (ul, h) = item (r&3) + 8*(r>>2) + 4h of the tile, user ul of the wave
                if (!user_ok) maskw = 0xffffffffu;
                if (t == n_tiles_all - 1) maskw |= tail_mask;
                const uint32_t mh = maskw >> (4 * h);
                const float* tb = tbias + buf * 32;
                uint64_t key[16];
                bool any = false;
#pragma unroll
                for (int g = 0; g < 4; ++g) {
                    const float4 bq = *reinterpret_cast<const float4*>(tb + 8 * g + 4 * h);
                    const float bb[4] = {bq.x, bq.y, bq.z, bq.w};
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        const int r = 4 * g + j;
                        const float s = chain_finish(acc[r], bb[j]);
                        const uint64_t x = like_key(s, t * 32 + 8 * g + 4 * h + j);
                        key[r] = ((mh >> (8 * g + j)) & 1u) ? 0ull : x;      // 0: below every like
                        any |= key[r] > lowest;
                    }
                }
                if (__ballot(any) != 0) {
                    int pos[16];
#pragma unroll
                    for (int r = 0; r < 16; ++r) pos[r] = 0;
#pragma unroll 1
                    for (int s = top; s > 0; s >>= 1) {          // pos = #{t_q < key}: 16 searches side by side
                        uint64_t tv[16];
#pragma unroll
                        for (int r = 0; r < 16; ++r) tv[r] = keys[min(base + pos[r] + s - 1, kLikeCap - 1)];
#pragma unroll
                        for (int r = 0; r < 16; ++r) pos[r] += (pos[r] + s <= P && tv[r] < key[r]) ? s : 0;
                    }
#pragma unroll
                    for (int r = 0; r < 16; ++r)
                        if (pos[r] > 0) atomicAdd(&cnt[base + pos[r] - 1], 1u);
                }
            }
            __syncthreads();                                     // tile t+1 staged; buffer `buf` may be overwritten next
        }

        // ---- rank(q) = sum of the counters from q up; one user per thread, added to what the other item ranges found
        if (tid < users) {
            const int r2 = block * users + tid;
            if (r2 < n_rows) {
                const int64_t l0 = like_ptr[r2], l1 = like_ptr[r2 + 1];
                const int a = chunk_pos(l0, cs, n_chunk), b = chunk_pos(l1, cs, n_chunk);
                uint32_t run = 0;
                for (int j = b - 1; j >= a; --j) {
                    run += cnt[j];
                    if (run && (uint32_t)(keys[j] >> 32) != kNoRank) atomicAdd(&rank_out[l0 + ws.sperm[cs + j]], (int)run);
                }
            }
        }
    }
}

// k > 256: a wave per row, a lane per column, the same chain (exact_score); every batch of 64 columns is compared with each like
// of the row, the wave's count goes to rank_out with one atomic
__global__ __launch_bounds__(256) void like_ranks_wide_kernel(const float* __restrict__ U, const int32_t* __restrict__ uidx, int n_rows,
                                                              const float* __restrict__ Vt, const float* __restrict__ bias, int n_cols,
                                                              int k, const uint32_t* __restrict__ mask, int pitch,
                                                              const int64_t* __restrict__ like_ptr, int32_t* __restrict__ rank_out, LikeWs ws) {
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (row >= n_rows || !like_csr_ok(like_ptr, n_rows, ws.cap)) return;
    const int64_t e0 = like_ptr[row], e1 = like_ptr[row + 1];
    if (e1 <= e0) return;
    const float* up = U + (size_t)(uidx ? uidx[row] : row) * k;
    for (int c0 = 0; c0 < n_cols; c0 += 64) {
        const int c = c0 + lane;
        uint64_t x = 0;                                          // 0: below every like
        if (c < n_cols && !(mask && col_masked(mask, pitch, row, c)))
            x = like_key(exact_score(up, Vt + (size_t)c * k, k, bias, c), c);
        for (int64_t e = e0; e < e1; ++e) {
            const uint64_t tq = ws.ukey[e];
            const int n = __popcll(__ballot(x > tq));
            if (lane == 0 && n && (uint32_t)(tq >> 32) != kNoRank) atomicAdd(&rank_out[e], n);
        }
    }
}

// item ranges per user block: whole rounds of the CUs; a range costs its tiles + a few tile-times of its own (operand and key
// loads, the suffix walk)
static int like_splits(int blocks, int n_tiles, int cus) {
    int best = 1;
    double best_cost = 1e30;
    for (int s = 1; s <= kLikeMaxSplits && s <= n_tiles; ++s) {
        const int tps = (n_tiles + s - 1) / s;
        const int used = (n_tiles + tps - 1) / tps;
        const double rounds = (double)(((size_t)blocks * used + cus - 1) / cus);
        const double cost = rounds * (tps + 6.0);
        if (cost < best_cost - 1e-9) { best_cost = cost; best = used; }
    }
    return best;
}

static int like_cus() {
    static int cus[16] = {0};
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 16) return 256;
    if (cus[dev] == 0) {
        int n = 0;
        cus[dev] = (hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) == hipSuccess && n > 0) ? n : 256;
    }
    return cus[dev];
}

template <int KHP>
static int launch_like_ranks(const float* U, const int32_t* uidx, int n_rows, const float* Vt, const float* bias, int n_cols, int k,
                             const uint32_t* mask, int pitch, const int64_t* like_ptr, int32_t* rank_out, const LikeWs& ws,
                             hipStream_t stream) {
    constexpr int KP = 2 * KHP + 4, users = like_waves<KHP>() * 32;
    const size_t lds = (size_t)(2 * 32 * KP + 64) * 4 + (size_t)kLikeCap * 12;
    static_assert((size_t)(2 * 32 * KP + 64) * 4 + (size_t)kLikeCap * 12 <= 160 * 1024, "LDS of a CU");
    auto kern = like_ranks_kernel<KHP>;
    TKR_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
    const int blocks = (n_rows + users - 1) / users, n_tiles = (n_cols + 31) / 32;
    const int S = like_splits(blocks, n_tiles, like_cus());
    const int tps = (n_tiles + S - 1) / S;
    hipLaunchKernelGGL(kern, dim3(blocks, (n_tiles + tps - 1) / tps), dim3(users * 2), lds, stream, U, uidx, n_rows, Vt, bias, n_cols, k,
                       mask, pitch, like_ptr, rank_out, ws, tps);
    return (int)hipGetLastError();
}

}  // namespace tkr

extern "C" int64_t tkr_like_ranks_workspace_bytes(int32_t n_rows, int32_t n_cols, int32_t k, int64_t n_likes) {
    if (n_rows <= 0 || n_cols <= 0 || k <= 0 || n_likes < 0) return 0;
    return (n_likes + 1) * 20 + 512;                             // two key arrays, the permutation, alignment
}

extern "C" int tkr_like_ranks(const float* U, const int32_t* user_idx, int32_t n_rows, const float* Vt, const float* bias,
                              int32_t n_cols, int32_t k, const uint32_t* mask, int32_t mask_pitch, const int64_t* like_ptr,
                              const int32_t* like_cols, int32_t* rank_out, void* workspace, int64_t workspace_bytes, void* stream_) {
    if (!U || !Vt || !like_ptr || !like_cols || !rank_out || !workspace) return TKR_EINVAL;
    if (n_rows <= 0 || n_cols <= 0 || n_cols >= (1 << 27) || k <= 0) return TKR_EINVAL;
    if (mask && mask_pitch < n_rows) return TKR_EINVAL;
    if (workspace_bytes < tkr_like_ranks_workspace_bytes(n_rows, n_cols, k, 0)) return TKR_EINVAL;
    hipStream_t stream = (hipStream_t)stream_;
    tkr::LikeWs ws;
    unsigned char* p = static_cast<unsigned char*>(workspace);
    const size_t skew = (size_t)(-(intptr_t)p) & 15;             // 16-byte aligned key arrays
    ws.cap = (workspace_bytes - (int64_t)skew - 64) / 20;
    ws.ukey = reinterpret_cast<uint64_t*>(p + skew);
    ws.skey = ws.ukey + ws.cap;
    ws.sperm = reinterpret_cast<int32_t*>(ws.skey + ws.cap);
    const dim3 rows_grid((n_rows + 3) / 4), rows_block(256);
    hipLaunchKernelGGL(tkr::like_keys_kernel, rows_grid, rows_block, 0, stream, U, user_idx, n_rows, Vt, bias, n_cols, k, mask, mask_pitch,
                       like_ptr, like_cols, rank_out, ws);
    TKR_LAUNCH_CHECK();
    if (k > 256) {
        hipLaunchKernelGGL(tkr::like_ranks_wide_kernel, rows_grid, rows_block, 0, stream, U, user_idx, n_rows, Vt, bias, n_cols, k, mask,
                           mask_pitch, like_ptr, rank_out, ws);
        TKR_LAUNCH_CHECK();
        return TKR_OK;
    }
    hipLaunchKernelGGL(tkr::like_sort_kernel, rows_grid, rows_block, 0, stream, n_rows, like_ptr, ws);
    TKR_LAUNCH_CHECK();
    const int kh = (k + 1) / 2;
#define TKR_LIKE_CASE(KHP) \
    if (kh <= KHP) return tkr::launch_like_ranks<KHP>(U, user_idx, n_rows, Vt, bias, n_cols, k, mask, mask_pitch, like_ptr, rank_out, ws, stream);
    TKR_LIKE_CASE(16)
    TKR_LIKE_CASE(32)
    TKR_LIKE_CASE(52)
    TKR_LIKE_CASE(64)
    TKR_LIKE_CASE(100)
    TKR_LIKE_CASE(128)
#undef TKR_LIKE_CASE
    return TKR_EUNSUPPORTED;
}
