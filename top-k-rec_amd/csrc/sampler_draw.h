// The (u, i, j) draw of K1, shared by the per-batch planner (sampler.hip) and the grid-wide one (planner_big.hip); its (i, j) part for a
// fixed user is the draw of K9 (foldin.hip), its negative part (draw_negative) also that of K10's positive role (foldin_items.hip).
// Replaces BPR._uniform_user_sampling (single/bpr.py:155-165); stream definition in oracle/plan_np.py.
#pragma once
#include "tkr_common.h"

namespace tkr {

constexpr int kMaxRounds = 64;   // oracle/plan_np.py MAX_ROUNDS

// is `item` among cols_sorted[lo, hi) (ascending)?  A 4-ary search: three pivots per step, loaded together -- the draw of a triplet is
// a chain of dependent loads (user -> row bounds -> positive; then this search for every candidate negative), and a binary search is
// log2(degree) trips where this is log4 (a degree of 36: 3 trips instead of 6; the draw is 4.9 us of the 17 us phase A of a batch).
// Wider is NOT faster (round 5, measured inside the planner prologue of csrc/bpr_own.hip: sixteen segments per step + a window of 32
// at the end = 2 trips and 47 loads per candidate took 9.0 us where this takes 5.6): a load whose 64 lanes hit 64 different lines
// occupies the CU's L1 for ~64 cycles whether or not anybody waits for it, so the cost is trips x ~0.5 us + loads x ~0.14 us.
__device__ __forceinline__ bool is_member(const int32_t* __restrict__ cols_sorted, int lo, int hi, int item) {
    int a = lo, b = hi;                              // if present, item sits in [a, b)
    while (b - a > 3) {
        const int q = (b - a) >> 2;
        const int m1 = a + q, m2 = a + 2 * q, m3 = a + 3 * q;
        const int v1 = cols_sorted[m1], v2 = cols_sorted[m2], v3 = cols_sorted[m3];
        if (item == v1 || item == v2 || item == v3) return true;
        if (item < v1) b = m1;
        else if (item < v2) { a = m1 + 1; b = m2; }
        else if (item < v3) { a = m2 + 1; b = m3; }
        else a = m3 + 1;
    }
    const int last = hi > lo ? hi - 1 : lo;
    const int c0 = cols_sorted[min(a, last)], c1 = cols_sorted[min(a + 1, last)], c2 = cols_sorted[min(a + 2, last)];
    return (a < b && c0 == item) || (a + 1 < b && c1 == item) || (a + 2 < b && c2 == item);
}

// A uniform draw over [0, n) that `rejected` does not refuse: the first of the two candidates a round (words x, y, then z, w) of rounds
// 1 .. kMaxRounds of the counter (c0, c1, round, C3) that passes, then a cyclic scan of at most n from the last candidate.
// -> false: nothing in [0, n) passes (`out` is then a refused candidate).
// C3 names the stream: 0 = K1 (training), 1 = K9 (fold-in of users, csrc/foldin.hip), 2 = K10 (fold-in of items,
// csrc/foldin_items.hip) -- disjoint under one seed.
template <uint32_t C3, class Rejected>
__device__ __forceinline__ bool draw_accepted(uint32_t n, uint32_t c0, uint32_t c1, uint32_t k0, uint32_t k1, Rejected rejected, int& out) {
    int cand = 0;
    bool found = false;
    for (uint32_t r = 1; r <= (uint32_t)kMaxRounds && !found; ++r) {
        const u32x4 w = philox4x32_10(c0, c1, r, C3, k0, k1);
        cand = (int)mulhi64(w.x, w.y, n);
        if (!rejected(cand)) { found = true; break; }
        cand = (int)mulhi64(w.z, w.w, n);
        if (!rejected(cand)) { found = true; break; }
    }
    if (!found) {   // cyclic scan fallback (user rated almost everything)
        uint32_t s = 0;
        for (; s < n && rejected(cand); ++s)
            cand = (cand + 1 == (int)n) ? 0 : cand + 1;
        found = s < n;
    }
    out = cand;
    return found;
}

// The negative of a draw for a user whose row is [lo, hi) of cols_sorted (hi > lo): uniform over the columns not in the row.
// -> false: the row covers the whole catalogue.  Shared by K1, K9 and K10's positive role.
template <uint32_t C3>
__device__ __forceinline__ bool draw_negative(const int32_t* __restrict__ cols_sorted, int lo, int hi, uint32_t n_items, uint32_t c0,
                                              uint32_t c1, uint32_t k0, uint32_t k1, int& j) {
    return draw_accepted<C3>(n_items, c0, c1, k0, k1, [&](int c) { return is_member(cols_sorted, lo, hi, c); }, j);
}

// The (i, j) part of a draw for a user whose row is [lo, hi) of pos_cols / cols_sorted (hi > lo, and the row does not cover the whole
// catalogue unless the caller accepts the candidate coming back unchanged): the positive from words z, w of the round-0 block `w0`,
// the negative by draw_negative on the same counter.
template <uint32_t C3>
__device__ __forceinline__ void draw_pair(const int32_t* __restrict__ pos_cols, const int32_t* __restrict__ cols_sorted, int lo, int hi,
                                          uint32_t n_items, u32x4 w0, uint32_t c0, uint32_t c1, uint32_t k0, uint32_t k1, int& i, int& j) {
    i = pos_cols[lo + (int)mulhi64(w0.z, w0.w, (uint32_t)(hi - lo))];
    draw_negative<C3>(cols_sorted, lo, hi, n_items, c0, c1, k0, k1, j);
}

__device__ __forceinline__ void draw_triplet(const int32_t* __restrict__ tr_users, uint32_t n_tr,
                                             const int32_t* __restrict__ row_ptr,
                                             const int32_t* __restrict__ pos_cols,
                                             const int32_t* __restrict__ cols_sorted, uint32_t n_items,
                                             uint32_t k0, uint32_t k1, uint64_t g, int& u, int& i, int& j) {
    const uint32_t c0 = (uint32_t)g, c1 = (uint32_t)(g >> 32);
    const u32x4 w = philox4x32_10(c0, c1, 0u, 0u, k0, k1);
    u = tr_users[mulhi64(w.x, w.y, n_tr)];
    draw_pair<0u>(pos_cols, cols_sorted, row_ptr[u], row_ptr[u + 1], n_items, w, c0, c1, k0, k1, i, j);
}

}  // namespace tkr
