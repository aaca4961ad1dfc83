// K10 -- fold-in of items: rows and biases for items that were not a line of `vid` when the model was trained, against FROZEN user
// factors and the frozen rest of the catalogue.  The item side of the fold-in body (K9, csrc/foldin.hip: the user side); the reference can only retrain.
//
// For one new item x, T times, the model's own step (single/bpr.py:81-100) on a batch of P triplets that all carry x -- as the
// positive of a user who likes it (role 1: x_p = b_x - b_j + <u, v_x - v_j>, the gradient of v_x gains -s u + li v_x, that of b_x
// -s + lb b_x, s = sigma(-x_p)) or as the negative of a user who does not (role 0: x_p = b_i - b_x + <u, v_i - v_x>, +s u + lj v_x,
// +s + lb b_x); mode 1: the sign forms of the regularisers.  Sums in the order p = 0 .. P-1, then one RMSProp update of v_x and one
// of b_x (slots from 1.0).  U, V, b are read only (tests/_item_foldin_oracle.py restates it with oracle/ref_np.py bpr_step).
//
// Items are independent: one wave owns an item from the first step to the last, in the body K9 and K10 share (csrc/fold_rows.h:
// fold_kernel in registers to k = 512, fold_wide_kernel in LDS beyond), b_x and its slot in every lane.  This file is the item
// side of it: the argument block, the draw, the rows of a triplet (the user's and the other item's), the formulas, the own bias.
//
// The draw of lane p < P in step t of item x: Philox counter (g lo, g hi, round, 2), g = ((first_row + x) T + t) P + p, key = seed.
//   round 0, word x        the role: 1 iff x < role_thresh[x] (0xffffffff: always 1, 0: never)
//   round 0, word y        not used
//   round 0, words z, w    the pick from a list, mulhi64(z | w << 32, length): role 1 -- the user u among the item's likers;
//                          role 0 -- the positive i in the row of the user the rounds found
//   rounds 1 .. 64         role 1 -- the negative j of u: sampler_draw.h draw_negative, as K1 and K9 (words x, y the first candidate of
//                          a round, z, w the second; then the cyclic scan over the catalogue);  role 0 -- the user u: the same two
//                          candidates a round over [0, n_users) and the same scan, bounded by n_users (draw_accepted), a candidate
//                          refused unless it has a training row and is not a liker of x (is_member on liker_rows)
// A triplet without a legal draw -- role 1 without likers or for a user whose row is the whole catalogue, role 0 when every user with
// a row likes x -- is recorded as (-1, -1, -1) and contributes nothing; a step all of whose triplets are such changes nothing.
// The chain user -> row bounds -> candidate -> membership is one dependent load longer than K9's, whose row bounds are per wave.
#include <math.h>

#include "fold_rows.h"
#include "sampler_draw.h"
#include "../../include/tkr.h"

namespace tkr {

struct ItemFoldArgs {
    const float* U;
    const float* V;
    const float* b;              // nullable: no bias in the score, none learnt
    const int64_t* user_ptr;
    const int32_t* user_cols;
    const int64_t* liker_ptr;
    const int32_t* liker_rows;
    const uint32_t* role_thresh;
    const float* start;          // V0, nullable: zeros
    const float* b0;             // nullable: zeros
    float* out;                  // Vn
    float* bn;
    float* loss;                 // nullable
    int32_t* trip;               // nullable
    int32_t m, n_users, n_items, k, mode, steps, P;
    float li, lj, lb, lr;
    uint32_t k0, k1;
    uint64_t first_row;
};

// the state of item x: its likers, its role threshold, and its own bias b_x with the slot (held by every lane)
struct ItemSide {
    using Args = ItemFoldArgs;
    static constexpr bool kBias = true;
    const int32_t* likers;
    int nl;
    uint32_t thresh;
    bool has_b;
    float b_start, bx, msb = 1.f;

    __device__ ItemSide(const Args& a, int64_t x) {
        const int64_t lo = a.liker_ptr[x];
        likers = a.liker_rows + lo;
        nl = (int)(a.liker_ptr[x + 1] - lo);
        thresh = a.role_thresh[x];
        has_b = a.b != nullptr;
        b_start = a.b0 ? a.b0[x] : 0.f;
        bx = has_b ? b_start : 0.f;
    }
    __device__ int steps(const Args& a) const { return a.steps; }
    // lane p < P holds triplet p as (role, user, other item), recorded as (-1, -1, -1) without a legal draw; lanes >= P hold role -1
    __device__ FoldTriplet draw(const Args& a, int64_t x, int t, int lane) const {
        int role = -1, du = -1, dother = -1;
        if (lane >= a.P) return {-1, 0, 0};
        const uint64_t g = fold_counter(a, x, t, lane);
        const uint32_t c0 = (uint32_t)g, c1 = (uint32_t)(g >> 32);
        const u32x4 w0 = philox4x32_10(c0, c1, 0u, 2u, a.k0, a.k1);
        if (thresh == 0xffffffffu || w0.x < thresh) {
            if (nl > 0) {
                const int u = likers[mulhi64(w0.z, w0.w, (uint32_t)nl)];
                const int64_t lo = a.user_ptr[u];
                const int deg = (int)(a.user_ptr[u + 1] - lo);
                int j = 0;
                bool found = deg < a.n_items;
                if (deg == 0) {                              // nothing to reject against (and no row to search): the first candidate
                    const u32x4 w = philox4x32_10(c0, c1, 1u, 2u, a.k0, a.k1);
                    j = (int)mulhi64(w.x, w.y, (uint32_t)a.n_items);
                } else if (found) {
                    found = draw_negative<2u>(a.user_cols + lo, 0, deg, (uint32_t)a.n_items, c0, c1, a.k0, a.k1, j);
                }
                if (found) { role = 1; du = u; dother = j; }
            }
        } else {
            int cand = 0;
            const bool found = draw_accepted<2u>((uint32_t)a.n_users, c0, c1, a.k0, a.k1, [&](int c) {
                return a.user_ptr[c + 1] <= a.user_ptr[c] || (nl > 0 && is_member(likers, 0, nl, c));
            }, cand);
            if (found) {
                const int64_t lo = a.user_ptr[cand];
                const uint32_t deg = (uint32_t)(a.user_ptr[cand + 1] - lo);
                role = 0;
                du = cand;
                dother = a.user_cols[lo + mulhi64(w0.z, w0.w, deg)];
            }
        }
        if (a.trip) {
            int32_t* out = a.trip + (((size_t)x * a.steps + t) * a.P + lane) * 3;
            out[0] = role; out[1] = du; out[2] = dother;
        }
        return {role, max(du, 0), max(dother, 0)};          // a triplet that was not drawn loads rows 0 and is not used
    }
    // A = the user's row, B = the other item's: d_x = <u, w>, d_o = <u, v_other>, the gradient gains -+s u + (li | lj) w
    static __device__ const float* row_a(const Args& a, int u) { return a.U + (size_t)u * a.k; }
    static __device__ const float* row_b(const Args& a, int o) { return a.V + (size_t)o * a.k; }
    static __device__ void biases(const Args& a, int, int o, float& bu, float& bo) {
        bu = 0.f;
        bo = a.b ? a.b[o] : 0.f;
    }
    static __device__ void dot(float w, float u, float vo, float& dx, float& d_o) {
        dx = fmaf(u, w, dx);
        d_o = fmaf(u, vo, d_o);
    }
    // x_p in the order of ref_np.bpr_step: b_i - b_j + x_ui - x_uj
    __device__ float score(int role, float, float bo, float dx, float d_o) const {
        return role == 1 ? bx - bo + dx - d_o : bo - bx + d_o - dx;
    }
    static __device__ float coef(int role, float s) { return role == 1 ? -s : s; }
    static __device__ float lam(const Args& a, int role) { return role == 1 ? a.li : a.lj; }
    static __device__ float dir(float u, float) { return u; }
    // the part of the objective that depends on (w, b_x): `rw` = |w|^2 / 2 (mode 1: |w|_1), over npos role-1 and nneg role-0 triplets
    __device__ float penalty(const Args& a, float rw, int npos, int nneg) const {
        return ((float)npos * a.li + (float)nneg * a.lj) * rw + (float)(npos + nneg) * a.lb * fold_reg_value(a.mode == 0, bx);
    }
    __device__ float bias_grad(const Args& a, float c, bool l2) const { return c + a.lb * (l2 ? bx : sgn(bx)); }
    __device__ void update_bias(const Args& a, float gb) {
        if (has_b) fold_rmsprop(msb, bx, gb, a.lr);
    }
    __device__ void store_bias(const Args& a, int64_t x) const { a.bn[x] = has_b ? bx : b_start; }
};

}  // namespace tkr

extern "C" int tkr_bpr_foldin_items(const float* U, const float* V, const float* b, int32_t n_users, int32_t n_items, int32_t k,
                                    const int64_t* user_ptr, const int32_t* user_cols, const int64_t* liker_ptr,
                                    const int32_t* liker_rows, const uint32_t* role_thresh, int32_t m, const float* V0, const float* b0,
                                    float li, float lj, float lb, float lr, int32_t mode, int32_t steps, int32_t triplets, uint64_t seed,
                                    uint64_t first_row, float* Vn, float* bn, float* loss, int32_t* trip, void* stream) {
    if (!U || !V || !user_ptr || !user_cols || !liker_ptr || !liker_rows || !role_thresh || !Vn || !bn) return TKR_EINVAL;
    if (n_users <= 0 || n_items <= 0 || k <= 0 || m < 0 || steps < 1 || triplets < 1 || triplets > TKR_WAVE) return TKR_EINVAL;
    if ((mode != 0 && mode != 1) || !(lr == lr) || !(li == li) || !(lj == lj) || !(lb == lb)) return TKR_EINVAL;
    if (m == 0) return TKR_OK;
    tkr::ItemFoldArgs a;
    a.U = U; a.V = V; a.b = b; a.user_ptr = user_ptr; a.user_cols = user_cols; a.liker_ptr = liker_ptr; a.liker_rows = liker_rows;
    a.role_thresh = role_thresh; a.start = V0; a.b0 = b0; a.out = Vn; a.bn = bn; a.loss = loss; a.trip = trip;
    a.m = m; a.n_users = n_users; a.n_items = n_items; a.k = k; a.mode = mode; a.steps = steps; a.P = triplets;
    a.li = li; a.lj = lj; a.lb = lb; a.lr = lr;
    a.k0 = (uint32_t)seed; a.k1 = (uint32_t)(seed >> 32);
    a.first_row = first_row;
    return tkr::launch_fold<tkr::ItemSide>(a, (uintptr_t)U | (uintptr_t)V | (uintptr_t)Vn | (uintptr_t)V0, (hipStream_t)stream);
}
