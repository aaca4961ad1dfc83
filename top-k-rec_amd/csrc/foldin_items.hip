// K10 -- fold-in of items: rows and biases for items that were not a line of `vid` when the model was trained, against FROZEN user
// factors and the frozen rest of the catalogue.  The item-side twin of K9 (csrc/foldin.hip); the reference can only retrain.
//
// For one new item x, T times, the model's own step (single/bpr.py:81-100) on a batch of P triplets that all carry x -- as the
// positive of a user who likes it (role 1: x_p = b_x - b_j + <u, v_x - v_j>, the gradient of v_x gains -s u + li v_x, that of b_x
// -s + lb b_x, s = sigma(-x_p)) or as the negative of a user who does not (role 0: x_p = b_i - b_x + <u, v_i - v_x>, +s u + lj v_x,
// +s + lb b_x); mode 1: the sign forms of the regularisers.  Sums in the order p = 0 .. P-1, then one RMSProp update of v_x and one
// of b_x (slots from 1.0).  U, V, b are read only (tests/_item_foldin_oracle.py restates it with oracle/ref_np.py bpr_step).
//
// Items are independent: one wave owns an item from the first step to the last, v_x, its slot and the gradient sum in registers
// (k <= 512; wider: foldin_items_wide_kernel keeps them in LDS), b_x and its slot in every lane.  No plan, no versions, no atomics.
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
    const float* V0;             // nullable: zeros
    const float* b0;             // nullable: zeros
    float* Vn;
    float* bn;
    float* loss;                 // nullable
    int32_t* trip;               // nullable
    int32_t m, n_users, n_items, k, mode, steps, P;
    float li, lj, lb, lr;
    uint32_t k0, k1;
    uint64_t first_row;
};

// the draw of step t for item x: lane p < P holds triplet p as (role, user, other item); lanes >= P hold role -1
__device__ __forceinline__ void item_fold_draw(const ItemFoldArgs& a, const int32_t* __restrict__ likers, int nl, uint32_t thresh,
                                               int64_t x, int t, int lane, int& role, int& du, int& dother) {
    role = -1;
    du = -1;
    dother = -1;
    if (lane >= a.P) return;
    const uint64_t g = ((a.first_row + (uint64_t)x) * (uint64_t)a.steps + (uint64_t)t) * (uint64_t)a.P + (uint64_t)lane;
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
}

// x_p of a triplet from the two dot products d_x = <u, v_x>, d_o = <u, v_other>, in the order of ref_np.bpr_step: b_i - b_j + x_ui - x_uj
__device__ __forceinline__ float item_fold_score(bool pos, float bx, float bo, float dx, float d_o) {
    return pos ? bx - bo + dx - d_o : bo - bx + d_o - dx;
}

// the part of the objective that depends on (v_x, b_x): `rv` = |v_x|^2 / 2 (mode 1: |v_x|_1), over npos role-1 and nneg role-0 triplets
__device__ __forceinline__ float item_fold_penalty(const ItemFoldArgs& a, float rv, float bx, int npos, int nneg) {
    const float rb = a.mode == 0 ? 0.5f * bx * bx : fabsf(bx);
    return ((float)npos * a.li + (float)nneg * a.lj) * rv + (float)(npos + nneg) * a.lb * rb;
}

template <int NE, bool VEC>
__global__ __launch_bounds__(kFoldWaves * TKR_WAVE) void foldin_items_kernel(const ItemFoldArgs a) {
    constexpr int G = kFoldGroup<NE>;
    const int lane = threadIdx.x & (TKR_WAVE - 1);
    const int64_t x = __builtin_amdgcn_readfirstlane((int)(blockIdx.x * kFoldWaves + (threadIdx.x >> 6)));
    if (x >= a.m) return;
    const int k = a.k, P = a.P;
    float v[NE], ms[NE], g[NE];
    if (a.V0) fold_load<NE, VEC>(a.V0 + (size_t)x * k, k, lane, v);
    else {
#pragma unroll
        for (int e = 0; e < NE; ++e) v[e] = 0.f;
    }
#pragma unroll
    for (int e = 0; e < NE; ++e) ms[e] = 1.f;
    const float b_start = a.b0 ? a.b0[x] : 0.f;
    const bool has_b = a.b != nullptr;
    float bx = has_b ? b_start : 0.f, msb = 1.f;
    const int64_t llo = a.liker_ptr[x];
    const int nl = (int)(a.liker_ptr[x + 1] - llo);
    const int32_t* likers = a.liker_rows + llo;
    const uint32_t thresh = a.role_thresh[x];
    const bool l2 = a.mode == 0;
    float loss = 0.f;
    for (int t = 0; t < a.steps; ++t) {
        int drole, du, dother;
        item_fold_draw(a, likers, nl, thresh, x, t, lane, drole, du, dother);
        if (__ballot(drole >= 0) == 0) continue;          // no triplet in this step: nothing moves, not even the slots
        const bool want_loss = a.loss != nullptr && t == a.steps - 1;
#pragma unroll
        for (int e = 0; e < NE; ++e) g[e] = 0.f;
        float gb = 0.f, loss_x = 0.f;
        int npos = 0, nneg = 0;
        for (int done = 0; done < P; done += G) {
            float ur[G][NE], vo[G][NE], bo[G];
            int rl[G];
#pragma unroll
            for (int q = 0; q < G; ++q) {              // slots beyond the last triplet, or of a triplet that was not drawn, load row 0 and are not used
                const int src = min(done + q, P - 1);
                rl[q] = (done + q < P) ? bcast_i(drole, src) : -1;
                const int u = max(bcast_i(du, src), 0), o = max(bcast_i(dother, src), 0);
                fold_load<NE, VEC>(a.U + (size_t)u * k, k, lane, ur[q]);
                fold_load<NE, VEC>(a.V + (size_t)o * k, k, lane, vo[q]);
                bo[q] = has_b ? a.b[o] : 0.f;
            }
#pragma unroll
            for (int q = 0; q < G; ++q) {
                if (rl[q] >= 0) {                       // wave-uniform
                    float dx = 0.f, d_o = 0.f;
#pragma unroll
                    for (int e = 0; e < NE; ++e) {
                        dx = fmaf(ur[q][e], v[e], dx);
                        d_o = fmaf(ur[q][e], vo[q][e], d_o);
                    }
                    wave_sum2(dx, d_o);
                    const bool pos = rl[q] == 1;
                    const float xs = item_fold_score(pos, bx, bo[q], dx, d_o);
                    const float s = sigmoid_neg(xs);
                    const float c = pos ? -s : s, lam = pos ? a.li : a.lj;
                    if (want_loss) loss_x += softplus_neg(xs);
                    npos += pos;
                    nneg += !pos;
#pragma unroll
                    for (int e = 0; e < NE; ++e) g[e] += c * ur[q][e] + lam * (l2 ? v[e] : sgn(v[e]));
                    gb += c + a.lb * (l2 ? bx : sgn(bx));
                }
            }
        }
        if (want_loss) {
            float r = 0.f;
#pragma unroll
            for (int e = 0; e < NE; ++e) r += l2 ? 0.5f * v[e] * v[e] : fabsf(v[e]);
            loss = loss_x + item_fold_penalty(a, wave_sum(r), bx, npos, nneg);
        }
#pragma unroll
        for (int e = 0; e < NE; ++e) {                   // TF SparseApplyRMSProp, momentum 0 (oracle/ref_np.py _rmsprop_rows)
            ms[e] = kFoldRho * ms[e] + (1.f - kFoldRho) * g[e] * g[e];
            v[e] = v[e] - a.lr * g[e] / sqrtf(ms[e] + kFoldEps);
        }
        if (has_b) {
            msb = kFoldRho * msb + (1.f - kFoldRho) * gb * gb;
            bx = bx - a.lr * gb / sqrtf(msb + kFoldEps);
        }
    }
    fold_store<NE, VEC>(a.Vn + (size_t)x * k, k, lane, v);
    if (lane == 0) {
        a.bn[x] = has_b ? bx : b_start;
        if (a.loss) a.loss[x] = loss;
    }
}

// ---- any width: v_x, its slot and the gradient sum in LDS (3 k floats), one wave = one workgroup = one item, as foldin_wide_kernel:
// element e belongs to lane e % 64 in every pass, so no lane reads what another wrote and no barrier is needed; two passes over the
// rows of a triplet (the dot products, then the gradient).
__global__ __launch_bounds__(TKR_WAVE) void foldin_items_wide_kernel(const ItemFoldArgs a) {
    extern __shared__ float4 item_fold_lds[];
    const int lane = threadIdx.x;
    const int64_t x = blockIdx.x;
    const int k = a.k, P = a.P;
    float* v = reinterpret_cast<float*>(item_fold_lds);
    float* ms = v + k;
    float* g = ms + k;
    for (int e = lane; e < k; e += TKR_WAVE) {
        v[e] = a.V0 ? a.V0[(size_t)x * k + e] : 0.f;
        ms[e] = 1.f;
    }
    const float b_start = a.b0 ? a.b0[x] : 0.f;
    const bool has_b = a.b != nullptr;
    float bx = has_b ? b_start : 0.f, msb = 1.f;
    const int64_t llo = a.liker_ptr[x];
    const int nl = (int)(a.liker_ptr[x + 1] - llo);
    const int32_t* likers = a.liker_rows + llo;
    const uint32_t thresh = a.role_thresh[x];
    const bool l2 = a.mode == 0;
    float loss = 0.f;
    for (int t = 0; t < a.steps; ++t) {
        int drole, du, dother;
        item_fold_draw(a, likers, nl, thresh, x, t, lane, drole, du, dother);
        if (__ballot(drole >= 0) == 0) continue;
        const bool want_loss = a.loss != nullptr && t == a.steps - 1;
        float gb = 0.f, loss_x = 0.f;
        int npos = 0, nneg = 0;
        bool first = true;
        for (int p = 0; p < P; ++p) {
            const int role = bcast_i(drole, p);
            if (role < 0) continue;                      // wave-uniform
            const int u = bcast_i(du, p), o = bcast_i(dother, p);
            const float* ur = a.U + (size_t)u * k;
            const float* vo = a.V + (size_t)o * k;
            const float bo = has_b ? a.b[o] : 0.f;
            float dx = 0.f, d_o = 0.f;
            for (int e = lane; e < k; e += TKR_WAVE) {
                const float w = ur[e];
                dx = fmaf(w, v[e], dx);
                d_o = fmaf(w, vo[e], d_o);
            }
            wave_sum2(dx, d_o);
            const bool pos = role == 1;
            const float xs = item_fold_score(pos, bx, bo, dx, d_o);
            const float s = sigmoid_neg(xs);
            const float c = pos ? -s : s, lam = pos ? a.li : a.lj;
            if (want_loss) loss_x += softplus_neg(xs);
            npos += pos;
            nneg += !pos;
            for (int e = lane; e < k; e += TKR_WAVE) {
                const float o_ = v[e];
                const float part = c * ur[e] + lam * (l2 ? o_ : sgn(o_));
                g[e] = first ? part : g[e] + part;
            }
            gb += c + a.lb * (l2 ? bx : sgn(bx));
            first = false;
        }
        if (want_loss) {
            float r = 0.f;
            for (int e = lane; e < k; e += TKR_WAVE) r += l2 ? 0.5f * v[e] * v[e] : fabsf(v[e]);
            loss = loss_x + item_fold_penalty(a, wave_sum(r), bx, npos, nneg);
        }
        for (int e = lane; e < k; e += TKR_WAVE) {
            const float ge = g[e];
            const float m2 = kFoldRho * ms[e] + (1.f - kFoldRho) * ge * ge;
            ms[e] = m2;
            v[e] = v[e] - a.lr * ge / sqrtf(m2 + kFoldEps);
        }
        if (has_b) {
            msb = kFoldRho * msb + (1.f - kFoldRho) * gb * gb;
            bx = bx - a.lr * gb / sqrtf(msb + kFoldEps);
        }
    }
    for (int e = lane; e < k; e += TKR_WAVE) a.Vn[(size_t)x * k + e] = v[e];
    if (lane == 0) {
        a.bn[x] = has_b ? bx : b_start;
        if (a.loss) a.loss[x] = loss;
    }
}

template <int NE>
static int launch_item_fold(const ItemFoldArgs& a, bool vec, hipStream_t s) {
    const dim3 grid((a.m + kFoldWaves - 1) / kFoldWaves), block(kFoldWaves * TKR_WAVE);
    if (vec) hipLaunchKernelGGL((foldin_items_kernel<NE, true>), grid, block, 0, s, a);
    else hipLaunchKernelGGL((foldin_items_kernel<NE, false>), grid, block, 0, s, a);
    return (int)hipGetLastError();
}

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
    a.role_thresh = role_thresh; a.V0 = V0; a.b0 = b0; a.Vn = Vn; a.bn = bn; a.loss = loss; a.trip = trip;
    a.m = m; a.n_users = n_users; a.n_items = n_items; a.k = k; a.mode = mode; a.steps = steps; a.P = triplets;
    a.li = li; a.lj = lj; a.lb = lb; a.lr = lr;
    a.k0 = (uint32_t)seed; a.k1 = (uint32_t)(seed >> 32);
    a.first_row = first_row;
    hipStream_t s = (hipStream_t)stream;
    const int ne = (k + TKR_WAVE - 1) / TKR_WAVE;
    const bool aligned = (((uintptr_t)U | (uintptr_t)V | (uintptr_t)Vn | (uintptr_t)V0) & 15) == 0;
    if (ne == 1) return tkr::launch_item_fold<1>(a, aligned && k == 64, s);
    if (ne == 2) return tkr::launch_item_fold<2>(a, aligned && k == 128, s);
    if (ne <= 4) return tkr::launch_item_fold<4>(a, aligned && k == 256, s);
    if (ne <= 8) return tkr::launch_item_fold<8>(a, aligned && k == 512, s);
    const size_t lds = (size_t)3 * k * sizeof(float);
    if (lds > (size_t)tkr::kFoldMaxLds) return TKR_EUNSUPPORTED;
    if (lds > 48 * 1024)
        TKR_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(tkr::foldin_items_wide_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    hipLaunchKernelGGL(tkr::foldin_items_wide_kernel, dim3(m), dim3(TKR_WAVE), lds, s, a);
    TKR_LAUNCH_CHECK();
    return TKR_OK;
}
