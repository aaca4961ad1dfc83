// K9 -- fold-in: user vectors for histories the model was not trained on, against FROZEN item factors.
//
// The reference has no such call (a user exists only as a row trained by single/bpr.py:136-150).  The step is the model's own:
// for one user, T times, the BPR step of single/bpr.py:81-100 on a batch of P triplets that all carry this user -- x = b_i - b_j +
// <u, v_i - v_j>, g = sum_p [-sigma(-x_p) (v_i - v_j) + lu u] (mode 1: lu sign(u)) in the order p = 0 .. P-1, one RMSProp update of u
// (slot from 1.0) -- with the item rows, their biases and their slots left alone (tests/_foldin_oracle.py restates it with
// oracle/ref_np.py bpr_step).
//
// Users are independent and nothing but U is written: one wave owns a user from the first step to the last, in the body K9 and K10
// share (csrc/fold_rows.h: fold_kernel in registers to k = 512, fold_wide_kernel in LDS beyond).  This file is the user side of it:
// the argument block, the draw -- lane p draws triplet p with sampler_draw.h draw_pair on stream 1: counter = (((first_row + x) T +
// t) P + p, round, 1), so a user's stream does not depend on who shares the call --, the two rows of a triplet (both from the item
// table, 5-9 MB at the benchmark shapes: it never leaves the caches), the formulas of the step, and the entry point.
#include <math.h>

#include "fold_rows.h"
#include "sampler_draw.h"
#include "../../include/tkr.h"

namespace tkr {

struct FoldArgs {
    const float* V;
    const float* b;              // nullable
    const int64_t* hist_ptr;
    const int32_t* hist_cols;
    const float* start;          // U0, nullable: zeros
    float* out;                  // U
    float* loss;                 // nullable
    int32_t* trip;               // nullable
    int32_t m, n_items, k, mode, steps, P;
    float lu, lr;
    uint32_t k0, k1;
    uint64_t first_row;
};

// the state of user x: `cols` is the user's row (ascending, unique: positives and membership test read the same array)
struct UserSide {
    using Args = FoldArgs;
    static constexpr bool kBias = false;
    const int32_t* cols;
    int deg;

    __device__ UserSide(const Args& a, int64_t x) {
        const int64_t lo = a.hist_ptr[x];
        cols = a.hist_cols + lo;
        deg = (int)(a.hist_ptr[x + 1] - lo);
    }
    // an empty history has no positive, one that covers the catalogue no negative: both keep the start vector, decided before any draw
    __device__ int steps(const Args& a) const { return (deg <= 0 || deg >= a.n_items) ? 0 : a.steps; }
    // lane p < P holds triplet p = (i, j), 0 < deg < n_items; the user is the user of every triplet: one role
    __device__ FoldTriplet draw(const Args& a, int64_t x, int t, int lane) const {
        int di = 0, dj = 0;
        if (lane < a.P) {
            const uint64_t g = fold_counter(a, x, t, lane);
            const uint32_t c0 = (uint32_t)g, c1 = (uint32_t)(g >> 32);
            const u32x4 w0 = philox4x32_10(c0, c1, 0u, 1u, a.k0, a.k1);
            draw_pair<1u>(cols, cols, 0, deg, (uint32_t)a.n_items, w0, c0, c1, a.k0, a.k1, di, dj);
            if (a.trip) reinterpret_cast<int2*>(a.trip)[((size_t)x * a.steps + t) * a.P + lane] = make_int2(di, dj);
        }
        return {1, di, dj};
    }
    // A = v_i, B = v_j: x_p = b_i - b_j + <w, v_i> - <w, v_j>, the gradient gains -s (v_i - v_j) + lu w
    static __device__ const float* row_a(const Args& a, int i) { return a.V + (size_t)i * a.k; }
    static __device__ const float* row_b(const Args& a, int j) { return a.V + (size_t)j * a.k; }
    static __device__ void biases(const Args& a, int i, int j, float& bi, float& bj) {
        bi = a.b ? a.b[i] : 0.f;
        bj = a.b ? a.b[j] : 0.f;
    }
    static __device__ void dot(float w, float vi, float vj, float& xi, float& xj) {
        xi = fmaf(w, vi, xi);
        xj = fmaf(w, vj, xj);
    }
    __device__ float score(int, float bi, float bj, float xi, float xj) const { return bi - bj + xi - xj; }
    static __device__ float coef(int, float s) { return -s; }
    static __device__ float lam(const Args& a, int) { return a.lu; }
    static __device__ float dir(float vi, float vj) { return vi - vj; }
    __device__ float penalty(const Args& a, float rw, int, int) const { return (float)a.P * a.lu * rw; }
};

}  // namespace tkr

extern "C" int tkr_bpr_foldin(const float* V, const float* b, int32_t n_items, int32_t k, const int64_t* hist_ptr,
                              const int32_t* hist_cols, int32_t m, const float* U0, float lu, float lr, int32_t mode, int32_t steps,
                              int32_t triplets, uint64_t seed, uint64_t first_row, float* U, float* loss, int32_t* trip, void* stream) {
    if (!V || !hist_ptr || !hist_cols || !U) return TKR_EINVAL;
    if (n_items <= 0 || k <= 0 || m < 0 || steps < 1 || triplets < 1 || triplets > TKR_WAVE) return TKR_EINVAL;
    if ((mode != 0 && mode != 1) || !(lr == lr) || !(lu == lu)) return TKR_EINVAL;
    if (m == 0) return TKR_OK;
    tkr::FoldArgs a;
    a.V = V; a.b = b; a.hist_ptr = hist_ptr; a.hist_cols = hist_cols; a.start = U0; a.out = U; a.loss = loss; a.trip = trip;
    a.m = m; a.n_items = n_items; a.k = k; a.mode = mode; a.steps = steps; a.P = triplets;
    a.lu = lu; a.lr = lr;
    a.k0 = (uint32_t)seed; a.k1 = (uint32_t)(seed >> 32);
    a.first_row = first_row;
    return tkr::launch_fold<tkr::UserSide>(a, (uintptr_t)V | (uintptr_t)U | (uintptr_t)U0, (hipStream_t)stream);
}
