// Host side of the VBPR step (K3), shared by csrc/vbpr_step.hip, csrc/vbpr_cols.hip and csrc/vbpr_wide.hip: which slices of a plan
// one batch reads (VbprBatch), where the step's scratch lies in the workspace (VbprCarve, and from it the size), the team dispatch,
// the state check of the two entry points, and the launchers the three files call in each other.
#pragma once
#include <type_traits>

#include "tkr_common.h"
#include "../../include/tkr.h"
#include "vbpr_rows.h"

// the step's own scratch; the loss words of a call's batches lie behind it (tkr_vbpr_workspace_floats, csrc/vbpr_step.hip)
extern "C" __attribute__((visibility("hidden"))) int64_t tkr_vbpr_workspace_core_floats(int32_t batch_size, int32_t kh, int32_t d);

namespace tkr {

constexpr int kSlice = 128;                      // d-columns per split-K slice of V1 (64 per MFMA k-slot)

inline int vbpr_slices(int d) { return (d + kSlice - 1) / kSlice; }

// ---- a plan as a call hands it over (every array starts at the call's first batch), and the slices of batch b
struct VbprPlan {
    const int32_t *tri_i, *tri_j, *rec, *occ, *hdr, *occt;
    const int32_t *tri_u, *tpar;                 // K1's per-triplet parities; both or neither
    const int32_t *colh, *cent, *tcnt, *tent;    // the column plan (tkr_vbpr_colplan) or null
    int row_cap;                                 // ... and the longest feature row it was made for
};

struct VbprBatch {
    int B, tcap;                                 // tcap = 2 * row_cap: a triplet's gather list holds two feature rows
    const int32_t *ti, *tj, *tu, *tp;            // tu, tp: null when the caller passed no parities
    const int32_t* rec;
    const int2* occ2;
    const int32_t* occt;
    const int4* hdr4;
    const int4* colh;
    const int2* cent;
    const int32_t* tcnt;
    const int2* tent;
};

inline VbprBatch vbpr_batch(const VbprPlan& p, int d, int b, int B) {
    const size_t stride_r = (size_t)tkr_plan_max_blocks(B) * tkr_plan_team(B) * 16, stride_o = (size_t)3 * B, at = (size_t)b * B;
    const bool par = p.tri_u && p.tpar, cols = p.colh != nullptr;
    VbprBatch v;
    v.B = B;
    v.tcap = 2 * p.row_cap;
    v.ti = p.tri_i + at;
    v.tj = p.tri_j + at;
    v.tu = par ? p.tri_u + at : nullptr;
    v.tp = par ? p.tpar + at : nullptr;
    v.rec = p.rec + b * stride_r;
    v.occ2 = reinterpret_cast<const int2*>(p.occ + b * stride_o * 2);
    v.occt = p.occt + b * stride_o;
    v.hdr4 = reinterpret_cast<const int4*>(p.hdr + (size_t)b * 4);
    v.colh = cols ? reinterpret_cast<const int4*>(p.colh) + (size_t)b * d * 2 : nullptr;
    v.cent = cols ? reinterpret_cast<const int2*>(p.cent) + at * v.tcap : nullptr;
    v.tcnt = cols ? p.tcnt + at : nullptr;
    v.tent = cols ? reinterpret_cast<const int2*>(p.tent) + at * v.tcap : nullptr;
    return v;
}

// ---- the workspace.  Regions in the order they lie; `floats` is what they take together.
//   five launches (csrc/vbpr_step.hip, G1-G4 of csrc/vbpr_wide.hip):
//     ppart [S][B][kh+1] split-K partials | s_buf [B] S_t | P [B][kh] | Wm [B][kh] uce_u, then W_t | Q [B] | Aw [slots][kh], ab [slots]
//     the sparse view's per-item sums | ab2 [4][B] alpha, beta, e^alpha, e^beta | t_buf [B] T_t
//   column plan (csrc/vbpr_cols.hip, W1 / W3 of csrc/vbpr_wide.hip), over the head of the same floats:
//     s_buf [B] | t_buf [B] | ab2 [4][B] | P [B][kh] | Wm [B][kh]
struct VbprCarve {
    float *ppart, *s_buf, *P, *Wm, *Q, *Aw, *ab, *ab2, *t_buf;
    int64_t floats;
};

inline VbprCarve vbpr_carve(float* ws, int B, int kh, int d, bool column_plan) {
    VbprCarve c{};
    auto take = [&](float*& region, int64_t n) { region = ws ? ws + c.floats : nullptr; c.floats += n; };
    const int64_t rows = (int64_t)B * kh;
    if (column_plan) {
        take(c.s_buf, B); take(c.t_buf, B); take(c.ab2, 4ll * B); take(c.P, rows); take(c.Wm, rows);
        return c;
    }
    const int64_t slots = (int64_t)tkr_plan_max_blocks(B) * tkr_plan_team(B);      // one per item task
    take(c.ppart, (int64_t)vbpr_slices(d) * B * (kh + 1));
    take(c.s_buf, B); take(c.P, rows); take(c.Wm, rows); take(c.Q, B);
    take(c.Aw, slots * kh); take(c.ab, slots);
    take(c.ab2, 4ll * B); take(c.t_buf, B);
    return c;
}

// ---- f(team, big) with the batch size's team (csrc/plan_parts.h team_for) and "above 65,536" as compile-time constants: there the
// records' 16-bit triplet halves no longer hold an index and the first four come from occt (vbpr_rows.h read_rec)
template <int T> using team_c = std::integral_constant<int, T>;
template <class F>
inline auto vbpr_team_dispatch(int B, F&& f) {
    const bool big = B > 65536;
    switch (tkr_plan_team(B)) {
        case 4: return big ? f(team_c<4>{}, std::true_type{}) : f(team_c<4>{}, std::false_type{});
        case 8: return big ? f(team_c<8>{}, std::true_type{}) : f(team_c<8>{}, std::false_type{});
        default: return big ? f(team_c<16>{}, std::true_type{}) : f(team_c<16>{}, std::false_type{});
    }
}

// what both entry points ask of the state (tkr_vbpr_run also wants feat and, with f_ptr, the CSR / CSC pointers)
inline int vbpr_state_check(const tkr_vbpr_state* st) {
    if (!st || !st->U || !st->msU || !st->I || !st->msI || !st->irb || !st->msirb || !st->cem || !st->mscem || !st->icb || !st->msicb)
        return TKR_EINVAL;
    return st->n_users <= 0 || st->n_items <= 0 || st->kh <= 0 || st->d <= 0 ? TKR_EINVAL : TKR_OK;
}

// ---- launchers of one batch that another file calls: (state, batch, carve, the batch's loss words or slots, stream)
// csrc/vbpr_wide.hip, for csrc/vbpr_step.hip: G1 (+ G2 without parities) in front of the pair launch, G3 + G4 behind it
__attribute__((visibility("hidden"))) void vbpr_gen_front(const tkr_vbpr_state& st, const VbprBatch& bt, const VbprCarve& c, float* loss, hipStream_t s);
__attribute__((visibility("hidden"))) void vbpr_gen_back(const tkr_vbpr_state& st, const VbprBatch& bt, const VbprCarve& c, float* loss, hipStream_t s);
// csrc/vbpr_wide.hip, for csrc/vbpr_cols.hip: W1 in front of the pair-sum launch, W3 behind it
__attribute__((visibility("hidden"))) void vbpr_wide_project(const tkr_vbpr_state& st, const VbprBatch& bt, const VbprCarve& c, float* loss, hipStream_t s);
__attribute__((visibility("hidden"))) int vbpr_wide_col_blocks(int d);
__attribute__((visibility("hidden"))) void vbpr_wide_update(const tkr_vbpr_state& st, const VbprBatch& bt, const VbprCarve& c, float* loss, hipStream_t s);

}  // namespace tkr
