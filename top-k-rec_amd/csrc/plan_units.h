// K1: what csrc/sampler.hip, csrc/planner_mid.hip and csrc/planner_big.hip call in each other.  Helpers between translation units,
// not entry points: hidden, and extern "C" as the entry points around them are.
#pragma once
#include <stdint.h>

#include "../../include/tkr.h"

#define TKR_UNIT extern "C" __attribute__((visibility("hidden")))

// csrc/sampler.hip: K1c, the touch maps of a call folded into the update counters
TKR_UNIT int tkr_plan_commit(int32_t n_users, int32_t n_items, int32_t* ucnt, int32_t* icnt, uint32_t* touch_u, uint32_t* touch_i, void* stream);

// csrc/planner_mid.hip: the counting planner (1024 < batch <= 16,384); arguments as tkr_sample_plan
TKR_UNIT int tkr_plan_mid_ok(int32_t n_users, int32_t n_items, int32_t B);
TKR_UNIT int64_t tkr_plan_mid_workspace_bytes(int32_t batch_size, int32_t n_batches);
TKR_UNIT int tkr_sample_plan_mid(const int32_t* tr_users, int32_t n_tr, const int32_t* row_ptr, const int32_t* pos_cols, const int32_t* cols_sorted,
                                 int32_t n_users, int32_t n_items, uint64_t seed, uint64_t first_triplet, const int64_t* ctl, int32_t n_batches, int32_t B,
                                 int32_t* ucnt, int32_t* icnt, uint32_t* touch_u, uint32_t* touch_i, int32_t* out_u, int32_t* out_i, int32_t* out_j,
                                 int32_t* task, int32_t* occ, int32_t* rec, int32_t* hdr, int32_t* occt, int32_t* tpar, void* workspace,
                                 int64_t workspace_bytes, void* stream);

// csrc/planner_big.hip: the grid-wide planner (any batch size); arguments as tkr_sample_plan
TKR_UNIT int64_t tkr_plan_workspace_bytes_for(int32_t batch_size, int32_t n_batches);
TKR_UNIT int tkr_sample_plan_big(const int32_t* tr_users, int32_t n_tr, const int32_t* row_ptr, const int32_t* pos_cols, const int32_t* cols_sorted,
                                 int32_t n_users, int32_t n_items, uint64_t seed, uint64_t first_triplet, const int64_t* ctl, int32_t n_batches, int32_t B,
                                 int32_t* ucnt, int32_t* icnt, uint32_t* touch_u, uint32_t* touch_i, int32_t* out_u, int32_t* out_i, int32_t* out_j,
                                 int32_t* task, int32_t* occ, int32_t* rec, int32_t* hdr, int32_t* occt, int32_t* tpar, void* workspace,
                                 int64_t workspace_bytes, void* stream);
