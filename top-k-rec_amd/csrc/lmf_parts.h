// The pieces of K25 (csrc/lmf.hip): its constants, and sigma and softplus, written ONCE for both kernels.  K27 (csrc/smf.hip) has the
// same tiles, pitches and heavy rows.
#pragma once
#include "als_parts.h"

namespace tkr {

typedef float lmf_f32x16 __attribute__((ext_vector_type(16)));

constexpr int kLmfBlock = 256;
constexpr int kLmfWaves = kLmfBlock / TKR_WAVE;
constexpr int kLmfTile = 32;                                      // rows of Y staged at a time = the MFMA's block edge
constexpr int kLmfRows = kLmfWaves * kLmfTile;                    // rows of X a workgroup owns: 32 per wave
constexpr int kLmfSlab = TKR_LMF_SLAB;
constexpr int kLmfPPitch = kLmfTile + 1;                          // floats between two rows of a wave's P: odd, so 32 rows lie in 32 banks
constexpr int kLmfLikeSlab = TKR_LMF_LIKE_SLAB;
constexpr int kLmfHeavyWaves = TKR_LMF_HEAVY_WAVES;
constexpr int kLmfHeavyBlock = kLmfHeavyWaves * TKR_WAVE;
static_assert(kLmfSlab % kLmfTile == 0 && kLmfHeavyBlock <= 1024, "whole tiles; one workgroup");

// floats between two staged rows of Y: odd, so the first product (a lane per staged row, two columns apart by lane half) and the second
// (a lane per column, ds_read_b32 banks by 32-lane half) both read without a conflict
__host__ __device__ constexpr int lmf_stage_pitch(int KT) { return KT * 32 + 1; }

// the workspace of K25 and K27: pieces of whole 16 bytes; the list of heavy rows is a counter, then the rows
static inline int64_t lmf_align(int64_t bytes) { return (bytes + 15) / 16 * 16; }
static inline int64_t lmf_list_bytes(int64_t n_x) { return lmf_align(16 + n_x * 4); }

// Finite at every finite s.  exp(-s) is +0 from s = 104 on and 1 + e is 1.0f from s = 17 on: sigma(s) == 1.0f for s >= 40.  exp(-s) is
// +inf below s = -88.8, and 1 / inf = +0: sigma(s) == +0 for s <= -110.  The division is IEEE: sigma(0) == 0.5f.
__device__ __forceinline__ float lmf_sigmoid(float s) { return 1.0f / (1.0f + __expf(-s)); }
// max(s, 0) + log1p(exp(-|s|)): the second term is at most log 2, and +0 where exp underflows -- softplus(1e4) == 1e4
__device__ __forceinline__ float lmf_softplus(float s) { return fmaxf(s, 0.f) + log1pf(__expf(-fabsf(s))); }

}  // namespace tkr
