// K3 for ANY factor width -- the generic form of the column-plan step (csrc/vbpr_cols.hip; single/vbpr.py:50-73,114).
//
// The kernels of csrc/vbpr_cols.hip hold a half-width row (kh = k // 2 factors) in one or two registers per lane and a cem row in
// the float4s of a column group: kh <= 128, kh % 4 == 0.  single/vbpr.py:18 takes any k.  Here nothing is resident: every kernel
// walks the factor dimension in strides of its thread count, on the SAME plan (K1's launch records, the column plan of
// tkr_vbpr_colplan), the same double buffering, the same loss words and the same pair-sum launch (vbpr_pairsum_kernel works on
// alpha / beta only).  Slow -- a row task re-walks its occurrence list once per 64 factors, a column task its run once per 64 --
// but the same objective and updates; sums in another order than the register form, inside the tolerance of the step tests.
//
//   W1 vbpr_wide_project_kernel   one workgroup per triplet: P_t = (f_i - f_j).cem from the triplet's gather list (staged in LDS),
//                                 alpha_t, beta_t, e^alpha, e^beta, uce_u(t), the regularisers' share of the loss
//   L2 vbpr_pairsum_kernel        (csrc/vbpr_cols.hip)
//   W3 vbpr_wide_update_kernel    row blocks: a wave per launch record (wave 0 of a heavy team walks the whole team), factor by factor;
//                                 column blocks: a wave per feature column, TF's dense ApplyRMSProp on cem[c][.] and icb[c]
#include "vbpr_host.h"

namespace tkr {

__global__ __launch_bounds__(256) void vbpr_wide_project_kernel(tkr_vbpr_state st, const int32_t* __restrict__ ti, const int32_t* __restrict__ tj,
                                                               const int32_t* __restrict__ tu, const int32_t* __restrict__ tpar,
                                                               const int32_t* __restrict__ tcnt, const int2* __restrict__ tent, int tcap, int B,
                                                               float* __restrict__ P, float* __restrict__ ab_out, float* __restrict__ Wraw,
                                                               float* __restrict__ loss_out) {
    extern __shared__ int2 s_ent[];                              // the triplet's gather list: (column, +-value bits)
    __shared__ float s_red[4][4];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, t = blockIdx.x;
    const int kh = st.kh, k2 = 2 * kh;
    const int n = tcnt[t];
    for (int e = tid; e < n; e += 256) s_ent[e] = tent[(size_t)t * tcap + e];
    const int pr = tpar[t], u = tu[t], i = ti[t], j = tj[t];
    const float* urow = st.U + ((size_t)(pr & 1) * st.n_users + u) * k2;
    const float* ri = st.I + ((size_t)((pr >> 1) & 1) * st.n_items + i) * kh;
    const float* rj = st.I + ((size_t)((pr >> 2) & 1) * st.n_items + j) * kh;
    const float bi = st.irb[(size_t)((pr >> 1) & 1) * st.n_items + i], bj = st.irb[(size_t)((pr >> 2) & 1) * st.n_items + j];
    __syncthreads();
    const bool l2 = st.mode == 0;
    float d = 0.f, q = 0.f, reg = 0.f;
    for (int c = tid; c < kh; c += 256) {
        float acc = 0.f;
        for (int e = 0; e < n; ++e) acc = fmaf(__int_as_float(s_ent[e].y), st.cem[(size_t)s_ent[e].x * kh + c], acc);
        P[(size_t)t * kh + c] = acc;
        const float a = urow[c], b = urow[kh + c], x = ri[c], y = rj[c];
        Wraw[(size_t)t * kh + c] = b;
        d = fmaf(a, x - y, d);
        d = fmaf(b, acc, d);
        reg += l2 ? 0.5f * ((a * a + b * b) * st.lu + x * x * st.li + y * y * st.lj) : (fabsf(a) + fabsf(b)) * st.lu + fabsf(x) * st.li + fabsf(y) * st.lj;
    }
    for (int e = tid; e < n; e += 256) q = fmaf(__int_as_float(s_ent[e].y), st.icb[s_ent[e].x], q);
    d = wave_sum(d); q = wave_sum(q); reg = wave_sum(reg);
    if (lane == 0) { s_red[wave][0] = d; s_red[wave][1] = q; s_red[wave][2] = reg; }
    __syncthreads();
    if (tid == 0) {
        const float beta = (s_red[0][0] + s_red[1][0]) + (s_red[2][0] + s_red[3][0]);
        const float alpha = bi - bj + ((s_red[0][1] + s_red[1][1]) + (s_red[2][1] + s_red[3][1]));
        ab_out[t] = alpha; ab_out[B + t] = beta; ab_out[2 * B + t] = pair_exp(alpha); ab_out[3 * B + t] = pair_exp(beta);
        if (loss_out)
            loss_out[t] = ((s_red[0][2] + s_red[1][2]) + (s_red[2][2] + s_red[3][2])) + (l2 ? 0.5f * (bi * bi + bj * bj) * st.lb : (fabsf(bi) + fabsf(bj)) * st.lb);
    }
}

// occurrence q of a record: the first four ride in it, the others in the occurrence lists (stride `team`)
__device__ __forceinline__ void wide_occurrence(const WaveRec& r, int q, const int2* __restrict__ occ, const int32_t* __restrict__ occt, int& oa, int& ob,
                                                int& ot) {
    if (q < 4) {
        oa = q == 0 ? r.oa[0] : q == 1 ? r.oa[1] : q == 2 ? r.oa[2] : r.oa[3];
        ob = q == 0 ? r.ob[0] : q == 1 ? r.ob[1] : q == 2 ? r.ob[2] : r.ob[3];
        ot = q == 0 ? r.ot[0] : q == 1 ? r.ot[1] : q == 2 ? r.ot[2] : r.ot[3];
    } else {
        const int2 o = occ[r.first + q * r.team];
        oa = o.x; ob = o.y; ot = occt[r.first + q * r.team];
    }
}

__global__ __launch_bounds__(256) void vbpr_wide_update_kernel(tkr_vbpr_state st, const int32_t* __restrict__ rec_all, const int2* __restrict__ occ,
                                                              const int32_t* __restrict__ occt, const int4* __restrict__ hdr,
                                                              const float* __restrict__ sS, const float* __restrict__ sT, const float* __restrict__ P,
                                                              const float* __restrict__ Wraw, const int4* __restrict__ colh, const int2* __restrict__ cent,
                                                              int n_row_blocks, int n_col_blocks, float* __restrict__ loss_out /*[B] | [B] | [column blocks]*/,
                                                              int B) {
    __shared__ float s_loss[4];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int kh = st.kh, k2 = 2 * kh;
    const bool l2 = st.mode == 0;
    const size_t ustride = (size_t)st.n_users * k2, istride = (size_t)st.n_items * kh;
    if ((int)blockIdx.x < n_row_blocks) {
        // ---- row tasks (vbpr_rows_body, factor by factor)
        const int4 h4 = *hdr;
        const int n_blocks = __builtin_amdgcn_readfirstlane(h4.x), nlb = __builtin_amdgcn_readfirstlane(h4.y);
        for (int it = blockIdx.x; it < n_blocks; it += n_row_blocks) {
            const int blk = n_blocks - 1 - it;
            const bool heavy = blk >= nlb;
            if (heavy && wave != 0) continue;                    // wave 0 walks the records of the whole team, in wave order
            const int n_rec = heavy ? 4 : 1;
            const WaveRec head = read_rec(rec_all, 4, blk, heavy ? 0 : wave, lane);
            if (head.rowk == -1) continue;
            const bool is_item = head.rowk < 0;
            const int row = head.rowk & 0x7fffffff, par = head.par, width = is_item ? kh : k2;
            const float* src = is_item ? st.I + par * istride + (size_t)row * kh : st.U + par * ustride + (size_t)row * k2;
            const float* msrc = is_item ? st.msI + par * istride + (size_t)row * kh : st.msU + par * ustride + (size_t)row * k2;
            float* po = is_item ? st.I + (par ^ 1) * istride + (size_t)row * kh : st.U + (par ^ 1) * ustride + (size_t)row * k2;
            float* mo = is_item ? st.msI + (par ^ 1) * istride + (size_t)row * kh : st.msU + (par ^ 1) * ustride + (size_t)row * k2;
            const float br = is_item ? st.irb[(size_t)par * st.n_items + row] : 0.f;
            float gb = 0.f;
            for (int c0 = 0; c0 < width; c0 += 64) {             // (wave-uniform trip count)
                const int c = c0 + lane;
                const bool in = c < width;
                const float own = in ? src[c] : 0.f;
                float g = 0.f;
                for (int w = 0; w < n_rec; ++w) {
                    const WaveRec r = w == 0 ? head : read_rec(rec_all, 4, blk, w, lane);
                    if (r.rowk == -1) continue;
                    for (int q = 0; q < r.n_occ; ++q) {
                        int oa, ob, ot;
                        wide_occurrence(r, q, occ, occt, oa, ob, ot);
                        const float sa = sS[ot], sg = sT[ot];        // rows under alpha are scaled by S_t, rows under beta by T_t
                        if (is_item) {
                            const int u = oa & kIdMaskV, pu = (oa >> 30) & 1;
                            const bool role_j = ob < 0;
                            const float lam = role_j ? st.lj : st.li;
                            const float ur = in ? st.U[pu * ustride + (size_t)u * k2 + c] : 0.f;
                            g += (role_j ? sg : -sg) * ur + lam * (l2 ? own : sgn(own));
                            if (c0 == 0) gb += (role_j ? sa : -sa) + st.lb * (l2 ? br : sgn(br));
                        } else {
                            const int i = oa & kIdMaskV, pi = (oa >> 30) & 1, j = ob & kIdMaskV, pj = (ob >> 30) & 1;
                            float partner = 0.f;
                            if (in) partner = c < kh ? st.I[pi * istride + (size_t)i * kh + c] - st.I[pj * istride + (size_t)j * kh + c] : P[(size_t)ot * kh + c - kh];
                            g += -sg * partner + st.lu * (l2 ? own : sgn(own));
                        }
                    }
                }
                if (in) {
                    const float m2 = st.rho * msrc[c] + (1.f - st.rho) * g * g;
                    mo[c] = m2;
                    po[c] = own - st.lr * g / sqrtf(m2 + st.eps);
                }
            }
            if (is_item && lane == 0) {
                const float m2 = st.rho * st.msirb[(size_t)par * st.n_items + row] + (1.f - st.rho) * gb * gb;
                st.msirb[(size_t)(par ^ 1) * st.n_items + row] = m2;
                st.irb[(size_t)(par ^ 1) * st.n_items + row] = br - st.lr * gb / sqrtf(m2 + st.eps);
            }
        }
        return;
    }
    // ---- column tasks: four feature columns per block, a wave each
    const int cb = (int)blockIdx.x - n_row_blocks;
    const int c = cb * 4 + wave;
    float lpart = 0.f;
    if (c < st.d) {
        const int4 h0 = colh[(size_t)c * 2];
        const int n = h0.x, beg = h0.y;
        for (int l0 = 0; l0 < kh; l0 += 64) {
            const int l = l0 + lane;
            const bool in = l < kh;
            float g = 0.f;
            for (int e = 0; e < n; ++e) {
                const int2 en = cent[beg + e];                   // (triplet, +-value bits)
                g = fmaf(-__int_as_float(en.y) * sT[en.x], in ? Wraw[(size_t)en.x * kh + l] : 0.f, g);
            }
            if (in) {
                const float v = st.cem[(size_t)c * kh + l];
                const float gg = g + st.le * (l2 ? v : sgn(v));
                lpart += l2 ? 0.5f * st.le * v * v : st.le * fabsf(v);
                float ms = st.mscem[(size_t)c * kh + l];
                ms += (gg * gg - ms) * (1.f - st.rho);
                st.mscem[(size_t)c * kh + l] = ms;
                st.cem[(size_t)c * kh + l] = v - st.lr * gg / sqrtf(ms + st.eps);
            }
        }
        float gi = 0.f;
        for (int e = lane; e < n; e += 64) {
            const int2 en = cent[beg + e];
            gi = fmaf(-__int_as_float(en.y), sS[en.x], gi);
        }
        gi = wave_sum(gi);
        if (lane == 0) {
            const float v = st.icb[c];
            const float gg = gi + st.lb * (l2 ? v : sgn(v));
            lpart += l2 ? 0.5f * st.lb * v * v : st.lb * fabsf(v);
            float ms = st.msicb[c];
            ms += (gg * gg - ms) * (1.f - st.rho);
            st.msicb[c] = ms;
            st.icb[c] = v - st.lr * gg / sqrtf(ms + st.eps);
        }
    }
    if (loss_out) {
        lpart = wave_sum(lpart);
        if (lane == 0) s_loss[wave] = lpart;
        __syncthreads();
        if (threadIdx.x == 0) loss_out[2 * B + cb] = (s_loss[0] + s_loss[1]) + (s_loss[2] + s_loss[3]);
    }
}

// one batch of the generic form; the pair-sum launch between the two is the caller's (csrc/vbpr_cols.hip)
void vbpr_wide_project(const tkr_vbpr_state& st, const VbprBatch& bt, const VbprCarve& c, float* loss, hipStream_t s) {
    hipLaunchKernelGGL(vbpr_wide_project_kernel, dim3(bt.B), dim3(256), (size_t)bt.tcap * sizeof(int2), s, st, bt.ti, bt.tj, bt.tu, bt.tp, bt.tcnt, bt.tent,
                       bt.tcap, bt.B, c.P, c.ab2, c.Wm, loss);
}
int vbpr_wide_col_blocks(int d) { return (d + 3) / 4; }

// ------------------------------------------------------------------------------------------------------------------------------
// The generic form of the five-launch sparse view (csrc/vbpr_step.hip S1 / V1b / V1p / V2 / S3) for kh > 128: the batches the column
// plan does not take (batch > 1024, feature rows of more than 1024 nonzeros, column counters beyond the LDS).  Same K1 records, same
// workspace carve, same loss slots, same byte maps and slots of the sparse scratch; only the factor dimension is walked in passes.
//   G1 vbpr_gen_project_kernel  one workgroup per triplet: the nonzeros of f_i (+value) then f_j (-value) staged in LDS 256 at a time,
//                               thread c of a pass sums value * cem[col][c] over them in that order -- no row cap, a fixed order
//   G2 vbpr_gen_occur_kernel    (without K1's per-triplet parities) a wave per user record, 64 factors per pass
//   V1p vbpr_pair_kernel        unchanged (its W_t scaling strides by 64)
//   G3 vbpr_gen_rows_kernel     a wave per launch record, 64 factors per pass, heavy teams reduced through LDS in wave order
//   G4 vbpr_gen_sdense_kernel   a wave per feature column, 256 factors per walk of the column's CSC list
constexpr int kGenTile = 256;        // factors per pass of G1 (a thread each) and of G4 (four per lane)

__global__ __launch_bounds__(256) void vbpr_gen_project_kernel(tkr_vbpr_state st, const int32_t* __restrict__ ti, const int32_t* __restrict__ tj, int B,
                                                              float* __restrict__ P, float* __restrict__ Q, const int32_t* __restrict__ tu,
                                                              const int32_t* __restrict__ tpar, float* __restrict__ ab_out, float* __restrict__ Wm,
                                                              float* __restrict__ loss_out) {
    __shared__ int s_col[kGenTile];
    __shared__ float s_val[kGenTile];
    __shared__ float s_red[4][3];
    __shared__ uint32_t s_par;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, t = blockIdx.x;
    const int kh = st.kh, k2 = 2 * kh;
    if (t == 0) {                                       // new batch: advance the counter, clear the byte map of the batch before (as S1)
        const SparseScratch x = sparse_scratch(st);
        if (tid == 0) { const uint32_t c = *x.counter + 1u; *x.counter = c; s_par = c & 1u; }
        __syncthreads();
        uint32_t* other = reinterpret_cast<uint32_t*>(x.member(s_par ^ 1u));
        for (int w = tid; w < x.map_words; w += blockDim.x) other[w] = 0u;
    }
    const int i = ti[t], j = tj[t];
    const int bi0 = st.f_ptr[i], ni = st.f_ptr[i + 1] - bi0;
    const int bj0 = st.f_ptr[j], nj = st.f_ptr[j + 1] - bj0;
    const int n = ni + nj;
    const bool fused = tpar != nullptr, l2 = st.mode == 0;
    const float* urow = nullptr;
    const float* ri = nullptr;
    const float* rj = nullptr;
    float bi = 0.f, bj = 0.f;
    if (fused) {
        const int pr = tpar[t];
        urow = st.U + ((size_t)(pr & 1) * st.n_users + tu[t]) * k2;
        ri = st.I + ((size_t)((pr >> 1) & 1) * st.n_items + i) * kh;
        rj = st.I + ((size_t)((pr >> 2) & 1) * st.n_items + j) * kh;
        bi = st.irb[(size_t)((pr >> 1) & 1) * st.n_items + i];
        bj = st.irb[(size_t)((pr >> 2) & 1) * st.n_items + j];
    }
    float q = 0.f, dsum = 0.f, reg = 0.f;
    for (int c0 = 0; c0 < kh; c0 += kGenTile) {
        const int c = c0 + tid;
        const bool in = c < kh;
        float acc = 0.f;
        for (int e0 = 0; e0 < n; e0 += kGenTile) {
            const int e = e0 + tid;
            int col = 0;
            float val = 0.f;
            if (e < n) {
                const bool side_i = e < ni;
                const int p = side_i ? bi0 + e : bj0 + (e - ni);
                col = st.f_col[p];
                val = side_i ? st.f_val[p] : -st.f_val[p];
                if (c0 == 0) q = fmaf(val, st.icb[col], q);
            }
            __syncthreads();                            // the readers of the chunk before are done
            s_col[tid] = col;
            s_val[tid] = val;
            __syncthreads();
            const int m = min(kGenTile, n - e0);
            if (in) {
#pragma unroll 8
                for (int x = 0; x < m; ++x) acc = fmaf(s_val[x], st.cem[(size_t)s_col[x] * kh + c], acc);
            }
        }
        if (in) {
            P[(size_t)t * kh + c] = acc;
            if (fused) {                                // what V1b does per user occurrence, here per triplet
                const float a = urow[c], b = urow[kh + c], xv = ri[c], yv = rj[c];
                Wm[(size_t)t * kh + c] = b;             // scaled by -T_t once the pair kernel knows it
                dsum = fmaf(a, xv - yv, dsum);
                dsum = fmaf(b, acc, dsum);
                reg += l2 ? 0.5f * ((a * a + b * b) * st.lu + xv * xv * st.li + yv * yv * st.lj)
                          : (fabsf(a) + fabsf(b)) * st.lu + fabsf(xv) * st.li + fabsf(yv) * st.lj;
            }
        }
    }
    dsum = wave_sum(dsum);
    q = wave_sum(q);
    reg = wave_sum(reg);
    if (lane == 0) { s_red[wave][0] = dsum; s_red[wave][1] = q; s_red[wave][2] = reg; }
    __syncthreads();
    if (tid == 0) {
        const float qsum = (s_red[0][1] + s_red[1][1]) + (s_red[2][1] + s_red[3][1]);
        Q[t] = qsum;
        if (fused) {
            const float beta = (s_red[0][0] + s_red[1][0]) + (s_red[2][0] + s_red[3][0]);
            const float alpha = bi - bj + qsum;
            ab_out[t] = alpha; ab_out[B + t] = beta; ab_out[2 * B + t] = pair_exp(alpha); ab_out[3 * B + t] = pair_exp(beta);
            if (loss_out)
                loss_add_spread(loss_out, ((s_red[0][2] + s_red[1][2]) + (s_red[2][2] + s_red[3][2])) +
                                              (l2 ? 0.5f * (bi * bi + bj * bj) * st.lb : (fabsf(bi) + fabsf(bj)) * st.lb));
        }
    }
}

template <int kVTeam, bool kBig>
__global__ __launch_bounds__((kVTeam * TKR_WAVE)) void vbpr_gen_occur_kernel(
    tkr_vbpr_state st, const int32_t* __restrict__ rec_all, const int2* __restrict__ occ, const int32_t* __restrict__ occt,
    const int4* __restrict__ hdr, int B, const float* __restrict__ Q, float* __restrict__ ab_out, const float* __restrict__ P,
    float* __restrict__ Wm, float* __restrict__ loss_out) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int n_blocks = __builtin_amdgcn_readfirstlane((*hdr).x);
    const int kh = st.kh, k2 = 2 * kh;
    const size_t ustride = (size_t)st.n_users * k2, istride = (size_t)st.n_items * kh;
    const bool l2 = st.mode == 0;
    for (int blk = blockIdx.x; blk < n_blocks; blk += gridDim.x) {
        const WaveRec r = read_rec<kBig>(rec_all, kVTeam, blk, wave, lane, occt);
        if (r.rowk < 0) continue;                       // item task or idle wave (-1)
        const float* urow = st.U + r.par * ustride + (size_t)r.rowk * k2;
        float loss = 0.f, loss_lane = 0.f;
        for (int done = 0; done < r.n_occ; done += 4) {
          const int n = min(4, r.n_occ - done);
          int oa4[4], ob4[4], ot4[4];
          next_occ(r, done, n, lane, occ, occt, oa4, ob4, ot4);
          for (int qq = 0; qq < n; ++qq) {
            const int oa = oa4[qq], ob = ob4[qq], t = ot4[qq];
            const int i = oa & kIdMaskV, pi = (oa >> 30) & 1, j = ob & kIdMaskV, pj = (ob >> 30) & 1;
            const float* ri = st.I + pi * istride + (size_t)i * kh;
            const float* rj = st.I + pj * istride + (size_t)j * kh;
            float d1 = 0.f, d2 = 0.f;
            for (int c0 = 0; c0 < kh; c0 += 64) {
                const int c = c0 + lane;
                const bool in = c < kh;
                const float ure = in ? urow[c] : 0.f, uce = in ? urow[kh + c] : 0.f, p = in ? P[(size_t)t * kh + c] : 0.f;
                const float vi = in ? ri[c] : 0.f, vj = in ? rj[c] : 0.f;
                d1 = fmaf(ure, vi - vj, d1);
                d2 = fmaf(uce, p, d2);
                loss_lane += l2 ? 0.5f * ((ure * ure + uce * uce) * st.lu + vi * vi * st.li + vj * vj * st.lj)
                                : (fabsf(ure) + fabsf(uce)) * st.lu + fabsf(vi) * st.li + fabsf(vj) * st.lj;
                if (in) Wm[(size_t)t * kh + c] = uce;   // scaled by -T_t once the pair kernel knows it
            }
            const float bi = st.irb[(size_t)pi * st.n_items + i], bj = st.irb[(size_t)pj * st.n_items + j];
            const float alpha = bi - bj + Q[t], beta = wave_sum(d1) + wave_sum(d2);
            loss += l2 ? 0.5f * (bi * bi + bj * bj) * st.lb : (fabsf(bi) + fabsf(bj)) * st.lb;
            if (lane == 0) { ab_out[t] = alpha; ab_out[B + t] = beta; ab_out[2 * B + t] = pair_exp(alpha); ab_out[3 * B + t] = pair_exp(beta); }
          }
        }
        if (loss_out) {
            const float tot = wave_sum(loss_lane) + loss;
            if (lane == 0) loss_add_spread(loss_out, tot);
        }
    }
}

// G3: vbpr_rows_body with the factors in passes of 64 (every pass re-walks the record's occurrences); a heavy team's waves add their
// partial gradients through LDS in wave order, wave 0 updates the row
template <int kVTeam, bool kBig>
__global__ __launch_bounds__((kVTeam * TKR_WAVE)) void vbpr_gen_rows_kernel(
    tkr_vbpr_state st, const int32_t* __restrict__ rec_all, const int2* __restrict__ occ, const int32_t* __restrict__ occt,
    const int4* __restrict__ hdr, const float* __restrict__ sS, const float* __restrict__ sT, const float* __restrict__ P,
    const float* __restrict__ Wm, float* __restrict__ Aw /*[slots][kh]*/, float* __restrict__ ab /*[slots]*/) {
    __shared__ float red[kVTeam][TKR_WAVE + 1];
    __shared__ float red2[kVTeam][TKR_WAVE + 1];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int4 h4 = *hdr;
    const int n_blocks = __builtin_amdgcn_readfirstlane(h4.x), nlb = __builtin_amdgcn_readfirstlane(h4.y);
    const int kh = st.kh, k2 = 2 * kh;
    const size_t ustride = (size_t)st.n_users * k2, istride = (size_t)st.n_items * kh;
    const bool l2 = st.mode == 0;
    for (int it = blockIdx.x; it < n_blocks; it += gridDim.x) {
        const int blk = n_blocks - 1 - it;
        const bool heavy = blk >= nlb;                  // (every wave of a heavy team holds a record of the same row)
        const WaveRec r = read_rec<kBig>(rec_all, kVTeam, blk, wave, lane, occt);
        if (r.rowk == -1) continue;
        const bool is_item = r.rowk < 0, owner = !heavy || wave == 0;
        const int row = r.rowk & 0x7fffffff, par = r.par, width = is_item ? kh : k2;
        const float* src = is_item ? st.I + par * istride + (size_t)row * kh : st.U + par * ustride + (size_t)row * k2;
        const float* msrc = is_item ? st.msI + par * istride + (size_t)row * kh : st.msU + par * ustride + (size_t)row * k2;
        float* po = is_item ? st.I + (par ^ 1) * istride + (size_t)row * kh : st.U + (par ^ 1) * ustride + (size_t)row * k2;
        float* mo = is_item ? st.msI + (par ^ 1) * istride + (size_t)row * kh : st.msU + (par ^ 1) * ustride + (size_t)row * k2;
        const float br = is_item ? st.irb[(size_t)par * st.n_items + row] : 0.f;
        const int slot = blk * kVTeam + wave;
        float gb = 0.f, asum = 0.f;
        for (int c0 = 0; c0 < width; c0 += 64) {        // (the same trip count for every wave of a heavy team)
            const int c = c0 + lane;
            const bool in = c < width;
            const float own = in ? src[c] : 0.f;
            float g = 0.f, aw = 0.f;
            for (int qo = 0; qo < r.n_occ; ++qo) {
                int oa, ob, ot;
                wide_occurrence(r, qo, occ, occt, oa, ob, ot);
                const float sa = sS[ot], sg = sT[ot];   // rows under alpha are scaled by S_t, rows under beta by T_t
                if (is_item) {
                    const int u = oa & kIdMaskV, pu = (oa >> 30) & 1;
                    const bool role_j = ob < 0;
                    const float lam = role_j ? st.lj : st.li;
                    const float ur = in ? st.U[pu * ustride + (size_t)u * k2 + c] : 0.f;
                    g += (role_j ? sg : -sg) * ur + lam * (l2 ? own : sgn(own));
                    if (in) {
                        const float w = Wm[(size_t)ot * kh + c];
                        aw += role_j ? -w : w;
                    }
                    if (c0 == 0) {
                        const float sgn_a = role_j ? sa : -sa;
                        gb += sgn_a + st.lb * (l2 ? br : sgn(br));
                        asum += sgn_a;
                    }
                } else {
                    const int i = oa & kIdMaskV, pi = (oa >> 30) & 1, j = ob & kIdMaskV, pj = (ob >> 30) & 1;
                    float partner = 0.f;
                    if (in) partner = c < kh ? st.I[pi * istride + (size_t)i * kh + c] - st.I[pj * istride + (size_t)j * kh + c] : P[(size_t)ot * kh + c - kh];
                    g += -sg * partner + st.lu * (l2 ? own : sgn(own));
                }
            }
            if (heavy) {
                red[wave][lane] = g;
                red2[wave][lane] = aw;
                if (lane == 0) { red[wave][64] = gb; red2[wave][64] = asum; }
                __syncthreads();
                if (wave == 0) {
                    float a = 0.f, a2 = 0.f;
                    for (int w = 0; w < kVTeam; ++w) { a += red[w][lane]; a2 += red2[w][lane]; }
                    g = a;
                    aw = a2;
                    if (c0 == 0) {
                        float b = 0.f, b2 = 0.f;
                        for (int w = 0; w < kVTeam; ++w) { b += red[w][64]; b2 += red2[w][64]; }
                        gb = b;
                        asum = b2;
                    }
                }
                __syncthreads();
            }
            if (owner && in) {
                if (is_item) Aw[(size_t)slot * kh + c] = aw;
                const float m2 = st.rho * msrc[c] + (1.f - st.rho) * g * g;
                mo[c] = m2;
                po[c] = own - st.lr * g / sqrtf(m2 + st.eps);
            }
        }
        if (owner && is_item && lane == 0) {            // the item joins the batch's byte map; its slot = this wave's record index
            ab[slot] = asum;
            const SparseScratch x = sparse_scratch(st);
            x.slots[row] = slot;
            x.member(*x.counter)[row] = 1;
            const float m2 = st.rho * st.msirb[(size_t)par * st.n_items + row] + (1.f - st.rho) * gb * gb;
            st.msirb[(size_t)(par ^ 1) * st.n_items + row] = m2;
            st.irb[(size_t)(par ^ 1) * st.n_items + row] = br - st.lr * gb / sqrtf(m2 + st.eps);
        }
    }
}

// G4: S3 with the factors in passes of 256 (four per lane): the column's CSC list is walked once per pass, the batch's items added in
// ascending item order (a fixed summation order), then TF's dense ApplyRMSProp on cem[c][pass] (and icb[c] in the first pass)
__global__ __launch_bounds__(256) void vbpr_gen_sdense_kernel(tkr_vbpr_state st, const float* __restrict__ Aw, const float* __restrict__ ab,
                                                             float* __restrict__ loss_out) {
    const int lane = threadIdx.x & 63, c = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (c >= st.d) return;
    const int kh = st.kh;
    const int beg = st.c_ptr[c], end = st.c_ptr[c + 1];
    const SparseScratch x = sparse_scratch(st);
    const unsigned char* __restrict__ member = x.member(*x.counter);
    const bool l2 = st.mode == 0;
    float lpart = 0.f;
    for (int c0 = 0; c0 < kh; c0 += kGenTile) {
        float g[kGenTile / 64], gi = 0.f;
#pragma unroll
        for (int s = 0; s < kGenTile / 64; ++s) g[s] = 0.f;
        for (int p0 = beg; p0 < end; p0 += 64) {
            const int p = p0 + lane;
            const bool valid = p < end;
            const int item = valid ? st.c_item[p] : 0;
            const float val = valid ? st.c_val[p] : 0.f;
            const bool hit = valid && member[item] != 0;
            const int slot_l = hit ? x.slots[item] : 0;
            uint64_t m = __ballot(hit);
            while (m) {                                 // ascending lane = ascending item
                const int l = __ffsll((long long)m) - 1;
                m &= m - 1;
                const int slot = __builtin_amdgcn_readlane(slot_l, l);
                const float v = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(val), l));
#pragma unroll
                for (int s = 0; s < kGenTile / 64; ++s) {
                    const int n2 = c0 + s * 64 + lane;
                    g[s] = fmaf(v, n2 < kh ? Aw[(size_t)slot * kh + n2] : 0.f, g[s]);
                }
                if (c0 == 0) gi = fmaf(v, ab[slot], gi);
            }
        }
#pragma unroll
        for (int s = 0; s < kGenTile / 64; ++s) {
            const int n2 = c0 + s * 64 + lane;
            if (n2 < kh) {
                const size_t o = (size_t)c * kh + n2;
                const float v = st.cem[o];
                const float gg = g[s] + st.le * (l2 ? v : sgn(v));
                lpart += l2 ? 0.5f * st.le * v * v : st.le * fabsf(v);
                float ms = st.mscem[o];
                ms += (gg * gg - ms) * (1.f - st.rho);  // TF dense ApplyRMSProp
                st.mscem[o] = ms;
                st.cem[o] = v - st.lr * gg / sqrtf(ms + st.eps);
            }
        }
        if (c0 == 0 && lane == 0) {
            const float v = st.icb[c];
            const float gg = gi + st.lb * (l2 ? v : sgn(v));
            lpart += l2 ? 0.5f * st.lb * v * v : st.lb * fabsf(v);
            float ms = st.msicb[c];
            ms += (gg * gg - ms) * (1.f - st.rho);
            st.msicb[c] = ms;
            st.icb[c] = v - st.lr * gg / sqrtf(ms + st.eps);
        }
    }
    if (loss_out) {
        lpart = wave_sum(lpart);
        if (lane == 0 && lpart != 0.f) loss_add_spread(loss_out, lpart);
    }
}

// one batch of the generic sparse view: G1 (+ G2 without parities) in front of the pair launch, G3 + G4 behind it (csrc/vbpr_step.hip)
void vbpr_gen_front(const tkr_vbpr_state& st, const VbprBatch& bt, const VbprCarve& c, float* loss, hipStream_t s) {
    hipLaunchKernelGGL(vbpr_gen_project_kernel, dim3(bt.B), dim3(256), 0, s, st, bt.ti, bt.tj, bt.B, c.P, c.Q, bt.tu, bt.tp, c.ab2, c.Wm, loss);
    if (bt.tp) return;                                  // with K1's per-triplet parities the projection also scored the triplet
    vbpr_team_dispatch(bt.B, [&](auto team, auto big) {
        constexpr int T = decltype(team)::value;
        hipLaunchKernelGGL((vbpr_gen_occur_kernel<T, decltype(big)::value>), dim3(vbpr_grid(bt.B, T)), dim3(T * 64), 0, s, st, bt.rec, bt.occ2, bt.occt,
                           bt.hdr4, bt.B, c.Q, c.ab2, c.P, c.Wm, loss);
    });
}
void vbpr_gen_back(const tkr_vbpr_state& st, const VbprBatch& bt, const VbprCarve& c, float* loss, hipStream_t s) {
    vbpr_team_dispatch(bt.B, [&](auto team, auto big) {
        constexpr int T = decltype(team)::value;
        hipLaunchKernelGGL((vbpr_gen_rows_kernel<T, decltype(big)::value>), dim3(vbpr_grid(bt.B, T)), dim3(T * 64), 0, s, st, bt.rec, bt.occ2, bt.occt,
                           bt.hdr4, c.s_buf, c.t_buf, c.P, c.Wm, c.Aw, c.ab);
    });
    hipLaunchKernelGGL(vbpr_gen_sdense_kernel, dim3((st.d + 3) / 4), dim3(256), 0, s, st, c.Aw, c.ab, loss);
}
void vbpr_wide_update(const tkr_vbpr_state& st, const VbprBatch& bt, const VbprCarve& c, float* loss, hipStream_t s) {
    const int n_row_blocks = vbpr_grid(bt.B, 4), n_col_blocks = vbpr_wide_col_blocks(st.d);
    hipLaunchKernelGGL(vbpr_wide_update_kernel, dim3(n_row_blocks + n_col_blocks), dim3(256), 0, s, st, bt.rec, bt.occ2, bt.occt, bt.hdr4, c.s_buf, c.t_buf, c.P,
                       c.Wm, bt.colh, bt.cent, n_row_blocks, n_col_blocks, loss, bt.B);
}

}  // namespace tkr
