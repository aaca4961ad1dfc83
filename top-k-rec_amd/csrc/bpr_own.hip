// K2o -- the persistent BPR step with OWNED item rows (round 4): the tables, versions and acknowledge protocol of K2f
// (csrc/bpr_flow.hip; sess.run([solver, obj]) of single/bpr.py:141 inside the loop of single/bpr.py:139-147, batch t+1 reads what
// batch t wrote), with the own-row chain that set K2f's pace taken out of memory.
//
// The own-row chain.  A popular item is updated in (nearly) every batch; under K2f the task of batch t+1 starts its arithmetic
// once the row written by the task of batch t has made the trip write-through store -> memory -> polling load of another CU.  Here
// every item row r has an OWNER: workgroup r % n_owner (one workgroup per CU, all resident).  K1 lays the
// item tasks of a batch out in (owner, row) order and names every owner's run (tkr_sample_plan_owned: `ohdr`); the owner's waves
// take them in plan order from a queue in LDS (one LDS atomic per task), and the row, its RMSProp slot, bias and acknowledge totals
// stay in the owner's LDS from the row's first update of a launch on: the task of batch t+1 finds what the task of batch t left
// there -- before that task's acknowledge wait and write-through stores, which now only serve the row's PARTNERS.
//
// An item task reads the partner rows of an occurrence -- the user row and the OTHER item's row -- from the granule tables at their
// exact versions, as in K2f (flow_task.h run_task).  Measured 2.18 us per batch at the ML-10M shape against 2.75 for K2f on the same
// box.  What bounds it: throughput -- two to three memory round trips per task in series at 2-3 us apiece, ~700 tasks per batch over
// 3,072 waves; the dependency structure alone forces only 0.38 hand-offs per batch against K2f's 1.14 (scripts/chain_model.py,
// DESIGN.md K2o).  The scalar-exchange form with its scout wave measured 2.74 and was removed (DESIGN.md section 4, K2o table;
// source: git show 7a0cd86:top-k-rec_amd/csrc/bpr_own.hip).
//
// User tasks are handed out by tickets as in K2f, to the remaining waves of every workgroup.  The granule tables are written
// through at every update exactly as by K2f, so a launch leaves them complete (get / set, the exchange of csrc/sync.hip, a K2f
// launch all work on the same state), and a chunk may be cut into launches anywhere: a task whose row was not yet updated in THIS
// launch (prec[5] < first batch of the launch) loads it from the tables like K2f does.
//
// Progress.  Producers of a task sit in earlier batches.  Owner queues are taken in plan order by their own waves, tickets in plan
// order by the ticket waves, one task per wave at a time (no claim-ahead: a claimed task that nobody works on blocked the waves
// behind it).  Needs every workgroup resident (grid = n_owner <= CUs); every spin is bounded (status word), and the engine steps
// down to K2f when one runs out.
//
// Results are bitwise reproducible run to run (the item and user tasks sum like K2f).
#include "flow_task.h"
// s_sleep between two polls of an LDS word (a row's tag).  The polls are ds_read now (flow_task.h lds_peek; as
// flat loads each took a trip down the vector-memory path, which throttled them by accident): a wave that spins on LDS at full rate
// takes issue cycles from the two working waves of its SIMD.  Measured per batch in steady state / per 20-batch call, ML-10M shape:
// nap 0: 2.03 us / 112 us, 1: 2.00 / 105, 2: 1.98 / 101, 4: 1.95 / 99, 8: 1.98 / 98, 16: 2.01 / 99, 32: 2.12 / 102 (flat polls: 2.2 / 110).
#ifndef TKR_TAG_NAP
#define TKR_TAG_NAP 4
#endif
#ifdef TKR_PLAN_STAMP         // profiling build (scripts/probe_short.py): the phases of the planner prologue, workgroup 0
namespace tkr { __device__ unsigned long long own_k1_prof[32]; }
#define K1_STAMP(i) do { if (blockIdx.x == 0 && threadIdx.x == 0) tkr::own_k1_prof[i] = __builtin_amdgcn_s_memrealtime(); } while (0)
#define K1_STAMP_ITEMS(i) do { if (blockIdx.x == 0 && threadIdx.x == 256) tkr::own_k1_prof[i] = __builtin_amdgcn_s_memrealtime(); } while (0)
#endif
#include "plan_parts.h"

namespace tkr {

// ---- the planner prologue (PLAN = true): K1 of a SHORT call inside the step's own launch -----------------------------------------
// A short call (the driver's `--steps 20`: one launch of 20 batches) used to be five launches -- sample_plan, resolve_flow_wide,
// commit, this kernel, own_loss -- and on a cold one-shot process the HOST's launch path (8-14 us per launch), not the device, was
// what the call waited for.  Here workgroups 0 .. n_plan-1 each plan one batch with the very device functions of csrc/sampler.hip
// (csrc/plan_parts.h; same words, bit for bit: tests/test_gpu_flow.py test_flow_plan_bit_exact runs this form too):
//   phase A   draw, sorts, task heads, touch bits (atomics)          -> arrive at kCtlPlanA, wait for all n_plan
//   phase B   versions from the complete bitmap, records (sc1 stores) -> arrive at kCtlPlanB, wait
//   commit    the rows whose first task of the call is mine: counter += touches, bitmap words back to zero
//   done      arrive at kCtlPlanC; EVERY workgroup waits for it, drops its L1 (one agent-scope acquire) and runs the step.
// All workgroups of the launch are resident (the step needs that anyway), so the barriers complete; every spin is bounded.
struct PlanArgs {
    const int32_t *tr_users, *row_ptr, *pos_cols, *cols_sorted;
    int32_t *ucnt, *icnt;
    uint32_t *touch_u, *touch_i;
    int32_t *out_u, *out_i, *out_j;
    int4* task;
    int2* occ;
    int32_t* occt;
    int4 *prec, *pocc;
    int32_t* ohdr;
    uint64_t seed, first_triplet;
    uint32_t n_tr, n_items;
    int n_plan, npad_items, own_words, reg_sort_ok;
};

// thread 0 adds the workgroup's arrival (if `arrive`) and polls until n have arrived; -> false when a bounded spin ran out (uniform)
template <int NAP>
__device__ __forceinline__ bool plan_rendezvous(uint32_t* counter, uint32_t n, bool arrive, uint32_t* ctl, volatile uint32_t* flag) {
    if (threadIdx.x == 0) {
        if (arrive) __hip_atomic_fetch_add(counter, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        uint32_t waited = 0, ok = 1u;
        while (ld_u32(counter) < n) {
            __builtin_amdgcn_s_sleep(NAP);                 // NAP x 64 clocks between polls (up to 256 pollers of one word: not a hot loop)
            if (spin_fail(waited, ctl, 0)) { ok = 0u; break; }
        }
        lds_poke(flag, ok);
    }
    __syncthreads();
    const bool ok = lds_peek(flag) != 0u;
    __syncthreads();                                   // (the flag word is reused by the next rendezvous)
    return ok;
}

constexpr uint32_t kOwnInvalid = 0xffffffffu;

// LDS of the planner prologue's two phases (they follow each other in the same bytes); the mirror of csrc/plan_parts.h lies behind
__host__ __device__ inline size_t plan_scratch_bytes(int B, int npad_items, int n_owner, int own_words) {
    size_t a = (size_t)npad_items * 8 + (kWideThreads / TKR_WAVE + 1) * 4;
    if (a < (size_t)(256 + 512) * 8 + 64) a = (size_t)(256 + 512) * 8 + 64;                  // plan_phase_a_split
    const size_t pb = (size_t)3 * B * 20 + (size_t)4 * n_owner * (own_words + 1) + (kWideThreads / TKR_WAVE + 1) * 4 + 16 + (size_t)3 * B * 32;    // plan_phase_b_wide_lds
    return ((a > pb ? a : pb) + 15) & ~(size_t)15;
}

// int4 number `idx16` of the plan's records.  PLAN (the records were written by other workgroups of THIS launch): past the L1
template <bool PLAN>
__device__ __forceinline__ int4 plan_ld(const int4* __restrict__ prec, const __amdgpu_buffer_rsrc_t& prec_r, size_t idx16) {
    if constexpr (PLAN) {
        const v4u x = __builtin_amdgcn_raw_buffer_load_b128(prec_r, (int)(idx16 * 16), 0, kAuxLoad);
        return make_int4((int)x.x, (int)x.y, (int)x.z, (int)x.w);
    } else {
        return prec[idx16];
    }
}
constexpr int kDotWin = 1024;            // ring of "queue position p has run" marks (power of two; see the item tasks' loop)

struct OwnQueue {                        // head of the workgroup's LDS block
    uint32_t head;                       // next position of the owner queue
    uint32_t total;                      // item tasks of this owner in the launch
    uint32_t arrival;
    uint32_t head_batch;                 // a batch <= the batch of position `head`
};

// the owner queue: position -> (batch, slot) through the prefix sums of the per-batch run lengths
struct QueueMap {
    const uint32_t* pre;                 // [nb + 1 + 64]: pre[0] = 0, pre[b + 1] = tasks up to and including batch b; padding 0xffffffff
    const uint32_t* start;               // [nb]: first slot of the owner's run in batch b
    uint32_t slots_per_batch;            // 3B
    // record index of position pos (counted from the launch's first batch); cur: a batch <= the position's, moved to it
    __device__ __forceinline__ uint32_t locate(uint32_t pos, uint32_t& cur, int lane) const {
        uint32_t before;
        for (;;) {
            const uint32_t v = pre[cur + 1 + lane];
            const unsigned long long m = __ballot(v > pos);
            if (m) {
                const int f = __ffsll((long long)m) - 1;
                before = f ? (uint32_t)bcast_i((int)v, f - 1) : pre[cur];
                cur += f;
                break;
            }
            cur += TKR_WAVE;
        }
        return cur * slots_per_batch + start[cur] + (pos - before);
    }
};

// user tasks: tickets over the slots [0, B) of every batch (a batch's user tasks come first; what else sits there is skipped)
template <bool PLAN>
struct UserTicketSrc {
    uint32_t ticket;
    int home, queues;                    // queues = min(32, ticket waves of the grid): every queue has a wave
    uint32_t total;                      // nb * B
    uint32_t B;
    const int4* __restrict__ prec;       // record 0 of the launch's first batch
    __amdgpu_buffer_rsrc_t prec_r;       // ... as a buffer (PLAN)
    __device__ __forceinline__ void prefetch(NextTask& nx, int lane) {
        const u64 i64 = (u64)(uint32_t)bcast_i((int)ticket, 0) * (uint32_t)queues + (uint32_t)home;
        const uint32_t idx = i64 < total ? (uint32_t)i64 : 0xffffffffu;
        nx.have = true;
        nx.w = make_int4(0, 0, 0, 0);
        if (idx == 0xffffffffu) { nx.idx = idx; return; }
        nx.idx = idx + 2u * B * (idx / B);
        if (lane < 8) nx.w = plan_ld<PLAN>(prec, prec_r, (size_t)nx.idx * 8 + lane);
    }
};

// ---- the own row of an item task ------------------------------------------------------------------------------------------------
// LDS layout of a resident row: [kp] values, [kp] slots, {bias, its slot, expect[0..3], -, -}
template <int NP>
__device__ __forceinline__ void lds_row_read(const float* row, int lane, bool sgd, float (&own)[2 * NP], float (&ms)[2 * NP], Own& o) {
    constexpr int KP = NP * 128;
#pragma unroll
    for (int q = 0; q < NP; ++q) {
        const float2 a = *reinterpret_cast<const float2*>(row + q * 128 + 2 * lane);
        own[2 * q] = a.x; own[2 * q + 1] = a.y;
        if (!sgd) {
            const float2 m = *reinterpret_cast<const float2*>(row + KP + q * 128 + 2 * lane);
            ms[2 * q] = m.x; ms[2 * q + 1] = m.y;
        }
    }
    const float4 t = *reinterpret_cast<const float4*>(row + 2 * KP);
    const float2 t2 = *reinterpret_cast<const float2*>(row + 2 * KP + 4);
    o.b = t.x; o.msb = t.y;
    o.exp[0] = __float_as_uint(t.z); o.exp[1] = __float_as_uint(t.w);
    o.exp[2] = __float_as_uint(t2.x); o.exp[3] = __float_as_uint(t2.y);
}

struct ItemRow {                         // where the own row of an item task is
    const u64 *own_p, *own_ms, *own_tail;     // the tables, at the version read
    const uint32_t* own_rd;
    uint32_t ver;
    bool from_lds;                       // an earlier task of this launch updated the row: it is (or will be) in LDS
    const volatile uint32_t* tag;        // the row's version word in LDS
    const float* row;                    // the row's slot in LDS
    int halves;                          // 16-byte halves of a tail in the tables
    // A copy of the row's acknowledge word taken beside the row, and whether there is one.  Always false since the loader that took
    // it was removed; the test in item_own_wait stays because dropping it changes how the kernel's registers are allocated.
    bool rd_staged;
    uint32_t rd_val;
};

// the task's way: wait for the row (LDS: the task before it in the chain; tables: only at a launch's first touch), then the acknowledge word
template <int NP>
__device__ __forceinline__ bool item_own_wait(const FlowTables& T, int lane, const ItemRow& r, bool sgd, float (&own)[2 * NP], float (&ms)[2 * NP],
                                              Own& o, uint32_t* ctl, uint32_t& spins) {
    if (r.from_lds) {
        uint32_t waited = 0;
        while (lds_peek(r.tag) != r.ver) {
#if TKR_TAG_NAP > 0
            __builtin_amdgcn_s_sleep(TKR_TAG_NAP);
#endif
            if (spin_fail(waited, ctl, 0)) {
                if (waited >= kSpinLimit && lane == 0 && atomicCAS(ctl + kCtlDebug, 0u, 4u) == 0u) {
                    ctl[kCtlDebug + 1] = lds_peek(r.tag); ctl[kCtlDebug + 3] = r.ver;
                }
                return false;
            }
        }
        spins += waited;
        asm volatile("" ::: "memory");                  // the row is read AFTER its tag
        lds_row_read<NP>(r.row, lane, sgd, own, ms, o);
        o.ok = true;
        if (r.rd_staged) {
            o.rd = r.rd_val;
            return true;
        }
    }
    return flow_own<NP>(T, lane, r.own_p, r.own_ms, r.own_tail, r.own_rd, r.ver, own, ms, o, sgd, ctl, spins, r.halves);   // o.ok: only rd is loaded
}

// an item task (csrc/flow_task.h run_task: both partner rows of an occurrence read from the tables like K2f does) takes its own row
// the way above and never prefetches a record
template <int NP>
struct LdsOwnStep {
    const FlowTables& T;
    int lane;
    const ItemRow& r;
    bool sgd;
    uint32_t* ctl;
    uint32_t& spins;
    __device__ __forceinline__ bool operator()(float (&own)[2 * NP], float (&ms)[2 * NP], Own& o) {
#ifdef TKR_OWN_PROF
        o.t_own0 = __builtin_amdgcn_s_memtime();
        const bool ok = item_own_wait<NP>(T, lane, r, sgd, own, ms, o, ctl, spins);
        o.t_own1 = __builtin_amdgcn_s_memtime();
        return ok;
#else
        return item_own_wait<NP>(T, lane, r, sgd, own, ms, o, ctl, spins);
#endif
    }
};
struct NoFeed {
    __device__ __forceinline__ void prefetch(NextTask& nx, int) { nx.have = true; }
};

// the new row from the old one and the gradient (TF SparseApplyRMSProp, momentum 0: single/bpr.py:100; or old/methods/bpr.py:57-61)
template <int NP>
__device__ __forceinline__ void own_update(const tkr_flow_state& st, bool sgd, const float (&own)[2 * NP], const float (&ms)[2 * NP],
                                           const Own& o, const float (&g)[2 * NP], float gb, float (&pn)[2 * NP], float (&mn)[2 * NP],
                                           float& bn, float& mbn) {
    constexpr int NE = 2 * NP;
    if (sgd) {
#pragma unroll
        for (int e = 0; e < NE; ++e) { pn[e] = own[e] - st.lr * g[e]; mn[e] = 0.f; }
        bn = o.b - st.lr * gb;
        mbn = o.msb;
    } else {
#pragma unroll
        for (int e = 0; e < NE; ++e) {
            mn[e] = st.rho * ms[e] + (1.f - st.rho) * g[e] * g[e];
            pn[e] = own[e] - st.lr * g[e] * __builtin_amdgcn_rsqf(mn[e] + st.eps);
        }
        mbn = st.rho * o.msb + (1.f - st.rho) * gb * gb;
        bn = o.b - st.lr * gb * __builtin_amdgcn_rsqf(mbn + st.eps);
    }
}

// version ver+1 lands on the buffer that held ver-1 (ver-3 with four buffers): wait until every reader of that version has
// acknowledged, then write through
template <int NP>
__device__ __forceinline__ bool own_publish(int lane, bool is_item, uint32_t bmask, bool sgd, u64* tabP, u64* tabM, u64* tabT, size_t woff,
                                            size_t n_rows, int row, int rowk, uint32_t ver, int n_occ, Own& o, const uint32_t* own_rd,
                                            const float (&pn)[2 * NP], const float (&mn)[2 * NP], float bn, float mbn, uint32_t* ctl,
                                            uint32_t& spins, uint32_t readers_per_occ) {
    const uint32_t nv = ver + 1u;
    const uint32_t expect = pick_exp(o, (ver + 1u) & bmask);            // readers of the version that buffer holds now
    uint32_t waited = 0;
    while ((int32_t)(o.rd - expect) < 0) {
        if (spin_fail(waited, ctl)) {
            if (waited >= kSpinLimit && lane == 0 && atomicCAS(ctl + kCtlDebug, 0u, 2u) == 0u) {
                ctl[kCtlDebug + 1] = o.rd; ctl[kCtlDebug + 2] = expect; ctl[kCtlDebug + 3] = ver; ctl[kCtlDebug + 4] = (uint32_t)rowk;
            }
            return false;
        }
        o.rd = ld_u32(own_rd);
    }
    spins += waited;
#ifdef TKR_OWN_PROF
    o.t_ack = __builtin_amdgcn_s_memtime();
#endif
    store_row<NP>(tabP + woff, lane, pn, nv);
    if (!sgd) store_row<NP>(tabM + woff, lane, mn, nv);
    store_tail(tabT, n_rows, row, bmask, lane, is_item, bn, mbn, o, ver, n_occ, readers_per_occ);
    return true;
}

// threads per workgroup: 12 waves at k <= 128 (<= 168 registers), 8 at k <= 256; launch bounds ask for one workgroup per CU
constexpr int own_threads(int np) { return np == 1 ? 768 : 512; }

template <int NP, bool PLAN = false>
__global__ __launch_bounds__(own_threads(NP), own_threads(NP) / 256) void bpr_own_kernel(
    tkr_flow_state st, const int4* __restrict__ prec /*record 0 of the first batch to run*/, const int4* __restrict__ pocc,
    const int32_t* __restrict__ occt, const int32_t* __restrict__ ohdr /*[n_owner][ohdr_stride], at the first batch to run*/, int ohdr_stride,
    int first_batch, int nb, int B, int n_owner, int owner_waves, uint32_t tune, uint32_t* __restrict__ ctl, float* __restrict__ loss_out,
    u64* __restrict__ xch /*per-task loss slots [batches of the plan][B][2], at batch 0 of the plan*/, uint32_t epoch, PlanArgs pa) {
    constexpr int TPB = own_threads(NP);
    constexpr int NE = 2 * NP;
    constexpr int KP = NP * 128;
    constexpr int ROWF = 2 * KP + 8;                                  // floats per resident row
    const int lane = threadIdx.x & (TKR_WAVE - 1), wave = threadIdx.x / TKR_WAVE;
    FlowTables T;
    T.tune = 0u;
    T.kp = KP;
    T.ustride = (size_t)st.n_users * T.kp;
    T.istride = (size_t)st.n_items * T.kp;
    T.imask = st.item_bufs == 4 ? 3u : 1u;
    const int item_halves = tail_halves(T.imask);
    T.U = reinterpret_cast<u64*>(st.U); T.msU = reinterpret_cast<u64*>(st.msU); T.tailU = reinterpret_cast<u64*>(st.tailU);
    T.V = reinterpret_cast<u64*>(st.V); T.msV = reinterpret_cast<u64*>(st.msV); T.tailV = reinterpret_cast<u64*>(st.tailV);
    T.rdU = st.rdU; T.rdV = st.rdV;
    const bool sgd = st.opt == 1;
    const bool want_loss = loss_out != nullptr;

    // ---- the workgroup's LDS: queue head | prefix sums | run starts | row tags | position marks | rows
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    OwnQueue* q = reinterpret_cast<OwnQueue*>(smem);
    uint32_t* pre = reinterpret_cast<uint32_t*>(smem + sizeof(OwnQueue));           // [nb + 1 + 64]
    uint32_t* start = pre + nb + 1 + TKR_WAVE;                                         // [nb]
    const int rows_here = (st.n_items + n_owner - 1) / n_owner;
    uint32_t* tags = start + nb;                                                       // [rows_here]
    uint32_t* dotmark = tags + rows_here;                                              // [kDotWin]: position + 1 of the task that has run
    float* rows = reinterpret_cast<float*>(smem + ((sizeof(OwnQueue) + (size_t)4 * (2 * nb + 1 + TKR_WAVE + rows_here + kDotWin) + 15) & ~(size_t)15));

    // owner number = workgroup number (every workgroup is resident: which CU it sits on means nothing).  The first ticket of a user-task
    // wave goes out NOW, beside the loads of the queue header: a launch used to start with three trips in series -- an arrival
    // counter, the header, the first ticket -- in front of every short call.
    const uint32_t me = blockIdx.x;
    bool alive = true;
    int commit_key = -1, commit_total = 0;       // PLAN: the row this thread commits at the end of the kernel (a task's row word), its touches
#ifdef TKR_PLAN_STAMP        // scripts/probe_short.py with a -DTKR_PLAN_STAMP build: s_memrealtime (100 MHz) of workgroups 0 and 255 at the prologue's phases
#define PLAN_STAMP(i) do { if ((me == 0 || me == gridDim.x - 1) && threadIdx.x == 0) reinterpret_cast<u64*>(ctl + kCtlProf)[(me ? 16 : 0) + (i)] = __builtin_amdgcn_s_memrealtime(); } while (0)
#else
#define PLAN_STAMP(i) do { } while (0)
#endif
    PLAN_STAMP(0);
    // what of the queue header does not come from the plan (before the prologue: a workgroup that plans nothing only waits there)
    for (int b = threadIdx.x; b < TKR_WAVE; b += TPB) pre[nb + 1 + b] = 0xffffffffu;
    for (int s = threadIdx.x; s < rows_here; s += TPB) tags[s] = kOwnInvalid;
    for (int s = threadIdx.x; s < kDotWin; s += TPB) dotmark[s] = 0u;
    if constexpr (PLAN) {
        static_assert(TPB == kWideThreads, "phase B of the planner is one thread per task slot");
        unsigned char* scratch = reinterpret_cast<unsigned char*>(rows);                 // the rows' region: no row is resident yet
        volatile uint32_t* flag = &q->arrival;
        const uint32_t n_plan = (uint32_t)pa.n_plan;
        int4 ct = make_int4(-1, 0, 0, 0);                   // this thread's task of the batch, for K1c below
        int cprev = 0, ctotal = 0;
        if (me < n_plan) {
            const int b = (int)me, n3 = 3 * B;
            int4* task_b = pa.task + (size_t)b * n3;
            int2* occ_b = pa.occ + (size_t)b * n3;
            int32_t* occt_b = pa.occt + (size_t)b * n3;
            const bool split = pa.reg_sort_ok != 0 && pa.npad_items == 512 && B > 128;
            const PlanMirror mir = plan_mirror(scratch + plan_scratch_bytes(B, pa.npad_items, n_owner, pa.own_words), B);      // behind both phases' own scratch
            if (split)                                       // the common short call (batch 129 .. 256): users and items side by side
                plan_phase_a_split<TPB>(scratch, b, pa.tr_users, pa.n_tr, pa.row_ptr, pa.pos_cols, pa.cols_sorted, pa.n_items, pa.seed,
                                        pa.first_triplet + (uint64_t)b * (uint64_t)B, B, pa.out_u + (size_t)b * B, pa.out_i + (size_t)b * B,
                                        pa.out_j + (size_t)b * B, task_b, occ_b, occt_b, pa.touch_u, pa.touch_i, mir);
            else
                plan_phase_a<TPB, 256>(scratch, b, pa.tr_users, pa.n_tr, pa.row_ptr, pa.pos_cols, pa.cols_sorted, pa.n_items, pa.seed,
                                       pa.first_triplet + (uint64_t)b * (uint64_t)B, B, pa.npad_items, pa.out_u + (size_t)b * B, pa.out_i + (size_t)b * B,
                                       pa.out_j + (size_t)b * B, task_b, occ_b, occt_b, pa.touch_u, pa.touch_i, pa.reg_sort_ok != 0);
            PLAN_STAMP(1);
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");                             // the touch atomics of every wave are out
            __syncthreads();
            PLAN_STAMP(2);
            alive = plan_rendezvous<4>(ctl + kCtlPlanA, n_plan, true, ctl, flag);
            PLAN_STAMP(3);
            if (alive) {
                if (split)
                    plan_phase_b_wide<true, true>(scratch, b, B, task_b, occ_b, occt_b, pa.ucnt, pa.icnt, pa.touch_u, pa.touch_i, pa.pocc + (size_t)b * n3,
                                                  pa.prec + (size_t)b * n3 * 8, n_owner, pa.ohdr, ohdr_stride, pa.own_words, ct, cprev, ctotal, mir);
                else
                    plan_phase_b_wide<true, false>(scratch, b, B, task_b, occ_b, occt_b, pa.ucnt, pa.icnt, pa.touch_u, pa.touch_i, pa.pocc + (size_t)b * n3,
                                                   pa.prec + (size_t)b * n3 * 8, n_owner, pa.ohdr, ohdr_stride, pa.own_words, ct, cprev, ctotal);
                PLAN_STAMP(4);
            }
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");                             // bitmap reads returned, record stores in memory
            __syncthreads();
            PLAN_STAMP(5);
        }
        // (a planner that gave up still arrives: the others then see the status word instead of spinning out one by one)
        alive = plan_rendezvous<12>(ctl + kCtlPlanC, n_plan, me < n_plan, ctl, flag) && alive;
        PLAN_STAMP(8);
        // every planner is past its reads of the bitmap: K1c (the rows whose first task of the call is this thread's get the call's
        // touches added to their counters, their bitmap words zeroed) may go out -- atomics and stores that nobody in this launch
        // reads.  They go out at the END of the kernel: issued here they sat in front of the queue set-up's loads in the planners'
        // memory queues (set-up 3.0 us on a planner against 1.2 elsewhere, and the planners own rows like everybody else).
        commit_key = (alive && me < n_plan && (int)threadIdx.x < 3 * B && ct.x != -1 && cprev == -1) ? ct.x : -1;
        commit_total = ctotal;
        // No acquire fence here (measured 4.5 us for one lane's buffer_inv, 14 for every wave's): the plan words other CUs wrote went
        // out write-through before they arrived (sc1 stores + vmcnt(0)), the L2s see each other's writes, and THIS CU's L1 -- dropped
        // at the start of the launch -- has never held a line of prec / pocc / ohdr: nothing in front of this point loads from
        // them.  The records and owner runs are read past the L1 all the same (plan_ld below).
        PLAN_STAMP(9);
    }
    const bool ticket_wave = wave > owner_waves;
    const int tw = wave - owner_waves - 1, n_tw = TPB / TKR_WAVE - owner_waves - 1;
    const int queues = min(kQueues, max(n_tw, 1) * (int)gridDim.x);
    const int home = ticket_wave ? (int)((me * (uint32_t)n_tw + (uint32_t)tw) % (uint32_t)queues) : 0;
    uint32_t ticket = 0;
    if (ticket_wave) ticket = grab_issue(ctl, lane, home);
    for (int b = threadIdx.x; b < nb; b += TPB) {
        uint32_t h = 0u;
        if (me < (uint32_t)n_owner) {
            if constexpr (PLAN) h = (uint32_t)__hip_atomic_load(ohdr + (size_t)me * ohdr_stride + b, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            else h = (uint32_t)ohdr[(size_t)me * ohdr_stride + b];
        }
        start[b] = h & 0xffffu;
        pre[b + 1] = h >> 16;
    }
    __syncthreads();
    if (wave == 0) {                                                                   // inclusive scan of the run lengths (nb <= 512)
        const int per = (nb + TKR_WAVE - 1) / TKR_WAVE;
        const int b0 = min(lane * per, nb), b1 = min(b0 + per, nb);
        uint32_t mine = 0;
        for (int b = b0; b < b1; ++b) mine += pre[b + 1];
        uint32_t incl = mine;
#pragma unroll
        for (int d = 1; d < TKR_WAVE; d <<= 1) {
            const uint32_t up = (uint32_t)__shfl_up((int)incl, d);
            if (lane >= d) incl += up;
        }
        uint32_t run = incl - mine;
        for (int b = b0; b < b1; ++b) { run += pre[b + 1]; pre[b + 1] = run; }
        if (lane == TKR_WAVE - 1) { q->total = incl; q->head = 0u; q->head_batch = 0u; }
        if (lane == 0) pre[0] = 0u;
    }
    __syncthreads();

    PLAN_STAMP(10);
    uint32_t spins = 0;
#ifdef TKR_OWN_PROF
    u64 prof[16] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    u64 tprev = __builtin_amdgcn_s_memtime();
#endif
    const QueueMap qm{pre, start, 3u * (uint32_t)B};
    const __amdgpu_buffer_rsrc_t prec_r = row_rsrc(prec, PLAN ? nb * 3 * B * 128 : 16);
    const uint32_t q_total = q->total;

    // the own row of the item task whose record is w
    auto item_row = [&](const int4 w, ItemRow& r, int& row, int& slot) {
        const int rowk = bcast_i(w.x, 0);
        const uint32_t ver = (uint32_t)bcast_i(w.y, 0);
        const int prev = bcast_i(w.y, 1);
        row = rowk & 0x7fffffff;
        slot = row / n_owner;
        const size_t roff = (size_t)(ver & T.imask) * T.istride + (size_t)row * T.kp;
        r.own_p = T.V + roff; r.own_ms = T.msV + roff;
        r.own_tail = T.tailV + ((size_t)(ver & T.imask) * st.n_items + row) * (2 * item_halves);
        r.own_rd = T.rdV + (T.imask + 1u) * (size_t)row + ((ver + 1u) & T.imask);
        r.ver = ver;
        r.from_lds = prev >= first_batch;
        r.tag = tags + slot;
        r.row = rows + (size_t)slot * ROWF;
        r.halves = item_halves;
        r.rd_staged = false;
        r.rd_val = 0u;
    };

    constexpr uint32_t kItemReaders = 2u;                         // an occurrence's user task and its other item's task read an item row
    if (wave <= owner_waves) {
        // ================= item tasks of the rows this workgroup owns =================
        uint32_t cur = 0;
        while (alive) {
            uint32_t pos = 0;
            if (lane == 0) pos = atomicAdd(&q->head, 1u);
            pos = (uint32_t)bcast_i((int)pos, 0);
            if (pos >= q_total) break;
            const uint32_t idx = qm.locate(pos, cur, lane);
            if (lane == 0) atomicMax(&q->head_batch, cur);
            int4 w = make_int4(0, 0, 0, 0);
            if (lane < 8) w = plan_ld<PLAN>(prec, prec_r, (size_t)idx * 8 + lane);
#ifdef TKR_OWN_PROF
            asm volatile("" : "+v"(w.x) :: "memory");
            const u64 t0 = __builtin_amdgcn_s_memtime();
            prof[5] += t0 - tprev;
#endif
            ItemRow r;
            int row, slot;
            item_row(w, r, row, slot);
            const int rowk = bcast_i(w.x, 0);
            const uint32_t ver = r.ver;
            const int n_occ = bcast_i(w.z, 0), first = bcast_i(w.w, 0);
            const size_t woff = (size_t)((ver + 1u) & T.imask) * T.istride + (size_t)row * T.kp;
            float* lrow = rows + (size_t)slot * ROWF;

            float own[NE], ms[NE], g[NE];
#pragma unroll
            for (int e = 0; e < NE; ++e) { g[e] = 0.f; ms[e] = 0.f; }
            Own o = {};
            float gb = 0.f;
            o.ok = r.from_lds;                                           // flow_fetch then leaves the own row alone
            NextTask nx;
            nx.idx = 0u; nx.w = make_int4(0, 0, 0, 0); nx.have = true;
            NoFeed feed;
            LdsOwnStep<NP> own_step{T, lane, r, sgd, ctl, spins};
            float loss_lane = 0.f;
            alive = run_task<NP, true, NoFeed, LdsOwnStep<NP>, 4>(st, T, lane, n_occ, first, w, pocc, r.own_p, r.own_ms, r.own_tail, ver, own, ms, o, g,
                                                                  gb, loss_lane, false, sgd, ctl, spins, nx, feed, own_step);
            if (!alive) break;
            // (the position marks and head_batch were read by the scout of the scalar-exchange form; the marks' words stay in the LDS
            // budget, which sets the item counts K2o takes)
            if (lane == 0) dotmark[pos & (kDotWin - 1)] = pos + 1u;
#ifdef TKR_OWN_PROF
            const u64 t1 = __builtin_amdgcn_s_memtime();
#endif
            float pn[NE], mn[NE], bn, mbn;
            own_update<NP>(st, sgd, own, ms, o, g, gb, pn, mn, bn, mbn);

            // the row's next task finds the new version HERE, now -- not behind the acknowledge wait and the trip through memory
#pragma unroll
            for (int qq = 0; qq < NP; ++qq) {
                *reinterpret_cast<float2*>(lrow + qq * 128 + 2 * lane) = make_float2(pn[2 * qq], pn[2 * qq + 1]);
                if (!sgd) *reinterpret_cast<float2*>(lrow + KP + qq * 128 + 2 * lane) = make_float2(mn[2 * qq], mn[2 * qq + 1]);
            }
            if (lane == 0) {
                const uint32_t rb = ver & T.imask, add = kItemReaders * (uint32_t)n_occ;
                *reinterpret_cast<float4*>(lrow + 2 * KP) = make_float4(bn, mbn, __uint_as_float(o.exp[0] + (rb == 0u ? add : 0u)),
                                                                        __uint_as_float(o.exp[1] + (rb == 1u ? add : 0u)));
                *reinterpret_cast<float2*>(lrow + 2 * KP + 4) =
                    make_float2(__uint_as_float(o.exp[2] + (rb == 2u ? add : 0u)), __uint_as_float(o.exp[3] + (rb == 3u ? add : 0u)));
            }
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");          // the row is in LDS before its tag says so
            if (lane == 0) lds_poke(tags + slot, ver + 1u);

            alive = own_publish<NP>(lane, true, T.imask, sgd, T.V, T.msV, T.tailV, woff, (size_t)st.n_items, row, rowk, ver, n_occ, o, r.own_rd, pn,
                                    mn, bn, mbn, ctl, spins, kItemReaders);
#ifdef TKR_OWN_PROF
            tprev = __builtin_amdgcn_s_memtime();
            prof[0] += o.t_own0 - t0; prof[1] += o.t_own1 - o.t_own0; prof[2] += t1 - o.t_own1;
            prof[3] += o.t_ack - t1; prof[4] += tprev - o.t_ack; prof[6] += 1; prof[7] += r.from_lds ? 1 : 0;
#endif
        }
    } else {
        // ================= user tasks, by ticket =================
        const uint32_t total = (uint32_t)nb * (uint32_t)B;
        NextTask nx;
        nx.idx = 0u; nx.w = make_int4(0, 0, 0, 0); nx.have = false;
        while (alive) {
            if (!nx.have) {
                UserTicketSrc<PLAN> first_feed{ticket, home, queues, total, (uint32_t)B, prec, prec_r};
                first_feed.prefetch(nx, lane);
                asm volatile("" : "+v"(nx.w.x), "+v"(nx.w.y), "+v"(nx.w.z), "+v"(nx.w.w) :: "memory");
            }
            const uint32_t idx = nx.idx;
            const int4 w = nx.w;
            if (idx == 0xffffffffu) break;
            nx.have = false;
            ticket = grab_issue(ctl, lane, home);                      // the ticket of the task after this one
            const int rowk = bcast_i(w.x, 0);
#ifdef TKR_OWN_PROF
            const u64 t0 = __builtin_amdgcn_s_memtime();
            prof[8] += t0 - tprev;
#endif
            if (rowk < 0) {                                             // an item task (its owner runs it) or an unused slot
#ifdef TKR_OWN_PROF
                tprev = t0;
#endif
                continue;
            }
            const uint32_t ver = (uint32_t)bcast_i(w.y, 0);
            const int n_occ = bcast_i(w.z, 0);
            const int first = bcast_i(w.w, 0);
            const int batch = bcast_i(w.x, 1);
            const int row = rowk;

            const size_t roff = (size_t)(ver & 1u) * T.ustride + (size_t)row * T.kp;
            const size_t woff = (size_t)((ver + 1u) & 1u) * T.ustride + (size_t)row * T.kp;
            const uint32_t* own_rd = T.rdU + 2 * (size_t)row + ((ver + 1u) & 1u);
            const u64* own_tail = T.tailU + ((size_t)(ver & 1u) * st.n_users + row) * 4;

            float own[NE], ms[NE], g[NE];
#pragma unroll
            for (int e = 0; e < NE; ++e) { g[e] = 0.f; ms[e] = 0.f; }
            Own o = {};
            float gb = 0.f, loss_lane = 0.f;
            UserTicketSrc<PLAN> feed{ticket, home, queues, total, (uint32_t)B, prec, prec_r};
            GlobalOwn<NP> own_step{T, lane, T.U + roff, T.msU + roff, own_tail, own_rd, ver, sgd, ctl, spins, 2};
            alive = run_task<NP, false, UserTicketSrc<PLAN>, GlobalOwn<NP>, 4>(st, T, lane, n_occ, first, w, pocc, T.U + roff, T.msU + roff, own_tail, ver,
                                                                         own, ms, o, g, gb, loss_lane, want_loss, sgd, ctl, spins, nx, feed, own_step);
            if (!alive) break;
#ifdef TKR_OWN_PROF
            const u64 t1 = __builtin_amdgcn_s_memtime();
#endif
            if (want_loss) {
                // A batch's loss is the sum over its ~250 user tasks.  As atomics on loss_out[batch] -- one word, one memory channel --
                // they cost 0.9 us of a 2.2 us batch (hardware fp32 atomics or a compare-and-swap loop alike: each is a memory
                // operation that the next task's first load waits behind).  Instead the task's sum goes to `xch` as ONE plain 8-byte
                // store {sum, epoch} in the slot of its record, and own_loss_kernel adds the slots of a batch up after the launch (fixed
                // order: the losses are bitwise reproducible).
                const float tot = wave_sum(loss_lane);
                if (lane == 0) {
                    const uint32_t slot = idx - (uint32_t)(batch - first_batch) * 3u * (uint32_t)B;     // user tasks: the first slots of a batch's 3B
                    // (write-through: the workgroup that adds the slots up -- own_loss_kernel, or the LAST one of this launch -- may sit on another XCD)
                    __hip_atomic_store(xch + ((size_t)batch * B + slot) * 2, ((u64)epoch << 32) | (u64)__float_as_uint(tot), __ATOMIC_RELAXED,
                                       __HIP_MEMORY_SCOPE_AGENT);
                }
            }
            float pn[NE], mn[NE], bn, mbn;
            own_update<NP>(st, sgd, own, ms, o, g, gb, pn, mn, bn, mbn);
            asm volatile("" : "+v"(nx.w.x), "+v"(nx.w.y), "+v"(nx.w.z), "+v"(nx.w.w));      // the next record is consumed before the stores go out
            alive = own_publish<NP>(lane, false, 1u, sgd, T.U, T.msU, T.tailU, woff, (size_t)st.n_users, row, rowk, ver, n_occ, o, own_rd, pn, mn,
                                    bn, mbn, ctl, spins, 2u);
#ifdef TKR_OWN_PROF
            tprev = __builtin_amdgcn_s_memtime();
            prof[9] += t1 - t0; prof[11] += o.t_ack - t1; prof[12] += tprev - o.t_ack; prof[13] += 1;
#endif
        }
    }

    if (lane == 0 && spins) atomicAdd(ctl + kCtlSpins, spins);
#ifdef TKR_OWN_PROF
    if (lane == 0)
        for (int qq = 0; qq < 16; ++qq) atomicAdd(reinterpret_cast<u64*>(ctl + kCtlProf) + qq, prof[qq]);
#endif
    // the last workgroup out puts the ticket words back to zero (as K2f: the next launch needs no memset)
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    PLAN_STAMP(11);
    if constexpr (PLAN) {
        if (commit_key != -1) plan_commit_first_touch(make_int4(commit_key, 0, 0, 0), -1, commit_total, pa.ucnt, pa.icnt, pa.touch_u, pa.touch_i);
    }
    const bool fold_loss = want_loss && (tune & 8u) != 0u;       // tune bit 3 (set by the host for short launches): the last workgroup out adds the losses up
    if (threadIdx.x == 0) {
        const bool last = __hip_atomic_fetch_add(ctl + kCtlLeave, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == gridDim.x - 1u;
        if (last) {
            for (int qq = 0; qq < kQueues; ++qq) ctl[qq * kQueueStride] = 0u;
            ctl[kCtlArrive] = 0u;
            ctl[kCtlLeave] = 0u;
            if constexpr (PLAN) { ctl[kCtlPlanA] = 0u; ctl[kCtlPlanB] = 0u; ctl[kCtlPlanC] = 0u; }
        }
        q->arrival = last ? 1u : 0u;
    }
    if (!fold_loss) return;
    // ---- the losses of a SHORT launch: the last workgroup out adds the per-task sums up, instead of a launch of own_loss_kernel behind
    // this one (4.4 us + a kernel boundary + a host launch, of a ~100 us call).  Every other workgroup has drained its stores (above)
    // before it arrived at kCtlLeave, and the slots are write-through.  Same summation order as own_loss_kernel, bit for bit: slot t
    // belongs to "thread" t & 255, a thread adds its slots in order, waves of 64 threads by wave_sum, (p0 + p1) + (p2 + p3).
    __syncthreads();
    if (q->arrival == 0u) return;
    for (int b = wave; b < nb; b += TPB / TKR_WAVE) {
        const int batch = first_batch + b;
        float part[4];
#pragma unroll
        for (int w = 0; w < 4; ++w) {
            float acc = 0.f;
            for (int t = w * TKR_WAVE + lane; t < B; t += 256) {
                const u64 g = __hip_atomic_load(xch + ((size_t)batch * B + t) * 2, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                if ((uint32_t)(g >> 32) == epoch) acc += __uint_as_float((uint32_t)g);
            }
            part[w] = wave_sum(acc);
        }
        if (lane == 0) loss_out[batch] = (part[0] + part[1]) + (part[2] + part[3]);
    }
}

// the losses of a launch's batches from the per-task sums its user tasks left in xch (row-read form): loss_out[b] = sum of the slots
// of batch b that carry this launch's epoch
__global__ __launch_bounds__(256) void own_loss_kernel(const u64* __restrict__ xch, int first_batch, int B, uint32_t epoch, float* __restrict__ loss_out) {
    __shared__ float part[4];
    const int b = first_batch + (int)blockIdx.x, lane = threadIdx.x & (TKR_WAVE - 1), wave = threadIdx.x / TKR_WAVE;
    float acc = 0.f;
    for (int s = threadIdx.x; s < B; s += 256) {
        const u64 g = xch[((size_t)b * B + s) * 2];
        if ((uint32_t)(g >> 32) == epoch) acc += __uint_as_float((uint32_t)g);
    }
    acc = wave_sum(acc);
    if (lane == TKR_WAVE - 1) part[wave] = acc;
    __syncthreads();
    if (threadIdx.x == 0) loss_out[b] = (part[0] + part[1]) + (part[2] + part[3]);       // ASSIGNED: a batch runs once (no fill in front of a short call)
}

static size_t own_lds_bytes(int np, int nb, int n_items, int n_owner) {
    const int rows_here = (n_items + n_owner - 1) / n_owner;
    const size_t head = (sizeof(OwnQueue) + (size_t)4 * (2 * nb + 1 + TKR_WAVE + rows_here + kDotWin) + 15) & ~(size_t)15;
    return head + (size_t)rows_here * (2 * np * 128 + 8) * 4;
}

// ... with the planner prologue: its scratch (phase A: sort keys + scan; phase B: the batch's occurrences, owner bitmaps) lies over the
// rows' region, which may be smaller (test shapes)
static size_t own_lds_bytes_planned(int np, int nb, int n_items, int n_owner, int B, int npad_items, int own_words) {
    const int rows_here = (n_items + n_owner - 1) / n_owner;
    const size_t head = (sizeof(OwnQueue) + (size_t)4 * (2 * nb + 1 + TKR_WAVE + rows_here + kDotWin) + 15) & ~(size_t)15;
    const size_t rows = (size_t)rows_here * (2 * np * 128 + 8) * 4;
    const size_t scratch = plan_scratch_bytes(B, npad_items, n_owner, own_words) + plan_mirror_lds(B);
    return head + (rows > scratch ? rows : scratch);
}

}  // namespace tkr

// workgroups (= owners) a process runs at once for factor width k when `share` processes split the device's CUs between them
// (share = 1: one workgroup per CU), or 0 when the item rows do not fit their owners' LDS
extern "C" int32_t tkr_bpr_own_owners_shared(int32_t n_items, int32_t k, int32_t share) {
    if (n_items <= 0 || k <= 0 || k > 256 || share <= 0) return 0;
    int dev = 0, cus = 0;
    if (hipGetDevice(&dev) != hipSuccess) return 0;
    if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || cus <= 0) return 0;
    const int owners = cus / share;
    if (owners <= 0) return 0;
    const int np = (k + 127) / 128;
    if (tkr::own_lds_bytes(np, 512, n_items, owners) > 160 * 1024) return 0;
    return owners;
}
extern "C" int32_t tkr_bpr_own_owners(int32_t n_items, int32_t k) { return tkr_bpr_own_owners_shared(n_items, k, 1); }

// one launch of the step on batches [first_batch, first_batch + n_batches); `pa` != nullptr: with the planner prologue (the caller has
// checked own_plan_fusable)
static int own_launch(const tkr_flow_state* st, const int32_t* prec, const int32_t* pocc, const int32_t* occt, const int32_t* ohdr,
                      int32_t ohdr_stride, int32_t n_owner, int32_t batch_size, int32_t first_batch, int32_t n_batches, uint32_t* ctl,
                      float* loss_out, int32_t owner_waves, void* xch, uint32_t epoch, const tkr::PlanArgs* pa, void* stream) {
    if (!st || !st->U || !st->V || !st->tailU || !st->tailV || !st->rdU || !st->rdV) return TKR_EINVAL;
    if (st->opt != 0 && st->opt != 1) return TKR_EINVAL;
    if (st->opt == 0 && (!st->msU || !st->msV)) return TKR_EINVAL;
    if (st->n_users <= 0 || st->n_items <= 0 || st->k <= 0) return TKR_EINVAL;
    if (st->k > 256) return TKR_EUNSUPPORTED;
    if (st->item_bufs != 0 && st->item_bufs != 2 && st->item_bufs != 4) return TKR_EINVAL;
    if (!xch || epoch == 0u) return TKR_EINVAL;
    if (!prec || !pocc || !occt || !ohdr || !ctl || batch_size <= 0 || n_batches < 0 || first_batch < 0 || n_owner <= 0) return TKR_EINVAL;
    if (ohdr_stride < first_batch + n_batches || n_batches > 512) return TKR_EINVAL;
    if (n_batches == 0) return TKR_OK;
    if ((uint64_t)(first_batch + n_batches) * 3u * (uint64_t)batch_size >= 0xffffffffull / 8) return TKR_EUNSUPPORTED;
    const int np = (st->k + 127) / 128;
    int dev = 0;
    TKR_CHECK(hipGetDevice(&dev));
    static int cached_cus[64];
    static bool attr_set[64][3];
    int cus;
    if (dev >= 0 && dev < 64 && cached_cus[dev] > 0) cus = cached_cus[dev];
    else {
        TKR_CHECK(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev));
        if (dev >= 0 && dev < 64) cached_cus[dev] = cus;
    }
    if (n_owner > cus) return TKR_EUNSUPPORTED;                    // every owner must be resident: one workgroup per CU
    size_t lds = tkr::own_lds_bytes(np, n_batches, st->n_items, n_owner);
    if (pa) lds = tkr::own_lds_bytes_planned(np, n_batches, st->n_items, n_owner, batch_size, pa->npad_items, pa->own_words);
    if (lds > 160 * 1024) return TKR_EUNSUPPORTED;
    const uint32_t tune = ((uint32_t)owner_waves >> 8) & 0xffu;     // experiment switches ride in bits 8..15
    owner_waves &= 0xff;
    // owner_waves bits 8 and 15 asked for the loader / consumer ring and the scalar exchange, bits 13 and 14 for 8 and 16 waves at
    // k <= 128: forms that were measured and lost, no longer built
    if ((tune & (1u | 128u)) || (np == 1 && (tune & (32u | 64u)))) return TKR_EUNSUPPORTED;
    if (pa && np != 1) return TKR_EINVAL;
    const int tpb = tkr::own_threads(np);
    const int waves = tpb / TKR_WAVE;
    // `ow` waves on the owner queue (waves 0 .. ow), the rest on user tickets
    int ow = owner_waves > 0 ? owner_waves : (waves == 12 ? 9 : 6);
    if (ow < 1) ow = 1;
    if (ow > waves - 2) ow = waves - 2;
    // a short launch adds its losses up itself (its last workgroup out); tune bit 1 (owner_waves bit 9): always own_loss_kernel
    const bool fold = loss_out && n_batches <= 64 && !(tune & 2u);
    const uint32_t ktune = (tune & ~8u) | (fold ? 8u : 0u);
    const void* fn = pa ? (const void*)tkr::bpr_own_kernel<1, true>
                   : np == 1 ? (const void*)tkr::bpr_own_kernel<1, false> : (const void*)tkr::bpr_own_kernel<2, false>;
    const int form = pa ? 2 : np - 1;
    if (lds > 64 * 1024 && !(dev >= 0 && dev < 64 && attr_set[dev][form])) {
        TKR_CHECK(hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
        if (dev >= 0 && dev < 64) attr_set[dev][form] = true;
    }
    // every owner must be RESIDENT (the dataflow inside a launch waits for workgroups that have to be running): asked of the runtime
    // once per kernel form and device, at the largest LDS size a launch may ask for (K2f had the query, K2o did not)
    static signed char fits[64][3];
    if (dev >= 0 && dev < 64 && fits[dev][form] == 0) {
        int per_cu = 0;
        TKR_CHECK(hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, fn, tpb, 160 * 1024));
        fits[dev][form] = per_cu >= 1 ? 1 : -1;
    }
    if (dev >= 0 && dev < 64 && fits[dev][form] < 0) return TKR_EUNSUPPORTED;
    hipStream_t s = (hipStream_t)stream;
    const int4* r4 = reinterpret_cast<const int4*>(prec) + (size_t)first_batch * 3 * batch_size * 8;      // record 0 of the first batch to run
    const int4* o4 = reinterpret_cast<const int4*>(pocc);
    ohdr += first_batch;
    const tkr::PlanArgs no_plan = {};
#define TKR_OWN_LAUNCH(NPV, PL)                                                                                                           \
    hipLaunchKernelGGL((tkr::bpr_own_kernel<NPV, PL>), dim3(n_owner), dim3(tkr::own_threads(NPV)), lds, s, *st, r4, o4, occt, ohdr, ohdr_stride,   \
                       first_batch, n_batches, batch_size, n_owner, ow, ktune, ctl, loss_out, static_cast<tkr::u64*>(xch), epoch, PL ? *pa : no_plan)
    if (pa) TKR_OWN_LAUNCH(1, true);
    else if (np == 1) TKR_OWN_LAUNCH(1, false);
    else TKR_OWN_LAUNCH(2, false);
#undef TKR_OWN_LAUNCH
    TKR_LAUNCH_CHECK();
    if (loss_out && !fold) {
        hipLaunchKernelGGL(tkr::own_loss_kernel, dim3(n_batches), dim3(256), 0, s, static_cast<const tkr::u64*>(xch), first_batch, batch_size, epoch,
                           loss_out);
        TKR_LAUNCH_CHECK();
    }
    return TKR_OK;
}

extern "C" int tkr_bpr_own_run(const tkr_flow_state* st, const int32_t* prec, const int32_t* pocc, const int32_t* occt, const int32_t* ohdr,
                               int32_t ohdr_stride, int32_t n_owner, int32_t batch_size, int32_t first_batch, int32_t n_batches,
                               uint32_t* ctl, float* loss_out, int32_t owner_waves, void* xch, uint32_t epoch, void* stream) {
    return own_launch(st, prec, pocc, occt, ohdr, ohdr_stride, n_owner, batch_size, first_batch, n_batches, ctl, loss_out, owner_waves, xch, epoch,
                      nullptr, stream);
}

// the same launch between two HIP events of the caller (nullable hipEvent_t, recorded on `stream`): whoever times the launch --
// bench.py's roofline -- does not come back through the host language between K1's launches, the event and this launch (a short
// call is ~130 us of device work; 20 us of interpreter between its launches leave the device idle)
extern "C" int tkr_bpr_own_run_between(void* ev_before, void* ev_after, const tkr_flow_state* st, const int32_t* prec, const int32_t* pocc,
                                       const int32_t* occt, const int32_t* ohdr, int32_t ohdr_stride, int32_t n_owner, int32_t batch_size,
                                       int32_t first_batch, int32_t n_batches, uint32_t* ctl, float* loss_out, int32_t owner_waves, void* xch,
                                       uint32_t epoch, void* stream) {
    if (ev_before) TKR_CHECK(hipEventRecord((hipEvent_t)ev_before, (hipStream_t)stream));
    const int rc = tkr_bpr_own_run(st, prec, pocc, occt, ohdr, ohdr_stride, n_owner, batch_size, first_batch, n_batches, ctl, loss_out, owner_waves,
                                   xch, epoch, stream);
    if (ev_after) TKR_CHECK(hipEventRecord((hipEvent_t)ev_after, (hipStream_t)stream));
    return rc;
}

extern "C" int tkr_bpr_own_plan_run(const tkr_plan_call* plan, const tkr_flow_state* st, int32_t first_batch, int32_t n_batches, uint32_t* ctl,
                                    float* loss_out, int32_t owner_waves, void* xch, uint32_t epoch, void* ev_before, void* ev_after,
                                    void* stream) {
    if (!plan || !st || first_batch < 0 || n_batches < 0 || first_batch + n_batches > plan->n_batches) return TKR_EINVAL;
    // K1 INSIDE the step's launch (the planner prologue of bpr_own_kernel) when the whole plan is what runs, one workgroup can plan
    // a batch with a thread per task slot, and the default form of the step is asked for; owner_waves bit 12: never
    const uint32_t tune = ((uint32_t)owner_waves >> 8) & 0xffu;
    const int B = plan->batch_size, n_owner = plan->n_owner;
    const int np = (st->k + 127) / 128;
    int npad = 1, npad_bits = 0;
    while (npad < 2 * B) { npad <<= 1; ++npad_bits; }
    const int own_words = n_owner > 0 ? ((plan->n_items + n_owner - 1) / n_owner + 31) / 32 : 0;
    const bool fusable = !(tune & 16u) && np == 1 && !(tune & (32u | 64u | 128u)) && first_batch == 0 && n_batches == plan->n_batches && n_batches > 0 &&
                         n_batches <= 64 && n_batches <= n_owner && B > 0 && 3 * B <= tkr::kWideThreads && plan->n_tr > 0 && plan->n_users > 0 &&
                         plan->n_items > 0 && plan->n_users < (1 << 25) && plan->n_items < (1 << 25) /*32-bit byte offsets into the bitmaps*/ && plan->ohdr_stride >= n_batches &&
                         plan->n_users == st->n_users && plan->n_items == st->n_items &&
                         tkr::own_lds_bytes_planned(np, n_batches, st->n_items, n_owner, B, npad, own_words) <= 160 * 1024;
    if (fusable) {
        if (!plan->tr_users || !plan->row_ptr || !plan->pos_cols || !plan->cols_sorted || !plan->ucnt || !plan->icnt || !plan->touch_u ||
            !plan->touch_i || !plan->out_u || !plan->out_i || !plan->out_j || !plan->task || !plan->occ || !plan->occt || !plan->prec ||
            !plan->pocc || !plan->ohdr)
            return TKR_EINVAL;
        tkr::PlanArgs pa;
        pa.tr_users = plan->tr_users; pa.row_ptr = plan->row_ptr; pa.pos_cols = plan->pos_cols; pa.cols_sorted = plan->cols_sorted;
        pa.ucnt = plan->ucnt; pa.icnt = plan->icnt; pa.touch_u = plan->touch_u; pa.touch_i = plan->touch_i;
        pa.out_u = plan->out_u; pa.out_i = plan->out_i; pa.out_j = plan->out_j;
        pa.task = reinterpret_cast<int4*>(plan->task); pa.occ = reinterpret_cast<int2*>(plan->occ); pa.occt = plan->occt;
        pa.prec = reinterpret_cast<int4*>(plan->prec); pa.pocc = reinterpret_cast<int4*>(plan->pocc); pa.ohdr = plan->ohdr;
        pa.seed = plan->seed; pa.first_triplet = plan->first_triplet;
        pa.n_tr = (uint32_t)plan->n_tr; pa.n_items = (uint32_t)plan->n_items;
        pa.n_plan = n_batches; pa.npad_items = npad; pa.own_words = own_words;
        pa.reg_sort_ok = (npad_bits < 31 && (uint64_t)(plan->n_users > plan->n_items ? plan->n_users : plan->n_items) < (1ull << (32 - npad_bits)) - 1ull) ? 1 : 0;
        if (ev_before) TKR_CHECK(hipEventRecord((hipEvent_t)ev_before, (hipStream_t)stream));
        const int rc = own_launch(st, plan->prec, plan->pocc, plan->occt, plan->ohdr, plan->ohdr_stride, n_owner, B, 0, n_batches, ctl, loss_out,
                                  owner_waves, xch, epoch, &pa, stream);
        if (ev_after) TKR_CHECK(hipEventRecord((hipEvent_t)ev_after, (hipStream_t)stream));
        return rc;
    }
    const int rc = tkr_sample_plan_owned(plan->tr_users, plan->n_tr, plan->row_ptr, plan->pos_cols, plan->cols_sorted, plan->n_users,
                                         plan->n_items, plan->seed, plan->first_triplet, plan->n_batches, plan->batch_size, plan->ucnt,
                                         plan->icnt, plan->touch_u, plan->touch_i, plan->out_u, plan->out_i, plan->out_j, plan->task,
                                         plan->occ, plan->occt, plan->prec, plan->pocc, plan->n_owner, plan->ohdr, plan->ohdr_stride, stream);
    if (rc != TKR_OK) return rc;
    return tkr_bpr_own_run_between(ev_before, ev_after, st, plan->prec, plan->pocc, plan->occt, plan->ohdr, plan->ohdr_stride, plan->n_owner,
                                   plan->batch_size, first_batch, n_batches, ctl, loss_out, owner_waves, xch, epoch, stream);
}

#ifdef TKR_PLAN_STAMP
extern "C" int tkr_debug_own_k1_prof(unsigned long long* out /*[32] host*/) {
    return hipMemcpyFromSymbol(out, HIP_SYMBOL(tkr::own_k1_prof), sizeof(unsigned long long) * 32) == hipSuccess ? 0 : -100;
}
#endif
