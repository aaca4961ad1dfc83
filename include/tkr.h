/* tkr.h -- C ABI of libtkr_hip.so: the MI355X (gfx950) hot path of top-k-rec.
 *
 * The reference (domainxz/top-k-rec) has no FFI: its boundary is the Python class API
 * (single/rec.py, single/bpr.py, single/vbpr.py) and the evaluate.py CLI, and internally the
 * two seams where Python hands work to a numerics runtime.  Each entry point below replaces
 * one such seam; the citation names the reference call site (file:line under the reference
 * root) whose work it does.
 *
 * Conventions
 *   - every function returns int: 0 = ok, > 0 = hipError_t, < 0 = TKR_E* below; nothing throws
 *   - all buffers are caller-owned DEVICE pointers (e.g. torch tensor.data_ptr()) with explicit
 *     sizes; the library keeps no device memory of its own, with one stated exception: K4's per-shape
 *     work-item table (a few KB, cached per device for the 8 most recent shapes)
 *   - NOT thread-safe: the reference is a single Python thread and so is the caller this
 *     library is written for.  Process-global state without locks: K4's work-item table cache and its
 *     arithmetic mode (tkr_topk_set_math), per-device attributes cached by K1 and K2f on first use.  One host
 *     thread per process calls in; one process per GPU.
 *   - `stream` is a hipStream_t passed as void*; all calls are asynchronous and stream-ordered;
 *     scalar results are written to device memory
 *   - ids are int32, parameters fp32
 *   - device memory means ORDINARY (coarse-grained) device allocations -- hipMalloc, a torch CUDA tensor.  loss_out, the K3
 *     workspace and every table must not be fine-grained / host-coherent memory (hipHostMalloc, hipMallocManaged,
 *     hipExtMallocWithFlags(fine-grained)): the loss sums of K2f / K3 use the hardware's global_atomic_add_f32, which such memory
 *     silently drops on gfx90a and later, and the write-through granule protocol of K2f / K2o assumes device-local lines
 */
#ifndef TKR_H
#define TKR_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define TKR_VERSION 120 /* (additions that change no existing entry point keep the number: K10 tkr_bpr_foldin_items, K11 tkr_ratings_*_dev, K12 tkr_rank_candidates, K13 tkr_lists_format_* / tkr_matrix_format_*, K15 tkr_group_*_dev / tkr_last_line_of_user_dev / tkr_compact_rows_*_dev, K16 tkr_fusion_*, K17 tkr_mmr_select / tkr_list_pair_sums, K21 tkr_als_solve_rows_prior / tkr_als_prior_workspace_bytes, K22 tkr_mlp_forward / tkr_mlp_fit / tkr_mlp_workspace_bytes, K27 tkr_smf_lse_rows / tkr_smf_dense_rows / tkr_smf_step_rows / tkr_smf_workspace_bytes, K4 tkr_topk_last_report (a diagnostic).) 0.1.20: K9 tkr_bpr_foldin (user vectors for new histories against frozen item factors; csrc/foldin.hip). 0.1.19: K8 tkr_like_ranks + tkr_like_ranks_workspace_bytes (filtered rank of every liked test column; csrc/like_ranks.hip). 0.1.18: K4 second form of bound-and-refine (csrc/topk_refine.hip; tkr_topk_workspace_bytes_for grows by the pieces' packed lists), any k (bpr_wide_kernel, score_topk_wide_kernel), tkr_lab_build; tkr_topk_set_finish is gone, tkr_topk_set_math(0) and tkr_vbpr_set_pairs(1 | 2) need the lab library. 0.1.17: tkr_vbpr_set_pairs (tkr_vbpr_workspace_floats + 64). 0.1.16: tkr_topk_set_finish (larger tkr_topk_workspace_bytes), tkr_bpr_own_plan_run plans inside the step's launch. 0.1.15: tkr_bpr_own_owners_shared; tkr_bpr_run takes `rec` non-const. 0.1.14: per-task loss sums instead of atomics on loss_out (larger tkr_vbpr_workspace_floats; K2 writes word 15 of its records). 0.1.13: tkr_bpr_own_plan_run, K4 to k = 768. 0.1.12: tkr_bpr_own_run_between. 0.1.11: K2o (tkr_sample_plan_owned, tkr_bpr_own_run: item rows owned by one workgroup each, resident in its LDS); prec[5] = last batch of the call that updated the row. 0.1.10: tkr_topk_workspace_bytes_for (K4 stages pre-converted fp16 tiles). 0.1.9: tkr_vbpr_colplan + tkr_vbpr_run_cols (VBPR in three launches per batch). 0.1.8: tkr_sync_flow_* (exchange of the granule tables). 0.1.7: K4 bound-and-refine arithmetic (tkr_topk_set_math(2), the default; larger tkr_topk_workspace_bytes); K2f leaves its ticket words zero. 0.1.6: K2f persistent dataflow step, tkr_plan_rollback, batches above 8192 */
#define TKR_OK 0
#define TKR_E_INVAL (-1)
#define TKR_E_UNSUPPORTED (-2)
#define TKR_E_IO (-3)          /* host text I/O: file cannot be opened / written */
#define TKR_E_PARSE (-4)       /* host text I/O: malformed line (where the reference raises) */
#define TKR_E_NOMEM (-5)       /* host text I/O: allocation failed */

int tkr_version(void);
/* 0.  The `make LAB=1` build that returned 1 is removed, with the kernel forms it held that were measured slower (K2o scalar exchange /
 * scout / 8 and 16 waves / loader ring, K4 bf16x3, the VBPR pair-sum placements 1 and 2; last source: git show 7a0cd86:top-k-rec_amd/csrc/<file>).
 * Asking for one of them returns TKR_E_UNSUPPORTED. */
int tkr_lab_build(void);

/* ---- K1: (u,i,j) draw + batch plan ---------------------------------------------------------
 * Replaces BPR._uniform_user_sampling (single/bpr.py:155-165) and the gradient de-duplication
 * bookkeeping TF does inside sess.run (single/bpr.py:100,141).
 *   tr_users[n_tr]           users with >= 1 positive (single/bpr.py:65)
 *   row_ptr[n_users+1], pos_cols[nnz]   tr_data as CSR, file order, duplicates kept (bpr.py:167-171)
 *   cols_sorted[nnz]         per-row ascending copy (membership test of bpr.py:163)
 *   seed, first_triplet      counter-based stream position (triplet g = first_triplet + b*B + t);
 *   ctl                      optional device int64[1]: batch index added to the stream position at
 *                            run time (lets one captured hipGraph walk through an epoch)
 *   ucnt[n_users], icnt[n_items]   running number of updates of every row (in/out); parity = which
 *                            of the two table buffers currently holds the row
 *   touch_u[n_users*16], touch_i[n_items*16]   scratch bitmaps, all-zero on entry and on exit
 *   out_u/out_i/out_j        [n_batches*B]
 *   task                     [n_batches][3B][4]  (row | kind<<31, occ_start, occ_count, parity); -1 = unused
 *   occ                      [n_batches][3B][2]  user occurrence: (i, j); item occurrence: (u, other|role<<31);
 *                            bit 30 of every id = parity of that row
 *   rec                      [n_batches][tkr_plan_max_blocks(B)*tkr_plan_team(B)][16]  per-wave launch records
 *   hdr                      [n_batches][4]  (workgroups used, light workgroups, heavy tasks, tasks)
 *   occt                     [n_batches][3B] triplet index t of every sorted occurrence (used by K3)
 *   tpar                     (nullable) [n_batches*B] per triplet: parity of u | parity of i << 1 | parity of j << 2 at its
 *                            batch -- lets K3's sparse view score a triplet where it projects it (no per-occurrence launch)
 *   prec, pocc               (both NULL, or both set = DATAFLOW form for K2f; rec / hdr / tpar are then not written and may
 *                            be NULL)  pocc [n_batches][3B][4]: per sorted occurrence (a, version of a, b | role<<31,
 *                            version of b); prec [n_batches][3B][32]: one 128-byte record per task slot:
 *                            [0] row | kind<<31 (-1 = unused slot) [1] version of the row [2] occurrences [3] index of its
 *                            first occurrence in pocc counted from batch 0 [4] batch [5] last batch < [4] of this call
 *                            that updated the row (-1: none) [8+4q..] pocc of occurrence q < 4 [24+q] the index of that
 *                            occurrence's triplet in its batch (= occt)
 *   workspace                (required for batch_size > 8192, nullable below) tkr_plan_workspace_bytes(batch_size, n_batches) bytes
 *                            of device scratch.  With it, batches of 1025 .. 65,536 are planned by a counting sort over row ranges
 *                            (csrc/planner_mid.hip: six launches; range sums, above 16,384 also 12 bytes per triplet of run lists) and larger ones grid-wide (device radix
 *                            sort of batch|row|occurrence keys, scans) instead of one workgroup per batch -- single/bpr.py:103-113
 *                            accepts any batch_size.  The touch maps are scratch INSIDE a call (zero before and after)
 * n_batches <= 512, ids < 2^30, batch_size <= 2^20 (the dataflow form: batch_size <= 8192).  Output is bit-exact against
 * oracle/plan_np.py for every batch size. */
int tkr_plan_team(int32_t batch_size);        /* waves per step workgroup / heavy-row team: 4 (B <= 1024), 8 (<= 16384) or 16 */
int tkr_plan_max_blocks(int32_t batch_size);  /* workgroups a batch can need */
int tkr_sample_plan(const int32_t* tr_users, int32_t n_tr, const int32_t* row_ptr, const int32_t* pos_cols,
                    const int32_t* cols_sorted, int32_t n_users, int32_t n_items, uint64_t seed,
                    uint64_t first_triplet, const int64_t* ctl, int32_t n_batches, int32_t batch_size,
                    int32_t* ucnt, int32_t* icnt, uint32_t* touch_u, uint32_t* touch_i, int32_t* out_u,
                    int32_t* out_i, int32_t* out_j, int32_t* task, int32_t* occ, int32_t* rec, int32_t* hdr,
                    int32_t* occt, int32_t* tpar, int32_t* prec, int32_t* pocc, void* workspace, int64_t workspace_bytes,
                    void* stream);
/* device scratch tkr_sample_plan needs for batch_size > 8192 (sort keys, ranks, hipcub storage); 0 for smaller batches */
int64_t tkr_plan_workspace_bytes(int32_t batch_size, int32_t n_batches);

/* Take batches [first_batch, first_batch + n_batches) of a plan out of the update counters again.  tkr_sample_plan
 * advances ucnt / icnt for every batch it PLANS; a caller that drops the rest of a plan (BPR.train stopping inside a
 * chunk, a parameter read-back between chunks) calls this so that the counters equal the updates that really RAN.
 * `task` is the array tkr_sample_plan wrote. */
int tkr_plan_rollback(const int32_t* task, int32_t batch_size, int32_t first_batch, int32_t n_batches, int32_t* ucnt,
                      int32_t* icnt, void* stream);

/* ---- K2: BPR mini-batch step ---------------------------------------------------------------
 * Replaces sess.run([solver, obj]) (single/bpr.py:141) on the graph of single/bpr.py:81-100.
 * Double-buffered tables: U, msU are [2][n_users][k]; V, msV [2][n_items][k]; b, msb [2][n_items];
 * the buffer holding row r is (ucnt[r] & 1) resp. (icnt[r] & 1) -- see K1.
 * opt = 1 selects the legacy plain-SGD update P -= lr * g of old/methods/bpr.py:57-61: the
 * objective and gradients are the same as mode 0 (old/methods/bpr.py:43-51), the ms* tables are neither read
 * nor written and may be NULL. */
typedef struct {
    float* U;
    float* msU;
    float* V;
    float* msV;
    float* b;
    float* msb;
    int32_t n_users, n_items, k;
    int32_t mode;            /* 0 = 'l2' (single/bpr.py:92-95), 1 = L1 variant (:96-99) */
    float lu, li, lj, lb;    /* lambda_u, lambda_i, lambda_j, lambda_b (single/bpr.py:20) */
    float lr;                /* RMSPropOptimizer(lr) (single/bpr.py:100) */
    float rho, eps;          /* TF defaults 0.9, 1e-10 */
    int32_t opt;             /* 0 = sparse RMSProp (single/bpr.py:100), 1 = plain SGD (old/methods/bpr.py:57-61) */
} tkr_bpr_state;

/* n_batches consecutive batches of a plan (the inner loop of single/bpr.py:139-147), one launch
 * each, in plan order; loss_out (nullable) is float[n_batches], pre-zeroed by the caller: the
 * batch objective (single/bpr.py:93-99) is added to loss_out[b].  How (all entries with a loss_out): thousands of waves summing
 * into one word with atomics cost 10 ns apiece, one after the other (4-5x the step at batch 8192).  Every user task therefore
 * leaves its sum in a place of its own -- here word 15 of its launch record in `rec` (K1 leaves it zero; that one word of `rec` is
 * WRITTEN by the step, which is why `rec` is not const; a plan run again with a loss_out overwrites it), under K2o a {sum, epoch} slot of `xch`, under K2f its workgroup's LDS, under K3 one of
 * 64 slots behind the workspace -- and one small launch per CALL adds them up into loss_out (tkr_bpr_own_run in its default
 * form ASSIGNS loss_out[b]: no fill is needed in front of it). */
/* any k: up to 512 (256 above batch_size 1024) a wave holds its row in registers; wider rows take the generic form
 * (csrc/bpr_step.hip bpr_wide_kernel: two passes over k per occurrence, the gradient sum through memory) */
int tkr_bpr_run(const tkr_bpr_state* st, int32_t* rec, const int32_t* occ, const int32_t* hdr,
                int32_t batch_size, int32_t n_batches, float* loss_out, void* stream);

/* ---- K2f: the same step as ONE persistent launch per chunk (dataflow form; csrc/bpr_flow.hip) ------------------
 * Replaces the same call site as K2 (single/bpr.py:139-147, the loop around sess.run) for small batches, where one launch
 * per batch is 96 % idle.  Batches are ordered by the data instead of by kernel boundaries: every table element is an
 * 8-byte granule {fp32 value, uint32 version tag}, double-buffered (version v of a row lives in buffer v & 1):
 *   U, msU   [2][n_users][kp] granules, kp = tkr_flow_row_granules(k) (k rounded up to 128; padding: value 0 / slot 1)
 *   V, msV   [2][n_items][kp]
 *   tailU/V  [2][n][4] granules per row: {item bias, its RMSProp slot, expect[0], expect[1] (uint32 bits)}; users carry
 *            zeros for the first two
 *   rdU/V    [n][2] uint32: acknowledged partner reads of the row, by parity of the version read
 * A freshly assigned table holds version 0 in buffer 0 (all tags 0, expects 0, rd 0) and tags 0xffffffff in buffer 1.
 * item_bufs = 4 (round 4): the ITEM tables have FOUR buffers -- V, msV [4][n_items][kp], tailV [4][n_items][8] granules per row
 * {bias, its slot, expect[0..3], 0, 0}, rdV [n_items][4], version v in buffer v & 3 -- so the task that writes version v+1 waits
 * for the readers of v-3 instead of v-1: with the rows of a chain handed over in LDS (K2o) the acknowledge round trip of TWO
 * buffers (publish -> partner reads -> acknowledge -> next publish, once per two batches) is what paces batch 256.
 * The plan is tkr_sample_plan's dataflow form (prec / pocc non-NULL there): `prec` points at the record of the first
 * task of the first batch to run, `pocc` and `loss_out` (nullable, pre-zeroed) at batch 0 of that plan call.
 * ctl: tkr_flow_ctl_words() uint32 of caller-owned device memory, zeroed once by the caller; every launch leaves its
 * ticket words at zero again (the last workgroup out does it), so calls on one stream follow each other without a
 * memset between them.  One ctl serves one launch at a time.  ctl[status word] != 0 after a launch means a bounded spin
 * ran out (results invalid; zero ctl again before anything else runs on it).
 * waves_per_cu: 0 = default (one 4-wave workgroup per CU below batch 320, two from there on: csrc/bpr_flow.hip).
 * k <= 256, 3 * batch_size * n_batches < 2^29. */
typedef struct {
    void* U;
    void* msU;
    void* tailU;
    uint32_t* rdU;
    void* V;
    void* msV;
    void* tailV;
    uint32_t* rdV;
    int32_t n_users, n_items, k;
    int32_t mode;            /* as tkr_bpr_state */
    float lu, li, lj, lb;
    float lr, rho, eps;
    int32_t opt;             /* 0 = sparse RMSProp, 1 = plain SGD (ms tables unused, may be NULL) */
    int32_t item_bufs;       /* buffers per ITEM row: 0 or 2 = two (as the user rows), 4 = four (see below) */
} tkr_flow_state;
int32_t tkr_flow_row_granules(int32_t k);
int32_t tkr_flow_ctl_words(void);
#define TKR_FLOW_CTL_STATUS 1026 /* index of the status word inside ctl */
#define TKR_FLOW_CTL_SPINS 1027  /* diagnostics: spin passes taken since the caller last zeroed it */
int tkr_bpr_flow_run(const tkr_flow_state* st, const int32_t* prec, const int32_t* pocc, int32_t batch_size,
                     int32_t n_batches, uint32_t* ctl, float* loss_out, int32_t waves_per_cu, void* stream);

/* ---- K2o: the persistent step with OWNED item rows (csrc/bpr_own.hip) ---------------------------------------------
 * Replaces the same call site as K2 / K2f (single/bpr.py:139-147) on the same granule tables (tkr_flow_state), and leaves them
 * in the same state as K2f does: the two kernels, the exchange and get / set may be mixed freely between launches.  Item row r is
 * served by workgroup r % n_owner, which keeps the row, its slot, bias and acknowledge totals in LDS from the row's first update
 * in a launch on: the task of batch t+1 finds the row of batch t there instead of polling memory for it (what bounded K2f at
 * batch 256).  Partner rows are read from the tables as in K2f.  User tasks are handed out by tickets as in K2f.
 *   tkr_bpr_own_owners(n_items, k)   n_owner for the current device (its CU count), or 0 when ceil(n_items / CUs) rows of
 *                                    8*kp + 16 bytes do not fit one CU's 160 KB of LDS (use K2f then)
 *   tkr_sample_plan_owned            tkr_sample_plan's dataflow form (prec, pocc; batch_size <= 8192) with the records of every
 *                                    batch's ITEM tasks in (row % n_owner, row) order -- same slots -- and
 *                                    ohdr[owner * ohdr_stride + batch] = first slot | tasks << 16 (ohdr_stride >= n_batches).
 *                                    (K2f runs such a plan too: the order of tasks inside a batch means nothing to it.)
 *   tkr_bpr_own_run                  batches [first_batch, first_batch + n_batches) of such a plan in ONE launch of n_owner
 *                                    workgroups (all resident: n_owner <= CUs).  prec / pocc / occt / ohdr / loss_out point at
 *                                    batch 0 of the plan call; owner_waves: waves per workgroup that serve the owner queue, 0 =
 *                                    default (workgroups of 12 waves at k <= 128: 10 on the owner queue, 2 on user tickets; 8
 *                                    waves above: 7 + 1); ctl as for tkr_bpr_flow_run.  owner_waves bits 8, 15 (and 13, 14 at
 *                                    k <= 128) asked for removed forms: TKR_E_UNSUPPORTED.
 *                                    xch: 16 * batch_size bytes per batch of the plan (the user tasks' loss sums {value, epoch},
 *                                    one slot per task), caller-owned, zeroed once; epoch: a
 *                                    number > 0 that no earlier launch on this xch used (a counter per plan buffer does).
 * k <= 256, n_batches <= 512. */
int32_t tkr_bpr_own_owners(int32_t n_items, int32_t k);
/* the same when `share` processes split one device's CUs between them (ranks packed on one GPU: each runs CUs / share owners, so
 * that the workgroups of all of them are resident together); 0 when ceil(n_items / (CUs / share)) rows do not fit an owner's LDS */
int32_t tkr_bpr_own_owners_shared(int32_t n_items, int32_t k, int32_t share);
int tkr_sample_plan_owned(const int32_t* tr_users, int32_t n_tr, const int32_t* row_ptr, const int32_t* pos_cols,
                          const int32_t* cols_sorted, int32_t n_users, int32_t n_items, uint64_t seed, uint64_t first_triplet,
                          int32_t n_batches, int32_t batch_size, int32_t* ucnt, int32_t* icnt, uint32_t* touch_u,
                          uint32_t* touch_i, int32_t* out_u, int32_t* out_i, int32_t* out_j, int32_t* task, int32_t* occ,
                          int32_t* occt, int32_t* prec, int32_t* pocc, int32_t n_owner, int32_t* ohdr, int32_t ohdr_stride,
                          void* stream);
int tkr_bpr_own_run(const tkr_flow_state* st, const int32_t* prec, const int32_t* pocc, const int32_t* occt, const int32_t* ohdr,
                    int32_t ohdr_stride, int32_t n_owner, int32_t batch_size, int32_t first_batch, int32_t n_batches, uint32_t* ctl, float* loss_out,
                    int32_t owner_waves, void* xch, uint32_t epoch, void* stream);
/* One call for a SHORT training call -- K1 of a chunk and the persistent step on it, back to back: tkr_sample_plan_owned with the
 * arguments of `plan` (a struct: a caller fills it once per plan buffer and changes first_triplet / n_batches per call), then
 * tkr_bpr_own_run on batches [first_batch, first_batch + n_batches) of that plan, with the caller's two events (hipEvent_t or NULL)
 * recorded around the step launch.  No trip back through the host language between them: a 20-batch call is ~90 us of device
 * work, and an interpreter between the launches leaves the device waiting for the host.
 * From 0.1.16 the whole plan is what most short calls run, and then K1 runs INSIDE the step's launch (ONE launch: workgroups
 * 0 .. n_batches-1 plan a batch each in front of the step, csrc/bpr_own.hip PLAN; the last workgroup out adds the losses up): when
 * first_batch == 0, n_batches == plan->n_batches <= min(64, n_owner), batch_size <= 256, k <= 128, the default step form, n_users and
 * n_items below 2^25; otherwise tkr_sample_plan_owned's launches + the step's, as before.  Same words in every plan array and the same
 * tables either way.  owner_waves bit 12: never the one-launch form; bit 9: the losses always by their own launch. */
typedef struct tkr_plan_call {
    const int32_t *tr_users, *row_ptr, *pos_cols, *cols_sorted;
    int32_t *ucnt, *icnt;
    uint32_t *touch_u, *touch_i;
    int32_t *out_u, *out_i, *out_j, *task, *occ, *occt, *prec, *pocc, *ohdr;
    uint64_t seed, first_triplet;
    int32_t n_tr, n_users, n_items, n_batches, batch_size, n_owner, ohdr_stride, reserved;
} tkr_plan_call;
int tkr_bpr_own_plan_run(const tkr_plan_call* plan, const tkr_flow_state* st, int32_t first_batch, int32_t n_batches, uint32_t* ctl,
                         float* loss_out, int32_t owner_waves, void* xch, uint32_t epoch, void* ev_before, void* ev_after, void* stream);
/* tkr_bpr_own_run between two events of the caller (hipEvent_t or NULL), recorded on `stream` right around the launch */
int tkr_bpr_own_run_between(void* ev_before, void* ev_after, const tkr_flow_state* st, const int32_t* prec, const int32_t* pocc,
                            const int32_t* occt, const int32_t* ohdr, int32_t ohdr_stride, int32_t n_owner, int32_t batch_size,
                            int32_t first_batch, int32_t n_batches, uint32_t* ctl, float* loss_out, int32_t owner_waves, void* xch,
                            uint32_t epoch, void* stream);

/* ---- K3: VBPR mini-batch step -------------------------------------------------------------
 * Replaces sess.run([solver, obj]) of single/vbpr.py:114 on the graph of single/vbpr.py:50-73 and the
 * per-batch host gather of two dense [B, d] feature slices (vbpr.py:114).  kh = k // 2.
 *   U, msU      [2][n_users][2*kh]  rows = [ure | uce]  (vbpr.py:37-40), double-buffered like K2
 *   I, msI      [2][n_items][kh]    ire (vbpr.py:41);   irb, msirb [2][n_items] (vbpr.py:43)
 *   cem, mscem  [d][kh], icb, msicb [d]: dense variables, updated in place every batch (vbpr.py:45-48,73)
 *   feat        [n_items][d] dense fp32, resident (REC.load_content_data, rec.py:23-33)
 * Optional sparse view of feat (f_ptr != NULL; content features are tf-idf-like, ~0.5 % dense at d = 20,000): the
 * projection gathers cem rows per nonzero instead of contracting over d, and the dense-variable update walks the
 * columns of feat (CSC) against the per-item sums of the batch.  Same arithmetic up to the order of the fp32 sums;
 * every element of cem / icb still gets TF's dense ApplyRMSProp every batch (vbpr.py:65,67,73).
 *   f_ptr [n_items+1], f_col / f_val [nnz]   CSR over items, ascending columns inside a row
 *   c_ptr [d+1], c_item / c_val [nnz]        CSC over feature columns, ascending items inside a column
 *   item_tag [n_items] int64                 scratch, zeroed ONCE by the caller and then owned by the library (per-batch
 *                                            membership bitmaps, slots and a batch counter live in it) */
typedef struct {
    float* U;
    float* msU;
    float* I;
    float* msI;
    float* irb;
    float* msirb;
    float* cem;
    float* mscem;
    float* icb;
    float* msicb;
    const float* feat;
    int32_t n_users, n_items, kh, d;
    int32_t mode;                /* 0 = 'l2' (vbpr.py:63-67), 1 = L1 variant (:68-72) */
    float lu, li, lj, lb, le;    /* lambda_u, lambda_i, lambda_j, lambda_b, lambda_e (vbpr.py:18) */
    float lr, rho, eps;
    const int32_t* f_ptr;
    const int32_t* f_col;
    const float* f_val;
    const int32_t* c_ptr;
    const int32_t* c_item;
    const float* c_val;
    int64_t* item_tag;
} tkr_vbpr_state;

/* floats of scratch tkr_vbpr_run needs (split-K partials, s_t, P_t, W_t; the sparse view's per-item sums A, a: the same carve at any kh) */
int64_t tkr_vbpr_workspace_floats(int32_t batch_size, int32_t kh, int32_t d);
/* tkr_vbpr_run_cols: where the [B, B] pair sums S_t, T_t of a batch (vbpr.py:61) are formed -- 0: a launch of their own between the
 * projection and the update (three launches per batch), the only placement.  1 (every task of the update works out the sums it
 * needs) and 2 (the first blocks of the update launch form them) were measured slower and removed: TKR_E_UNSUPPORTED. */
int tkr_vbpr_set_pairs(int32_t mode);
/* n_batches consecutive batches planned by tkr_sample_plan (tri_i / tri_j = its out_i / out_j);
 * any batch_size (batches above 8192 are planned grid-wide, see tkr_sample_plan; above 65,536 the first four triplet indices of a
 * launch record are read from occt); kh <= 128 holds rows in registers, kh > 128 runs the generic form of the sparse view
 * (csrc/vbpr_wide.hip: factors walked in passes) and needs the CSR view (st->f_ptr): the dense MFMA view at kh > 128 is
 * TKR_E_UNSUPPORTED; loss_out as in tkr_bpr_run.
 * RANGE (this entry point and tkr_vbpr_run_cols): a pair term sigma(-(alpha_a + beta_b)), alpha_a = irb_i - irb_j + (f_i - f_j).icb of
 * triplet a, beta_b = x_ui - x_uj of triplet b, is evaluated as 1 / (1 + e^alpha_a * e^beta_b) with alpha and beta EACH clamped to
 * [-80, 80] before its exponential (csrc/tkr_common.h pair_exp).  With |alpha| <= 80 and |beta| <= 80 for every triplet of the batch
 * the step is the reference's (a product that overflows or underflows gives the saturated 0 or 1, which is the fp32 value).  Outside
 * that range it is not: alpha = 100, beta = -85 is scored as sigma(0) = 0.5 where the objective has sigma(-15) = 3e-7.  Nothing
 * checks the range; tables set from outside are the caller's to keep inside it. */
int tkr_vbpr_run(const tkr_vbpr_state* st, const int32_t* tri_i, const int32_t* tri_j, const int32_t* rec,
                 const int32_t* occ, const int32_t* hdr, const int32_t* occt, const int32_t* tri_u /*nullable*/,
                 const int32_t* tpar /*nullable*/, int32_t batch_size,
                 int32_t n_batches, float* workspace, float* loss_out, void* stream);

/* Column-plan form of the same step (batch_size <= 1024, CSR view of feat; kh % 4 == 0 and kh <= 128: rows and cem rows in registers,
 * any other kh: the generic kernels of csrc/vbpr_wide.hip on the same plan): three launches per batch
 * (project + score / pair sums / row tasks and column tasks side by side) instead of four to six, csrc/vbpr_cols.hip.
 * Which (triplet, feature column) pairs a batch touches depends on the sampled triplets and on the structure of feat only,
 * so it is prepared beside K1, off the step's critical path:
 *   tkr_vbpr_colplan   for each of n_batches batches (tri_i / tri_j = tkr_sample_plan's out_i / out_j), from the CSR
 *                      f_ptr / f_col / f_val of feat, with tcap = 2 * row_cap and row_cap >= the longest row of feat:
 *                      tcnt [n_batches][B], tent [n_batches][B][tcap][2]   per triplet the (column, value bits) of f_i's nonzeros
 *                                          (+value) followed by f_j's (-value): the gather list of the projection
 *                      cent [n_batches][B * tcap][2]   the same entries as (t, +-value bits) grouped by feature column, every
 *                                          column's run in (t, side) order
 *                      colh [n_batches][d][8]   per column (entries, first entry in cent, then its first three entries inline)
 *                      One workgroup per batch keeps the d column counters in LDS: tkr_vbpr_colplan_lds_bytes(batch_size, d)
 *                      <= 160 KB, else TKR_E_UNSUPPORTED (the caller then stays with tkr_vbpr_run).
 *   tkr_vbpr_run_cols  the batches themselves; arguments as tkr_vbpr_run (tri_u and tpar required; st->feat and the CSC
 *                      members of st are not read) plus the column plan.  cols_per_block: feature columns per 256-thread
 *                      workgroup of the dense update, 0 = as many as fit (sparse features); 1-2 when runs are long (a narrow
 *                      dense feat: every column meets every triplet).
 * Same arithmetic as tkr_vbpr_run up to the order of fp32 sums; bitwise reproducible run to run. */
int64_t tkr_vbpr_colplan_lds_bytes(int32_t batch_size, int32_t d);
int tkr_vbpr_colplan(const int32_t* f_ptr, const int32_t* f_col, const float* f_val, int32_t d, const int32_t* tri_i,
                     const int32_t* tri_j, int32_t batch_size, int32_t n_batches, int32_t row_cap, int32_t* colh, int32_t* cent,
                     int32_t* tcnt, int32_t* tent, void* stream);
int tkr_vbpr_run_cols(const tkr_vbpr_state* st, const int32_t* tri_i, const int32_t* tri_j, const int32_t* rec, const int32_t* occ,
                      const int32_t* hdr, const int32_t* occt, const int32_t* tri_u, const int32_t* tpar, const int32_t* colh,
                      const int32_t* cent, const int32_t* tcnt, const int32_t* tent, int32_t row_cap, int32_t cols_per_block,
                      int32_t batch_size, int32_t n_batches, float* workspace, float* loss_out, void* stream);

/* ---- K4: full-catalogue score -> rated mask -> top-K -------------------------------------------
 * Replaces evaluate.py:78-81 (np.dot + bias + np.argsort over every row) and the rated-item filter
 * of the rank walk (evaluate.py:96-105).
 *   U [*, k] user factors; user_idx[n_rows] (nullable) picks the rows to rank (default 0..n_rows-1)
 *   Vt [n_cols, k], bias[n_cols] (nullable): the scenario's test-item rows, already gathered
 *     (evaluate.py:75-77; bias gathered per test id -- the reference's broadcast at :79-80 is only
 *     defined when the scenario's id list equals vid)
 *   mask [ceil(n_cols/32)][mask_pitch] (nullable): bit (c & 31) of word (c >> 5, row) = column c is
 *     train-rated by row's user (evaluate.py:98); built by tkr_build_rated_mask into a zeroed buffer
 *   out_ids [n_rows, K]: the K best unrated columns, descending score, ties -> higher column first;
 *     -1 where fewer than K unrated columns exist.  out_scores (nullable) alike, -inf padded.
 *   THE CANONICAL ORDER (K4, K6, K8 and K12 rank by it) covers every fp32 value a score can take:
 *       NaN  >  +inf  >  the finite scores  >  -inf;   ties -> the higher column first.
 *     All NaNs tie, whatever their sign and payload (the GPU makes positive ones, an x86 host and a "-nan" token of a model
 *     file negative ones); -0.0 == +0.0.  It is np.argsort(scores, kind='stable') read backwards -- numpy sorts a NaN of either
 *     sign as the largest value -- that is oracle/ref_np.py filtered_topk(canonical=True), the order evaluate.py:81 gives a model
 *     that diverged.  An unrated column is listed whatever its score: a NaN column comes first, a true -inf score is an entry
 *     with its id.  out_scores (and K12's score_out) hold A NaN for a NaN score, the payload is not specified; every other score
 *     keeps its bits.  -1 / -inf is the padding of a short list and nothing else.
 *     Under mode 2 a user block is ranked by the mode-1 kernel when its margin means nothing: the user row or the item table or
 *     the bias holds a NaN or an infinity, |u| * max|v_i| + max|bias| comes near fp32's range, or the largest |element| of the
 *     row (of the table) is outside [2^-47, 2^60) and not 0 -- the row's sum of squares or the fp16 scaling would overflow or
 *     underflow --, or max|bias| in the user's scaled units leaves fp32's range.  What the fp16 pass made of such a block is thrown
 *     away, the thresholds it published included; the lists are mode 1's either way (tests/test_gpu_nonfinite_scores.py).
 *   workspace (nullable, device, workspace_bytes): scratch for per-item-range partial lists; with
 *     tkr_topk_workspace_bytes(n_rows, K) bytes the launch splits the catalogue so that the grid fills
 *     the 256 CUs in whole rounds (results are identical with or without it)
 * Arithmetic of the scores (tkr_topk_set_math, initial value from TKR_TOPK_MATH=refine|fp32):
 *   2 "refine" (default; k <= 128, needs the workspace, n_cols < 2^27): bound-and-refine.  ONE fp16 product per element
 *     (factors scaled by powers of two, v_mfma_f32_32x32x16_f16) scores the catalogue within a rigorous margin
 *     (2^-10 * 1.05 * |u| * max|v_i| + roundings, see csrc/topk.hip); the candidate lists keep everything within twice the
 *     margin of the K-th best approximate score, and the survivors are rescored with the arithmetic of mode 1, which
 *     decides the order: ids and score bits are those of mode 1, at 2.1x its speed.  A list that cannot hold its margin
 *     (massive near-ties) sends its user block through the mode-1 kernel.  Without a workspace the call runs as mode 1.
 *   0 "bf16x3" (six exact bf16 partial products) is removed: tkr_topk_set_math(0) returns TKR_E_UNSUPPORTED, and
 *     TKR_TOPK_MATH=bf16x3 runs as mode 1;
 *   1 "fp32": v_mfma_f32_32x32x2_f32, used for every k and always for k > 128: per score the fma chain
 *     acc <- fma(v[j], u[j], acc); acc <- fma(v[KH+j], u[KH+j], acc), j = 0 .. KH-1, KH = ceil(k/2), then fl(acc + bias)
 *     (oracle/ref_np.py mfma_chain_scores restates it; bit-exact on generic inputs).
 *   On gfx950 the fp32 MFMA runs at the vector-ALU rate and overlaps nothing; mode 2 is 1.5-2.1x faster than mode 1.
 * K <= 32 per launch (larger K: rank 32, add the found columns to the mask with tkr_build_rated_mask, rank
 * again -- top-k-rec_amd/tkr_hip.py score_topk does this); any k (above 768: score_topk_wide_kernel, one wave per row, a lane per item,
 * the same fma chain; 256 < k <= 768: mode 1 with the k dimension in slabs -- 128 factors of each half of k per slab, so
 * the chain of a score is the one above, the two halves of the WHOLE width interleaved, at these widths too; 60 % of the
 * fp32-MFMA peak at k = 512, register spills above 512). */
int64_t tkr_topk_workspace_bytes(int32_t n_rows, int32_t K);
/* the same + room for the item factors of mode 2 pre-converted to scaled fp16 (k <= 128), laid out as the LDS image of every
 * 32-item tile: with a workspace of at least this size a K4 call converts V once (a ~5 us pre-pass) and every workgroup stages
 * its tiles with one direct-to-LDS load per thread instead of converting them again (results are identical either way) */
int64_t tkr_topk_workspace_bytes_for(int32_t n_rows, int32_t n_cols, int32_t k, int32_t K);
int tkr_topk_set_math(int32_t mode);
/* A DIAGNOSTIC, for tests: what the last tkr_score_topk call of the process did under mode 2.  `out` is a HOST array of n >= 6 words:
 *   out[0] form: 0 = no bound-and-refine pass ran (mode 1, k > 128, no room for the block flags in the workspace, or a refused
 *          call), 1 = the first form (csrc/topk.hip score_topk_bf16_kernel), 2 = the second (csrc/topk_refine.hip)
 *   out[1] width of the candidate ids, 16 or 32;  out[2] 1 when the pre-converted tile image was used
 *   out[3] user blocks;  out[4] workgroups of the plan: (user block, item range) pairs, or the pieces of the work-item table --
 *          more than out[3] means the catalogue was cut into item ranges
 *   out[5] FLAGGED user blocks: those the fp16 pass gave up (a list could not hold its margin, or a row's margin means nothing)
 *          and the mode-1 kernel ranked;  out[6 + b], b < min(out[3], n - 6): 1 when block b is one of them
 * The last call of the process wins and nothing is locked (the library is not thread-safe).  Valid only while that call's
 * workspace is alive and before the next tkr_score_topk: the flags live in the workspace.  Unlike every other entry point it
 * SYNCHRONISES the call's stream (it copies the flag words to the host); with form 0 it touches no device.  Changes no result. */
int tkr_topk_last_report(int32_t* out, int32_t n);
int tkr_build_rated_mask(const int64_t* rated_ptr, const int32_t* rated_cols, int32_t n_rows, int32_t n_cols,
                         uint32_t* mask, int32_t mask_pitch, void* stream);
int tkr_score_topk(const float* U, const int32_t* user_idx, int32_t n_rows, const float* Vt, const float* bias,
                   int32_t n_cols, int32_t k, const uint32_t* mask, int32_t mask_pitch, int32_t K,
                   int32_t* out_ids, float* out_scores, void* workspace, int64_t workspace_bytes, void* stream);

/* ---- K5: hit counting of the rank walk (evaluate.py:99-103) ------------------------------------
 * first_bucket[p / step] += 1 (uint64 atomics) for every kept position p < interval*step of row r
 * whose column is in like_cols[like_ptr[r] .. like_ptr[r+1]) (ascending); hits[q] of the reference
 * is the running sum over buckets <= q. */
int tkr_count_hits(const int32_t* ids, int32_t n_rows, int32_t K, const int64_t* like_ptr, const int32_t* like_cols,
                   int32_t step, int32_t interval, uint64_t* first_bucket, void* stream);

/* ---- K6 / K7: the rank walk of utils.evaluate (utils.py:101-127) -----------------
 * utils.evaluate buckets a hit by the item's RAW rank t -- train-rated columns included (utils.py:113-117:
 * j = t // step) -- and sums reciprocal ranks 1/(t+1).  With ids = K4's first K unrated columns of each row,
 *   raw_rank[r][p] = p + #{rated columns of row r ranked before ids[r][p]}   (-1 where ids is -1)
 * under K4's canonical order over every fp32 value (NaN > +inf > finite > -inf, all NaNs tie, ties -> higher column first: a rated
 * column whose score is NaN is in front of every kept column that is not); kept and rated columns are scored
 * by the fp32 chain of tkr_score_topk's modes 1 and 2 (fl(acc + bias), -0.0 -> +0.0): the bits the kept list was
 * ordered by, so the count agrees with K4, K8 and K12 down to the last ulp.  rated_ptr/rated_cols: the CSR given to
 * tkr_build_rated_mask (columns in [0, n_cols) of Vt; they are not checked).
 * tkr_count_hits_rr: hit_first[r][j] += 1 and rr_first[r][j] += 1/(t+1) (fp64) for every kept liked column with
 * j = t / step < interval, sequentially per row (reproducible); the caller zeroes both arrays, sums over rows and
 * accumulates buckets <= k (utils.py:115-117).  K <= 256 per launch (TKR_E_UNSUPPORTED above; utils.evaluate
 * chunks a longer list), any factor width k. */
int tkr_raw_ranks(const float* U, const int32_t* user_idx, int32_t n_rows, const float* Vt, const float* bias, int32_t k,
                  const int64_t* rated_ptr, const int32_t* rated_cols, const int32_t* ids, int32_t K, int32_t* raw_rank,
                  void* stream);
int tkr_count_hits_rr(const int32_t* ids, const int32_t* raw_rank, int32_t n_rows, int32_t K, const int64_t* like_ptr,
                      const int32_t* like_cols, int32_t step, int32_t interval, int32_t* hit_first, double* rr_first,
                      void* stream);

/* ---- K8: filtered rank of every liked test column (the rank walk of evaluate.py:96-105, to any depth) -----------
 * U, user_idx, n_rows, Vt, bias, n_cols, k, mask, mask_pitch: exactly those of tkr_score_topk (mask nullable);
 * like_ptr [n_rows+1] (starts at 0), like_cols: the CSR of tkr_count_hits, ascending columns inside a row.  For entry e of row r
 * with column l = like_cols[e]:
 *   rank_out[e] = -1 when l is masked for the row (a rated like is never reached by the reference walk) or not in [0, n_cols)
 *   rank_out[e] = #{c < n_cols unmasked, c != l : s(r,c) > s(r,l) or (s(r,c) == s(r,l) and c > l)} otherwise
 * -- the number of kept columns in front of l in K4's canonical order, with s the mode-1 score above (the fma chain, fl(acc + bias),
 * -0.0 -> +0.0), bit for bit, and ">" / "==" those of the canonical order stated there (every NaN one score above +inf, whatever its
 * sign and payload): a like at position p of tkr_score_topk's list has rank p.  Integer and deterministic.  accuracy@k for
 * any step / total, AUC, NDCG, MRR and MAP all follow from the ranks (top-k-rec_amd/rankmetrics.py).
 * k <= 256: the fp32-MFMA tile loop of K4 with a counting epilogue (the sorted like scores of a user block and one counter each in
 * LDS, a binary search per score; item ranges of a block add up in rank_out by integer atomics); k > 256: one wave per row, a lane
 * per column.  Any number of likes per row; n_cols < 2^27.
 * workspace (required): tkr_like_ranks_workspace_bytes(n_rows, n_cols, k, n_likes) bytes, n_likes = like_ptr[n_rows].  The call
 * writes every rank_out[e] itself (no zeroing by the caller); a workspace sized for fewer likes than the CSR holds leaves -2 in all
 * of them. */
int64_t tkr_like_ranks_workspace_bytes(int32_t n_rows, int32_t n_cols, int32_t k, int64_t n_likes);
int tkr_like_ranks(const float* U, const int32_t* user_idx, int32_t n_rows, const float* Vt, const float* bias,
                   int32_t n_cols, int32_t k, const uint32_t* mask, int32_t mask_pitch, const int64_t* like_ptr,
                   const int32_t* like_cols, int32_t* rank_out, void* workspace, int64_t workspace_bytes, void* stream);

/* ---- K12: score and rank per-user candidate lists (re-ranking a shortlist; evaluation against sampled negatives) -----------
 * The opposite shape of K4 / K8: many rows, a short list of candidate columns each -- a gather of nnz item rows, no matrix product.
 * U, user_idx, n_rows, Vt, bias, n_cols, k, mask, mask_pitch: exactly those of tkr_score_topk (user_idx, bias, mask nullable; a mask
 * needs mask_pitch >= n_rows).  cand_ptr [n_rows+1] int64 (starts at 0, never decreases), cand_cols [cand_ptr[n_rows]] int32: the
 * candidate columns of every row as CSR, STRICTLY ASCENDING inside a row and in [0, n_cols) (no duplicates; the caller's contract --
 * top-k-rec_amd/tkr_hip.py rank_candidates checks the pointer, evaluate._group builds such rows).  For entry e of row r, c = cand_cols[e]:
 *   score_out[e] = s(r, c), masked entries included: the mode-1 score of K4 (the fma chain with the two k-halves interleaved, fl(acc +
 *                  bias), -0.0 -> +0.0; csrc/score_chain.h exact_score, restated by oracle/ref_np.py mfma_chain_scores), at every k
 *   rank_out[e]  = -1 when c is masked for the row, otherwise
 *                  #{e' in row r, unmasked, e' != e : s(r, c_e') > s(r, c_e) or (s equal and c_e' > c_e)}
 * -- K4's canonical order restricted to the list.  Integer and bit-exact; no atomics; two runs give the same bits, and a block of rows
 * ranked alone gives what it gives inside a larger call.  When a row lists every column 0 .. n_cols-1, the entry with rank p < K is
 * position p of tkr_score_topk's list with the same score bits (every k; tests/test_gpu_score_chain.py),
 * and the rank of every liked column is tkr_like_ranks's rank (every k).  A column outside [0, n_cols) is never dereferenced: score
 * -inf, rank -1.  ">" and "equal" are those of K4's canonical order over every fp32 value: a NaN score (any sign, any payload) is
 * above +inf and ties with every other NaN; score_out holds a NaN for it.
 * Shapes: any k, empty rows, any n_rows, a row of any length up to n_cols.  A row of at most TKR_CANDIDATES_RESIDENT entries belongs to
 * one wave from first score to last rank (a lane per candidate on the chain; the item rows of 64 candidates at a time come through LDS
 * in slabs of k when k % 8 == 0, otherwise every lane gathers its own; the list's 32-bit ordered keys stay in LDS and lane e counts
 * the keys ahead of its own) -- lists of tens to a few thousand are the design point.  A longer row is still right
 * but slow: a whole workgroup scores it, then counts it in tiles of TKR_CANDIDATES_RESIDENT keys rebuilt from score_out, quadratic in
 * its length (40,000 entries: tens of milliseconds).  A caller that ranks most of the catalogue for a row wants tkr_score_topk /
 * tkr_like_ranks instead.
 * Arguments are checked before any device access and before any launch (TKR_E_INVAL): null U / Vt / cand_ptr / cand_cols / outputs,
 * n_rows <= 0, n_cols <= 0, k <= 0, a mask with mask_pitch < n_rows. */
#define TKR_CANDIDATES_RESIDENT 2048
int tkr_rank_candidates(const float* U, const int32_t* user_idx, int32_t n_rows, const float* Vt, const float* bias,
                        int32_t n_cols, int32_t k, const int64_t* cand_ptr, const int32_t* cand_cols, const uint32_t* mask,
                        int32_t mask_pitch, float* score_out, int32_t* rank_out, void* stream);

/* ---- K9: fold-in -- user vectors for histories the model was not trained on (new design: the reference can only retrain) ----
 * For each of m users, `steps` times: the step of K2 (single/bpr.py:81-100) on a batch of `triplets` triplets that all carry this user,
 * with the item side FROZEN --  x_p = b_i - b_j + <u, v_i - v_j>,  g = sum_p [-sigma(-x_p) (v_i - v_j) + lu u]  (mode 1: lu sign(u)),
 * summed in the order p = 0 .. triplets-1, then one RMSProp update of u (slot from 1.0, rho 0.9, eps 1e-10 as K2).  V, b are read only.
 *   V [n_items, k], b [n_items] (nullable)   the exported item factors and biases (fie / fib: a VBPR model folds in unchanged)
 *   hist_ptr [m+1] int64 (starts at 0), hist_cols int32   the positives of every user as CSR, ascending and unique inside a row, every
 *                         column in [0, n_items) (the CSR of tkr_build_rated_mask)
 *   U0 [m, k] (nullable: zeros)   start vectors; the gradient at zero is not zero
 *   U [m, k]                      result;  loss [m] (nullable): the objective of the LAST step at its pre-step u, as K2's loss_out with
 *                                 lambda_i = lambda_j = lambda_b = 0: sum_p log(1 + exp(-x_p)) + triplets * lu |u|^2 / 2  (mode 1: lu |u|_1)
 *   trip [m, steps, triplets, 2] int32 (nullable)   the drawn (i, j), for tests
 * The draw: positive uniform over the row, negative uniform over the columns not in it -- K1's rounds, membership test and cyclic
 * fallback (csrc/sampler_draw.h) on Philox counter (g & 0xffffffff, g >> 32, round, 1), g = ((first_row + x) * steps + t) * triplets + p
 * (mod 2^64), key = seed: K1 has 0 in the fourth counter word, so the stream is disjoint from training under one seed, and rows
 * [a, b) of a call with first_row = f equal a call on those rows alone with first_row = f + a.
 * A row with no column, or with all n_items of them, has no triplet: U = U0, loss = 0, its part of trip is not written.
 * One wave per user, the row in registers up to k = 512; above, the generic form keeps u, its slot and the gradient sum in one
 * workgroup's LDS (12 k bytes <= 160 KB, i.e. k <= 13,653; wider: TKR_E_UNSUPPORTED).  1 <= triplets <= 64, steps >= 1; arguments are
 * checked before any device access (TKR_E_INVAL).  Deterministic: bitwise the same U run to run. */
int tkr_bpr_foldin(const float* V, const float* b, int32_t n_items, int32_t k, const int64_t* hist_ptr, const int32_t* hist_cols,
                   int32_t m, const float* U0, float lu, float lr, int32_t mode, int32_t steps, int32_t triplets, uint64_t seed,
                   uint64_t first_row, float* U, float* loss, int32_t* trip, void* stream);

/* ---- K10: fold-in of items -- rows and biases for items that were no line of `vid` at training time (new design, the twin of K9) ----
 * For each of m new items x, `steps` times: the step of K2 on `triplets` triplets that all carry x, everything but (v_x, b_x) FROZEN.
 *   role 1, x the positive of a liker u:      x_p = b_x - b_j + <u, v_x - v_j>;  grad v_x += -s u + li v_x,  grad b_x += -s + lb b_x
 *   role 0, x the negative of a non-liker u:  x_p = b_i - b_x + <u, v_i - v_x>;  grad v_x += +s u + lj v_x,  grad b_x += +s + lb b_x
 * with s = sigma(-x_p) (mode 1: li sign(v_x), lb sign(b_x) ...), summed in the order p = 0 .. triplets-1, then one RMSProp update of
 * v_x and one of b_x (slots from 1.0, rho 0.9, eps 1e-10 as K2).  U, V, b are read only.
 *   U [n_users, k], V [n_items, k], b [n_items] (nullable: no bias enters the score, none is learnt, bn = b0)
 *   user_ptr [n_users+1] int64, user_cols int32   the users' training positives as CSR, ascending and unique inside a row, every column
 *                         in [0, n_items) (the CSR tkr_bpr_foldin documents)
 *   liker_ptr [m+1] int64, liker_rows int32       the user rows that like each new item, ascending and unique, in [0, n_users)
 *   role_thresh [m] uint32   a triplet has role 1 iff the first word of its round-0 Philox block is < role_thresh[x]; 0xffffffff: always,
 *                         0: never (foldin.fold_in_items derives it from the rates of the model's own sampler)
 *   V0 [m, k], b0 [m] (nullable: zeros)   start values
 *   Vn [m, k], bn [m]     results;  loss [m] (nullable): the objective of the LAST step at its pre-step values, the terms that depend on
 *                         (v_x, b_x): sum_p log(1 + exp(-x_p)) + (n1 li + n0 lj) |v_x|^2 / 2 + (n1 + n0) lb b_x^2 / 2  (mode 1: |.|_1, |.|)
 *   trip [m, steps, triplets, 3] int32 (nullable)   the drawn (role, u, other item), for tests
 * The draw, on Philox counter (g & 0xffffffff, g >> 32, round, 2), g = ((first_row + x) * steps + t) * triplets + p (mod 2^64), key =
 * seed -- K1 has 0 and K9 has 1 in the fourth word: round 0 gives the role (word 0) and a pick from a list (words 2, 3: role 1 the
 * user among the likers, role 0 the positive in the found user's row); rounds 1 .. 64 and a cyclic scan give, role 1, the negative j
 * not in u's row exactly as K1 does and, role 0, the user: two candidates a round over [0, n_users), legal = has a row and is not a
 * liker.  Items [a, b) of a call with first_row = f equal a call on those items alone with first_row = f + a.
 * A triplet without a legal draw (role 1: no liker, or u's row is the whole catalogue; role 0: every user with a row is a liker) is
 * recorded as (-1, -1, -1) and contributes nothing; a step without any triplet changes nothing, so an item without any keeps V0, b0,
 * loss 0.  The scan of role 0 is bounded by n_users.
 * One wave per item, the row in registers up to k = 512, in LDS above (12 k bytes <= 160 KB; wider: TKR_E_UNSUPPORTED), as K9.
 * 1 <= triplets <= 64, steps >= 1; arguments are checked before any device access (TKR_E_INVAL); m = 0 returns 0 and launches nothing.
 * Deterministic: bitwise the same run to run. */
int tkr_bpr_foldin_items(const float* U, const float* V, const float* b, int32_t n_users, int32_t n_items, int32_t k,
                         const int64_t* user_ptr, const int32_t* user_cols, const int64_t* liker_ptr, const int32_t* liker_rows,
                         const uint32_t* role_thresh, int32_t m, const float* V0, const float* b0, float li, float lj, float lb, float lr,
                         int32_t mode, int32_t steps, int32_t triplets, uint64_t seed, uint64_t first_row, float* Vn, float* bn,
                         float* loss, int32_t* trip, void* stream);

/* ---- multi-GPU: pack / unpack of the replicated item-side tables around the per-epoch all-reduce ---------
 * (new design, the reference is single-process: SURVEY.md §8e).  Users are sharded over the GPUs, every rank updates its
 * own copy of the item tables and once per epoch  P <- P0 + sum_g (P_g - P0),  ms <- mean_g ms_g.  For a table
 * P, ms [2][n][w] whose current row r lives in buffer (cnt[r] & 1) (cnt NULL: a single-buffered [n][w] table):
 *   tkr_sync_snapshot  start[r] = current P[r]                                   (at the start of the epoch)
 *   tkr_sync_pack      flat_delta[r] = current P[r] - start[r];  flat_ms[r] = current ms[r] * inv_world
 *   (the caller all-reduces flat_delta | flat_ms with SUM: RCCL over xGMI through torch.distributed)
 *   tkr_sync_unpack    P[0][r] = start[r] + flat_delta[r];  ms[0][r] = flat_ms[r];  the caller then zeroes cnt */
int tkr_sync_snapshot(const float* P, const int32_t* cnt, float* start, int64_t n, int32_t w, void* stream);
/* the same exchange for the granule tables of tkr_flow_state (item side: V, msV, tailV, rdV; n = n_items): start / flat_delta /
 * flat_ms hold the n*k elements of V followed by the n item biases.  tkr_sync_flow_unpack leaves the tables as a fresh assignment
 * does (version 0 in buffer 0, none in the others, expect = rd = 0) and zeroes the update counters itself.  item_bufs = 2 or 4:
 * the buffers per item row of the tables (tkr_flow_state.item_bufs). */
int tkr_sync_flow_snapshot(const void* V, const void* tailV, const int32_t* icnt, float* start, int32_t n, int32_t k, int32_t item_bufs,
                           void* stream);
int tkr_sync_flow_pack(const void* V, const void* msV, const void* tailV, const int32_t* icnt, const float* start, float* flat_delta,
                       float* flat_ms, int32_t n, int32_t k, float inv_world, int32_t item_bufs, void* stream);
int tkr_sync_flow_unpack(void* V, void* msV, void* tailV, uint32_t* rdV, int32_t* icnt, float* start /* in: epoch start; out: the new
                         values = the next epoch's start (no snapshot needed if nothing else writes the tables in between) */,
                         const float* flat_delta, const float* flat_ms, int32_t n, int32_t k, int32_t item_bufs, void* stream);
int tkr_sync_pack(const float* P, const float* ms, const int32_t* cnt, const float* start, float* flat_delta, float* flat_ms,
                  int64_t n, int32_t w, float inv_world, void* stream);
int tkr_sync_unpack(float* P, float* ms, const float* start, const float* flat_delta, const float* flat_ms, int64_t n, int32_t w,
                    void* stream);

/* ---- profiling aid: dst[r] = src[r] + 1 for the n listed rows of a [*, k] table, with the step
 * kernels' access pattern; used by scripts/pmc_calibrate.py to calibrate rocprofv3 byte counters */
int tkr_calib_rowcopy(const float* src, float* dst, const int32_t* rows, int32_t n, int32_t k, void* stream);

/* ---- host-side text I/O of the reference's data formats (no GPU work) ------------
 * The reference parses its inputs with per-element Python loops (utils.py:58-70 get_data_from_file,
 * evaluate.py:30-45 get_history and :84-93 the test file, utils.py:28-44 / evaluate.py:19-28 the '%f ' matrices,
 * utils.py:47-55 the writer); these do the same in one pass and return flat arrays.
 *
 * id map: token -> index, built from the n '\n'-separated tokens of `blob` (no trailing newline) and their
 *   indices (the host passes the reference's own dict, duplicate-line quirk of utils.py:10-16 included).
 * ratings ("uid,iid:like,iid:like,..." per line): one record per line -- line_user[l] = index of the uid or -1,
 *   entries [line_ptr[l], line_ptr[l+1]) in field order with item[e] = index of the iid or -1 and like[e] = the
 *   integer after the first ':' (a field without ':' or with a non-integer like -> TKR_E_PARSE, where the
 *   reference raises IndexError / ValueError).  Which entries count (known user, known item, like == 1, last line
 *   of a user wins, ...) is the caller's rule, as it differs between utils.py:58-70, evaluate.py:30-45 and :84-93.
 * matrix: every line parsed as ' '-separated decimal numbers (strtod, narrowed to fp32: the two roundings of
 *   np.float32(str)); ragged rows -> TKR_E_PARSE.  tkr_matrix_write emits "%f " per element and '\n' per row,
 *   byte-identical to utils.py:47-55.
 * Handles are created by *_create / *_parse / *_read and released by *_destroy. */
int tkr_idmap_create(const char* blob, int64_t blob_len, const int32_t* index, int64_t n, void** out_map);
int tkr_idmap_destroy(void* map);
int tkr_ratings_parse(const char* path, const void* user_map, const void* item_map, void** out_ratings);
int tkr_ratings_sizes(const void* ratings, int64_t* n_lines, int64_t* n_entries);
int tkr_ratings_copy(const void* ratings, int32_t* line_user, int64_t* line_ptr /*[n_lines+1]*/, int32_t* item,
                     int32_t* like);
int tkr_ratings_destroy(void* ratings);
int tkr_matrix_read(const char* path, void** out_matrix);
int tkr_matrix_sizes(const void* matrix, int64_t* rows, int64_t* cols);
int tkr_matrix_copy(const void* matrix, float* dst /*[rows*cols]*/);
int tkr_matrix_destroy(void* matrix);
int tkr_matrix_write(const char* path, const float* data, int64_t rows, int64_t cols);

/* ---- K11: tkr_ratings_parse on the device (csrc/parse_dev.hip) ------------------------------------
 * The same four arrays as tkr_ratings_parse / tkr_ratings_copy, bit for bit, from the n_bytes bytes of the file in device memory
 * (`text`, 16-byte aligned; NULL only for n_bytes == 0).  Same rules: lines end at '\n' only, a last line without one counts, a line
 * is stripped of ' ' \t \n \r \v \f at both ends, every ',' opens one field, the iid token is the unstripped bytes before the
 * field's first ':', like is the stripped decimal integer (optional sign, saturating at +-2,147,483,647) between the first and
 * the second ':' or the field end.  All offsets and counts are 64-bit.  No kernel reads outside [0, n_bytes).
 *
 * Two calls with one read-back between them, because the outputs are sized by what the first one counts:
 *   tkr_ratings_count_dev   totals_out (device int64[2]) = {n_lines, n_entries}; fills `workspace` (16-byte aligned,
 *                           tkr_parse_dev_workspace_bytes(n_bytes, chunk_bytes) bytes) with the per-chunk offsets
 *   tkr_ratings_emit_dev    with the SAME text, chunk_bytes and workspace and the totals read back: line_user int32[n_lines],
 *                           line_ptr int64[n_lines + 1], item / like int32[n_entries]; line_start int64[n_lines] is scratch.
 *                           status (device int64): -1, or the smallest start offset of a malformed field (no ':', or a like
 *                           that is no such integer) -- the caller's TKR_E_PARSE; the arrays are then not to be used.
 * chunk_bytes: a power of two, 64 ... 1,048,576: the piece of text one wave counts and walks.  It changes no output.
 *
 * Token lookup: an open-addressing table per id list.  tkr_idtable_build (HOST call, host pointers) lays it out from the blob
 * and index array tkr_idmap_create takes: slots int32[n_slots][4] = {offset into blob, length (-1 = empty), index, hash},
 * n_slots = tkr_idtable_slots(n) (a power of two >= 2 n, >= 8), linear probing from hash & (n_slots - 1), hash = FNV-1a of the
 * token's bytes with h ^= h >> 15 at the end.  A token listed twice keeps its last index.  The caller uploads slots (16-byte
 * aligned) and blob (4-byte aligned, < 2^31 bytes) and passes both to tkr_ratings_emit_dev; a hit compares the bytes.
 * Arguments are checked before any device access (TKR_E_INVAL; the two size functions return it as their value). */
int64_t tkr_parse_dev_workspace_bytes(int64_t n_bytes, int64_t chunk_bytes);
int64_t tkr_idtable_slots(int64_t n);
int tkr_idtable_build(const char* blob, int64_t blob_len, const int32_t* index, int64_t n, int32_t* slots, int64_t n_slots);
int tkr_ratings_count_dev(const void* text, int64_t n_bytes, int64_t chunk_bytes, void* workspace, int64_t workspace_bytes,
                          int64_t* totals_out, void* stream);
int tkr_ratings_emit_dev(const void* text, int64_t n_bytes, int64_t chunk_bytes, void* workspace, int64_t workspace_bytes,
                         int64_t n_lines, int64_t n_entries, const int32_t* user_slots, int64_t user_n_slots,
                         const void* user_blob, int64_t user_blob_len, const int32_t* item_slots, int64_t item_n_slots,
                         const void* item_blob, int64_t item_blob_len, int64_t* line_start, int32_t* line_user,
                         int64_t* line_ptr, int32_t* item, int32_t* like, int64_t* status, void* stream);

/* ---- K13: the text writers on the device (csrc/format_dev.hip) --------------------------------------------------------------
 * Replace the per-field Python formatting of recommend.py:50-56 (format_lines: one '%s:%f' expression and one dict lookup per list
 * entry) with the write loop of recommend.py:239-241, and the one-thread sprintf("%f ") loop of tkr_matrix_write
 * (csrc/textio.hip:263-283; utils.py:47-55 in the reference).  The bytes are those of glibc printf / Python's '%f' % float(x) for
 * every fp32 bit pattern: round half to even on the exact binary value, a set sign bit always prints '-', +-inf as inf / -inf,
 * every NaN as nan; computed with integers only, |x| >= 2^64 included (no host fall-back).  A value takes at most 47 bytes.
 *
 * lists: row r of ids int32[n][K] / scores fp32[n][K] becomes "uid,iid:%f,iid:%f,...\n", uid = token row_user[r] of the user table,
 *   iid = token ids[r][j] of the item table; a negative id is skipped wherever it stands; a row without a valid entry is the uid alone.
 *   A token table is addressed by index: token i = blob[start[i], start[i] + len[i]), len[i] = -1: no token has index i; blob_len
 *   <= 2^29.  A row_user or a non-negative id outside its table, one that names an empty slot, or a token outside its blob sets
 *   the status word to the row number (atomic min: the first such row); the text is then not to be used.
 * matrix: row r of data fp32[rows][cols] becomes "%f " per element and '\n' (cols = 0: the '\n' alone), as tkr_matrix_write.
 *
 * Two calls with one read-back between them, because the text is sized by what the first one counts:
 *   *_sizes_dev   line_ptr (device int64[n + 1]) = the offset of every row in the text, line_ptr[n] = its size; totals (device
 *                 int64[2]) = {size of the text, status: -1 or the first offending row}.  No workspace: the row lengths are summed
 *                 in place in line_ptr by one workgroup (no library scan).
 *   *_emit_dev    with the SAME inputs and line_ptr: rows [first_row, first_row + n_rows) of the text into out[0, out_bytes)
 *                 (16-byte aligned), the byte at offset q of the whole text at out[q - line_ptr[first_row]].  status (device int64):
 *                 -1, or a row whose line_ptr entries do not lie in the block or do not match its text.  Nothing is stored outside
 *                 [line_ptr[r] - line_ptr[first_row], line_ptr[r + 1] - line_ptr[first_row]) of a row, whatever the arrays hold.
 * All offsets are 64-bit.  Arguments are checked before any device access (TKR_E_INVAL).  Deterministic. */
int tkr_lists_format_sizes_dev(const int32_t* ids, const float* scores, const int32_t* row_user, int64_t n, int32_t K,
                               const void* user_blob, int64_t user_blob_len, const int64_t* user_start, const int32_t* user_len,
                               int64_t n_users, const void* item_blob, int64_t item_blob_len, const int64_t* item_start,
                               const int32_t* item_len, int64_t n_items, int64_t* line_ptr, int64_t* totals, void* stream);
int tkr_lists_format_emit_dev(const int32_t* ids, const float* scores, const int32_t* row_user, int64_t n, int32_t K,
                              const void* user_blob, int64_t user_blob_len, const int64_t* user_start, const int32_t* user_len,
                              int64_t n_users, const void* item_blob, int64_t item_blob_len, const int64_t* item_start,
                              const int32_t* item_len, int64_t n_items, const int64_t* line_ptr, int64_t first_row, int64_t n_rows,
                              void* out, int64_t out_bytes, int64_t* status, void* stream);
int tkr_matrix_format_sizes_dev(const float* data, int64_t rows, int64_t cols, int64_t* line_ptr, int64_t* totals, void* stream);
int tkr_matrix_format_emit_dev(const float* data, int64_t rows, int64_t cols, const int64_t* line_ptr, int64_t first_row,
                               int64_t n_rows, void* out, int64_t out_bytes, int64_t* status, void* stream);

/* ---- K14: tkr_matrix_read on the device (csrc/scan_dev.hip, csrc/scan_num.h) ---------------------------------------------------
 * The same fp32 array as tkr_matrix_read / tkr_matrix_copy, bit for bit, from the n_bytes bytes of the file in device memory (`text`,
 * 16-byte aligned; NULL only for n_bytes == 0).  The rules are the host reader's: lines end at '\n' only, a last line without one
 * counts, a line is stripped of ' ' \t \n \r \v \f at both ends, tokens are split on ' ' only (an empty token is TKR_E_PARSE), every
 * token goes through strtod, must be consumed whole and is narrowed with (float) -- two roundings, decimal -> 53 bits -> 24 bits,
 * both to nearest even ("1.0000000596046448" is 0x3f800000, not 0x3f800001) --, cols is the first line's token count and any
 * other count is TKR_E_PARSE.  The device decides nothing about malformed input.  It does two jobs:
 *
 * Layout.  A file is CANONICAL when it holds none of \t \r \v \f, its first byte is a token byte (anything but ' ' and '\n'), it
 *   holds none of the pairs "  ", "\n ", "\n\n", and every line has as many tokens as the first.  Then a token starts at p when
 *   byte[p] is a token byte and p == 0 or byte[p - 1] is ' ' or '\n', and runs to the next ' ', '\n' or the end: the host's
 *   tokenisation.  The empty file is canonical, shape (0, 0).  For any other file the status word holds the smallest offset that
 *   breaks a rule (-1: none); the caller then hands the WHOLE file to tkr_matrix_read, which returns the array or TKR_E_PARSE.
 * Tokens.  A token is PLAIN when it is [+-]? digits* ('.' digits*)? with at least one digit, at most 19 digits from its first
 *   non-zero digit to its last and at most 19 behind the '.': w / 10^f with w < 10^19 and 10^f < 2^64, converted exactly with
 *   64-bit integers (a 64-step restoring division, the remainder as the sticky bit, the two roundings above).  Its value is 0
 *   (keeping its sign: "-0.000000" is 0x80000000) or lies in [1e-19, 1e19).  Every other token is HARD (exponent forms, inf, nan,
 *   hex floats, longer digit strings, garbage): its bit in `hard` is set, data holds 0 there, and the caller runs
 *   tkr_matrix_tokens_host on those tokens -- the very check of tkr_matrix_read -- and patches the results in.
 *
 * Two calls with one read-back between them, because the outputs are sized by what the first one counts:
 *   tkr_matrix_count_dev    totals_out (device int64[3]) = {n_lines, n_tokens, layout status}; fills `workspace` (16-byte aligned,
 *                           tkr_scan_dev_workspace_bytes(n_bytes, chunk_bytes) bytes) with the per-chunk offsets
 *   tkr_matrix_emit_dev     with the SAME text, chunk_bytes and workspace, the totals read back and cols = the token count of the
 *                           first line (the host counts it): tok_start int64[n_tokens] = the offset of every token, data
 *                           fp32[n_tokens] = row-major values, hard uint64[(n_tokens + 63) / 64] = bit (i & 63) of word i >> 6
 *                           for token i, counts (device int64[2]) = {layout status, n_hard}.  The status is set here when a line
 *                           does not start at token line * cols (its start offset), or n_lines * cols != n_tokens (n_bytes).
 * chunk_bytes: a power of two, 64 ... 1,048,576: the piece of text one wave counts and walks.  It changes no output.
 * A token or a line may straddle any number of chunks.  All offsets are 64-bit.  No kernel reads outside [0, n_bytes).  The only
 * atomic is the status word's atomic min.  Deterministic.  Arguments are checked before any device access (TKR_E_INVAL; the size
 * function returns it as its value).
 *
 * HOST calls (host pointers, no GPU):
 *   tkr_matrix_token_host   the device's classify-and-convert routine run on the CPU on tok[0, len): 1 = plain, *out converted;
 *                           0 = hard, *out untouched; TKR_E_INVAL on bad arguments
 *   tkr_matrix_tokens_host  for k < n the token of text[0, n_bytes) that starts at start[k] and runs to the next ' ', '\n' or the
 *                           end: out[k] = (float)strtod(token), TKR_E_PARSE where tkr_matrix_read would return it */
int64_t tkr_scan_dev_workspace_bytes(int64_t n_bytes, int64_t chunk_bytes);
int tkr_matrix_count_dev(const void* text, int64_t n_bytes, int64_t chunk_bytes, void* workspace, int64_t workspace_bytes,
                         int64_t* totals_out, void* stream);
int tkr_matrix_emit_dev(const void* text, int64_t n_bytes, int64_t chunk_bytes, void* workspace, int64_t workspace_bytes,
                        int64_t n_lines, int64_t n_tokens, int64_t cols, int64_t* tok_start, float* data, uint64_t* hard,
                        int64_t* counts, void* stream);
int tkr_matrix_token_host(const char* tok, int64_t len, float* out);
int tkr_matrix_tokens_host(const char* text, int64_t n_bytes, const int64_t* start, int64_t n, float* out);

/* ---- K15: parsed ratings -> CSR rows on the device (csrc/group_dev.hip) ---------------------------------------------------------
 * What evaluate._group builds for rows that arrive grouped.  A SOURCE is a set of n_seg segments over n_entries entries: segment g is
 * the entries [seg_ptr[g], seg_ptr[g + 1]) of item (and like) -- the lines of a parsed ratings file (seg_ptr = line_ptr of
 * tkr_ratings_emit_dev) or the rows of a CSR -- and seg_of_row[r] names the segment that feeds row r: -1 none, NULL the identity
 * (then n_seg >= n_rows).  An entry counts when item >= 0 and, with like_only != 0, like == 1 (like may be NULL without like_only).
 * Row r of the result is the ascending, duplicate-free union of the counted items of its segment in each of the n_src (1 or 2)
 * sources; ptr is the 64-bit exclusive prefix of the row sizes.  All pointers but `src` itself are device pointers.
 *
 * Two calls with one read-back between them, because cols is sized by what the first one counts:
 *   tkr_group_count_dev   ptr int64[n_rows + 1]; totals (device int64[2]) = {ptr[n_rows], status}
 *   tkr_group_emit_dev    with the SAME sources and ptr: cols int32[n_out], n_out = ptr[n_rows]; status (device int64)
 * A row's set is a bitmap of n_cols bits in LDS (no sort): one wave per row while n_cols <= TKR_GROUP_WAVE_COLS, one workgroup per row
 * up to TKR_GROUP_MAX_COLS (what the 160 KB of a CU hold); above that both return TKR_E_UNSUPPORTED.  Rows of any length run.
 * The input is not trusted.  status: -1, or the smallest 4 * index + kind of what was refused: kind 0 -- seg_of_row[index] outside
 * [-1, n_seg); 1 -- seg_ptr decreases at segment `index`, or leaves [0, n_entries] (every segment is checked; kind 1 with a row as
 * index when the row met it first); 2 -- row `index` holds a counted item >= n_cols; 3 (emit) -- ptr is not the ptr of these
 * sources at row `index`.  What is refused is never used as an index; the outputs are then not to be used.  Deterministic.
 *
 *   tkr_last_line_of_user_dev   last int64[n_users]: the largest line i with line_user[i] == u, -1 where none (a line_user outside
 *                               [0, n_users) belongs to nobody)
 *   tkr_compact_rows_count_dev  pos int64[n_rows + 1]: exclusive count of the rows of the CSR `ptr` with at least one element;
 *                               pos[n_rows] = n_kept, which the caller reads back
 *   tkr_compact_rows_emit_dev   rows int64[n_kept]: those rows, ascending; out_ptr int64[n_kept + 1]: the ptr of the CSR that keeps
 *                               only them (the same cols); status: -1, or 4 * row + 3 when pos is not the pos of this ptr
 * Arguments are checked before any device access (TKR_E_INVAL: a NULL that is not allowed, n_rows / n_cols / n_lines / n_users < 1). */
#define TKR_GROUP_WAVE_COLS 32768
#define TKR_GROUP_MAX_COLS 1308672
typedef struct tkr_group_source {
    const int64_t* seg_ptr;    /* [n_seg + 1] */
    const int32_t* item;       /* [n_entries] */
    const int32_t* like;       /* [n_entries] or NULL */
    const int64_t* seg_of_row; /* [n_rows] or NULL */
    int64_t n_seg, n_entries;
} tkr_group_source;
int tkr_group_count_dev(const tkr_group_source* src, int32_t n_src, int64_t n_rows, int32_t n_cols, int32_t like_only,
                        int64_t* ptr, int64_t* totals, void* stream);
int tkr_group_emit_dev(const tkr_group_source* src, int32_t n_src, int64_t n_rows, int32_t n_cols, int32_t like_only,
                       const int64_t* ptr, int32_t* cols, int64_t n_out, int64_t* status, void* stream);
int tkr_last_line_of_user_dev(const int32_t* line_user, int64_t n_lines, int64_t n_users, int64_t* last, void* stream);
int tkr_compact_rows_count_dev(const int64_t* ptr, int64_t n_rows, int64_t* pos, void* stream);
int tkr_compact_rows_emit_dev(const int64_t* ptr, const int64_t* pos, int64_t n_rows, int64_t n_kept, int64_t* rows,
                              int64_t* out_ptr, int64_t* status, void* stream);

/* ---- K16: the weights of a linear fusion of several trained models (csrc/fusion.hip) ----------------------------------------------
 * Replaces the learning half of the reference's old/methods/bfusion.py + ranking_fusion.py and efusion.py.  (Serving a fused model
 * needs no entry point: top-k-rec_amd/fusion.py concatenates the tables.)  The models arrive in one struct: n_models <= 16 table pairs
 * over the same n_users and n_items, each with its own width k (= its row pitch) and an optional bias [n_items].  All pointers inside
 * are device pointers; the struct itself is read on the host.
 * The per-model score s_m(u, c) is the score of tkr_rank_candidates / tkr_score_topk bit for bit (csrc/score_chain.h exact_score: the
 * fma chain with the two k-halves interleaved, fl(acc + bias), -0.0 -> +0.0; oracle/ref_np.py mfma_chain_scores), one lane per score.
 *
 *   tkr_fusion_features      triplet g = first_triplet + t, t < count, is K1's draw (tkr_sample_plan's stream under `seed`:
 *                            oracle/plan_np.py sample_triplets) on the CSR tr_users / row_ptr / pos_cols / cols_sorted;
 *                            D_out[t, m] = fl(s_m(u, i) - s_m(u, j)), fp32 [count, n_models]; trip_out (nullable) int32 [count, 3] =
 *                            (u, i, j).  A lane per triplet; no atomics, no workspace.  A drawn id outside the tables is never used
 *                            as an index (the row of D is NaN).
 *   tkr_fusion_sgd           the loop of ranking_fusion.py:48-54 on D [n_rows, n_models]: for batch z = 0 .. n_batches-1 (rows
 *                            [z * batch, (z + 1) * batch); n_batches * batch <= n_rows), with x_t = sum_m W[m] D[t, m] (an fma chain, m
 *                            ascending) on the W from before the update:
 *                              loss_out[z] = sum_t log(1 + e^-x_t) + lambda_w / 2 * sum_m W[m]^2         (nullable)
 *                              W[m] += lr * (sum_t sigma(-x_t) D[t, m] - lambda_w W[m])
 *                            W fp32 [n_models] in/out.  ONE workgroup walks the batches; every sum goes through one fixed tree (DPP
 *                            inside a wave, the waves in wave order), and the thread of a row depends on the row's place in its batch
 *                            alone: two runs give the same bits, and so does a call cut into calls of whole batches with W carried.
 *   tkr_fusion_user_weights  efusion.py:57-82 on the CSR of the users' training likes (like_ptr int64 [n_users + 1] from 0, like_cols
 *                            int32, a SET per row):  r[u, m] = sqrt(sum_{c in likes(u)} (s_m(u, c) - 1)^2 / max(|likes(u)|, 1)),
 *                            w[u, m] = exp(-(r[u, m] - mean_m r[u, .])), and 1.0 where that mean is exactly 0 (an empty row; the
 *                            reference leaves 0 there).  rmse_out, w_out fp32 [n_users, n_models].  A wave per user, rows of any
 *                            length.  A column outside [0, n_items) is never dereferenced (the user's figures are NaN).
 * Arguments are checked before any device access and before any launch (TKR_E_INVAL): a NULL that is not allowed, n_models outside
 * [1, 16], a model without U or V or with k < 1, n_items / n_users that differ from the struct's, count / batch / n_batches < 1,
 * n_batches * batch > n_rows. */
#define TKR_FUSION_MAX_MODELS 16
typedef struct tkr_fusion_model {
    const float* U;    /* [n_users, k] */
    const float* V;    /* [n_items, k] */
    const float* bias; /* [n_items] or NULL */
    int32_t k, reserved;
} tkr_fusion_model;
typedef struct tkr_fusion_models {
    tkr_fusion_model m[TKR_FUSION_MAX_MODELS];
    int32_t n_models, n_users, n_items, reserved;
} tkr_fusion_models;
int tkr_fusion_features(const tkr_fusion_models* models, const int32_t* tr_users, int32_t n_tr, const int32_t* row_ptr,
                        const int32_t* pos_cols, const int32_t* cols_sorted, int32_t n_items, uint64_t seed, uint64_t first_triplet,
                        int64_t count, float* D_out, int32_t* trip_out, void* stream);
int tkr_fusion_sgd(const float* D, int64_t n_rows, int32_t n_models, int32_t batch, int64_t n_batches, float lr, float lambda_w, float* W,
                   float* loss_out, void* stream);
int tkr_fusion_user_weights(const tkr_fusion_models* models, const int64_t* like_ptr, const int32_t* like_cols, int32_t n_users,
                            float* rmse_out, float* w_out, void* stream);

/* ---- K23: the sums of one Newton pass of the SVM fusion (csrc/fusion_svm.hip) -------------------------------------------------------
 * The reference's old/methods/sfusion.py fits LinearSVC(C) to the score differences of sampled triplets, row t as +d_t with label +1
 * (t even) or as -d_t with label -1 (t odd): squared hinge, L2 penalty, the intercept regularised as one more feature of value 1, i.e.
 *   f(w, b) = (|w|^2 + b^2) / 2 + C sum_t max(0, 1 - z_t)^2,   z_t = w . d_t + y_t b,   y_t = +1 (t even), -1 (t odd).
 * top-k-rec_amd/svmfusion.py minimises f by Newton's method on the host; every pass is one reduction over all rows, done here.
 *
 *   tkr_fusion_svm_sums      D fp32 [n_rows, n_models] as tkr_fusion_features writes it; row t is row g = first_row + t of the run, of
 *                            parity g & 1, x~ = (d, y).  W device fp64 [n_models + 1]: the weights, then the intercept.
 *                            z = sum_m W[m] d[m] + y W[M] in fp64, ONE fma chain, m ascending.  A row is active iff 1 - z > 0 (strictly:
 *                            a row exactly on the hinge adds nothing).  Over the active rows, every term one fp64 fma:
 *                              S      the upper triangle of sum x~ x~^T, row by row: (M + 1)(M + 2) / 2 values
 *                              r      sum (1 - z) x~, M + 1 values
 *                              q      sum (1 - z)^2
 *                              count  the number of active rows
 *                            One workgroup per slab of TKR_FUSION_SVM_SLAB rows, slabs cut at multiples of the slab IN g; lanes and
 *                            waves are combined through one fixed tree, and a slab's sums (S | r | q | count, all fp64) go to
 *                            partial[slab_offset + s], s = 0, 1, ... over the slabs that [first_row, first_row + n_rows) touches.
 *                            With out != NULL a second launch adds partial[0 .. slab_offset + this call's slabs) in ascending order into
 *                            out: fp64 S | r | q, then the count as int64 -- (M + 1)(M + 2) / 2 + M + 3 eight-byte words.  The result
 *                            depends on g alone: two calls give the same bits, and so does a run cut into calls of whole slabs
 *                            (first_row a multiple of the slab, slab_offset carried, out passed to the last call only).
 *                            No float atomics.  A row with an entry that is not finite (tkr_fusion_features writes NaN for an id
 *                            outside the tables) is never summed: *status (device int64, set to -1 by the call with slab_offset 0)
 *                            takes the smallest such g by atomic min, and the second launch then leaves out as it is.
 *   tkr_fusion_svm_partial_bytes   the bytes of partial for the rows [first_row, first_row + n_rows), or TKR_E_INVAL.
 * Arguments are checked before any device access and before any launch (TKR_E_INVAL): a null D / W / partial / status, n_models outside
 * [1, 16], n_rows < 1, first_row < 0 (either above 2^42), slab_offset < 0, a misaligned D / W / partial / out / status, partial_bytes too
 * small for slab_offset + this call's slabs. */
#define TKR_FUSION_SVM_SLAB 4096
int tkr_fusion_svm_sums(const float* D, int64_t n_rows, int32_t n_models, int64_t first_row, const double* W, double* partial,
                        int64_t partial_bytes, int64_t slab_offset, double* out, int64_t* status, void* stream);
int64_t tkr_fusion_svm_partial_bytes(int64_t n_rows, int32_t n_models, int64_t first_row);

/* ---- K17: diversify a pool into a list (greedy MMR) and the pair sums of list diversity (csrc/diversity.hip) ----------------------
 * New design: the reference sorts every list by score alone.  Both entry points are built on the similarity of two entries of a row,
 *   sim(a, b) = chain(S[id_a], S[id_b]),   S fp32 [n_items, k]: whatever the caller measures similarity in (row-normalised item factors
 * for cosine, the factors themselves for dot; top-k-rec_amd/diversity.py prepare), chain = the mode-1 score of K4 / K12 without a bias
 * (csrc/score_chain.h exact_score; oracle/ref_np.py mfma_chain_scores): symmetric bit for bit.
 *
 *   tkr_mmr_select      ids int32 [n_rows, N]: a pool per row, valid up to the first negative id (the -1 padding of tkr_score_topk);
 *                       rel fp32 [n_rows, N]: the relevance of every entry.  sel_pos int32 [n_rows, t]: pool POSITIONS in pick order,
 *                       -1 where the row has fewer than t valid entries.  With lam32 = (float)lam, mu32 = 1.0f - lam32 (fp32) and
 *                       a_e = fl(lam32 * rel_e) (one fp32 multiply, kept): pick 0 = argmax a_e; before pick r > 0, pen_e = the maximum
 *                       over the r picked entries s of sim(e, s) (it may be negative), obj_e = fma(-mu32, pen_e, a_e), pick r = argmax
 *                       of obj_e over the unpicked valid entries; every tie goes to the lower pool position (-0.0 counts as +0.0).
 *                       t * N similarities per row, never an N x N matrix.  1 <= t <= N <= TKR_MMR_MAX_POOL (above: TKR_E_UNSUPPORTED).
 *                       One workgroup per row, a thread per entry; the valid rows of S are staged once in LDS when N rows of it fit
 *                       the 160 KB of a CU, otherwise both rows of every chain are read through L2; any k.
 *   tkr_list_pair_sums  ids int32 [n_rows, t]: the final lists, the same prefix rule; pair_sum float64 [n_rows, t]:
 *                       pair_sum[r, b] = sum over a < b of (1 - sim(a, b)), the subtraction and the sum (a ascending) in float64, 0
 *                       behind the valid prefix.  Intra-list diversity at every cut-off is a prefix sum of a row.
 *                       t <= TKR_MMR_MAX_POOL.
 * An id >= n_items is never dereferenced: it ends its row like a negative id, and the row is reported in `status` (device int64[1],
 * written by the call; K15's convention): -1, or 4 * row + 1 for the smallest such row (bit 0: an id outside the table).  Only the
 * entry that ENDS a row is looked at; what follows it is ignored.  Arguments are checked before any device access and before any
 * launch (TKR_E_INVAL): a null S / ids / rel / output / status, n_items / k / n_rows / N / t < 1, t > N, lam not finite or outside
 * [0, 1].  Deterministic; no atomics but the status word's minimum.  S and every row of it 16-byte aligned when k % 8 == 0. */
#define TKR_MMR_MAX_POOL 1024
int tkr_mmr_select(const float* S, int32_t n_items, int32_t k, const int32_t* ids, const float* rel, int32_t n_rows, int32_t N,
                   double lam, int32_t t, int32_t* sel_pos, int64_t* status, void* stream);
int tkr_list_pair_sums(const float* S, int32_t n_items, int32_t k, const int32_t* ids, int32_t n_rows, int32_t t, double* pair_sum,
                       int64_t* status, void* stream);

/* ---- K18: the metric values of every test line, and their sums over resampled lines (csrc/line_metrics.hip) ---------------------
 * New design: the reference reports one mean per scenario.  What a bootstrap needs on the device, next to K8's output.
 *
 *   tkr_line_metrics    ranks int32 [n_likes]: tkr_like_ranks' output in the order of the like CSR (-1: a rated like); like_ptr,
 *                       rated_ptr int64 [n_lines + 1] (only the row SIZES of the rated CSR are used); gain float64 [total],
 *                       gain[r] = 1 / log2(r + 2); ideal float64 [total + 1], ideal[d] = gain[0] + ... + gain[d - 1] -- both made by the
 *                       caller: the device calls no logarithm.  X float64 [n_lines, C], C = 3 * interval + 5, interval = total / step
 *                       (0 is legal).  For line r with ranks >= 0 rho_0 < rho_1 < ... (P of them), K_b = step * (b + 1) and
 *                       N = n_cols - |rated_r| - P:
 *                         X[r, b]                    = #{q : rho_q < K_b}                                          b < interval
 *                         X[r, interval]             = the line's likes, rated ones included
 *                         X[r, interval + 1], [+ 2]  = 1 - (sum rho_q - P (P - 1) / 2) / (P N) and 1.0 where P >= 1 and N >= 1, else 0, 0
 *                                                      (numerator and P N exact in int64; one division, one subtraction)
 *                         X[r, interval + 3], [+ 4]  = 1 / (rho_0 + 1) and 1.0 where P >= 1, else 0, 0
 *                         X[r, interval + 5 + b]     = (sum_{rho_q < K_b} gain[rho_q]) / ideal[min(P, K_b)], 0 where P = 0
 *                         X[r, 2 interval + 5 + b]   = (sum_{rho_q < K_b} (q + 1) / (rho_q + 1)) / min(P, K_b), 0 where P = 0
 *                       both sums added in ascending q from 0.0, no fused multiply-add: X is defined bit for bit.
 *                       A wave per line, the line's ranks as a bitmap in LDS; a line of any length is two passes over its ranks.
 *                       total <= TKR_LINE_MAX_TOTAL, n_cols <= TKR_LINE_MAX_COLS (above: TKR_E_UNSUPPORTED).
 *                       The input is not trusted.  status (device int64[1], written by the call; K15's convention): -1, or the smallest
 *                       4 * line + kind of what was refused: kind 0 -- a rank below -1; 1 -- a rank >= n_cols - |rated_line|; 2 -- a rank
 *                       >= 0 named twice in the line; 3 -- like_ptr / rated_ptr do not start at 0, descend at this line, leave
 *                       [0, n_likes], or give the line more than n_cols rated columns.  Nothing refused is used as an index; X is then
 *                       not to be used.
 *   tkr_bootstrap_sums  X float64 [n, C], row r at X + r * pitch (pitch >= C doubles); out float64 [R, C]: out[r, c] = sum over t < n of X[idx(r, t), c] -- R resamples of n lines
 *                       with replacement, each applied to all columns.  The draw, on the library's Philox stream with stream word 3
 *                       (0 / 1 / 2: K1 / K9 / K10): w = philox4x32_10(c0 = low word of t >> 1, c1 = its high word, c2 = r, c3 = 3,
 *                       k0 = low word of seed, k1 = high word); idx = mulhi64(w.x, w.y, n) for even t, mulhi64(w.z, w.w, n) for odd t
 *                       (oracle/plan_np.py).  The order of the sum is fixed by (n, C): a wave sums TKR_BOOT_CHUNK consecutive draws
 *                       (L = the power of two >= max(C, 8) lanes read a row; lane group g adds the draws t with t mod (64 / L) = g in
 *                       ascending order; the groups are added in a butterfly), the chunks are added in ascending order.  Two calls
 *                       give the same bits, whatever the pitch; no float atomics.  A pitch of whole 64- or 128-byte lines (8, 16, 32,
 *                       48, 64 doubles) reads faster than rows that straddle lines.  workspace: 8-byte aligned, at least
 *                       R * ceil(n / TKR_BOOT_CHUNK) * C * 8 bytes.  1 <= C <= TKR_BOOT_MAX_COLUMNS, 1 <= n < 2^31, 1 <= R.
 * Arguments are checked before any device access and before any launch (TKR_E_INVAL): a null or misaligned pointer (ranks may be
 * null when n_likes = 0), n_likes < 0, n_lines / n_cols / step / total < 1, C, n or R outside their limits, pitch < C, a workspace too small. */
#define TKR_LINE_MAX_TOTAL 1024
#define TKR_LINE_MAX_COLS 1308672
#define TKR_BOOT_MAX_COLUMNS 64
#define TKR_BOOT_CHUNK 8192
int tkr_line_metrics(const int32_t* ranks, int64_t n_likes, const int64_t* like_ptr, const int64_t* rated_ptr, int64_t n_lines,
                     int32_t n_cols, int32_t step, int32_t total, const double* gain, const double* ideal, double* X, int64_t* status,
                     void* stream);
int tkr_bootstrap_sums(const double* X, int64_t n, int32_t C, int64_t pitch, int32_t R, uint64_t seed, double* out, void* workspace,
                       int64_t workspace_bytes, void* stream);

/* ---- K19: the nearest anchors of every list entry (csrc/explain.hip) ---------------------------------------------------------------
 * New design: the reference writes lists and nothing about them.  "Why is this item on my list?" -- because of the user's own likes
 * whose factors are closest to it; "is the list more of the same?" -- 1 - the similarity of an entry to the nearest item of the
 * history (unexpectedness).  Both are one operation: for every entry of a row's list, the e most similar items of a second, per-row
 * set, the ANCHORS.  sim(a, b) = chain(S[a], S[b]) is K17's similarity exactly: S fp32 [n_items, k] is whatever the caller measures
 * similarity in (top-k-rec_amd/diversity.py similarity_table), chain = the mode-1 score of K4 / K12 without a bias (csrc/score_chain.h
 * exact_score; oracle/ref_np.py mfma_chain_scores), -0.0 mapped to +0.0, symmetric bit for bit; any k.
 *
 *   tkr_nearest_anchors  ids int32 [n_rows, t]: a list per row, valid up to the first id that is negative or >= n_items (K17's prefix
 *                        rule).  Row r's anchors are anchor_cols[anchor_ptr[r] : anchor_ptr[r + 1]] (anchor_ptr int64 [n_rows + 1]
 *                        from 0, anchor_cols int32 [n_anchors]); they need not be sorted or unique, and their POSITIONS, counted from
 *                        the row's start, are what is ranked: a column named twice is two anchors.  For entry (r, p) inside the valid
 *                        prefix the eligible anchors are the positions q with 0 <= anchor_cols[q] < n_items and anchor_cols[q] !=
 *                        ids[r, p] (an item does not explain itself).  best_pos int32 [n_rows, t, e]: the eligible positions in
 *                        descending sim, ties to the lower position; best_sim fp32 [n_rows, t, e]: their similarities, the chain's
 *                        bits.  Where fewer than e anchors are eligible, and everywhere behind the valid prefix: -1 and -inf.
 *                        Similarities are compared through the ordered 32-bit key K12 keeps its scores in (the bits of a float with
 *                        the sign bit set are inverted, all others get the sign bit), so the order is total: NaNs with the sign bit
 *                        < -inf < the negative numbers < +0.0 < the positive numbers < +inf < NaNs without the sign bit (-0.0 does
 *                        not occur).  t <= TKR_ANCHOR_MAX_T, e <= TKR_ANCHOR_MAX_E (above: TKR_E_UNSUPPORTED).
 *                        One workgroup per row; its threads are cut into groups of t, so that a lane holds one (entry, anchor) pair
 *                        at a time and owns its entry's e best as packed 64-bit (key, inverted position) words; the list's rows of S
 *                        are staged once in LDS when t + 8 rows of it fit the 160 KB of a CU, and the anchors' rows stream through LDS
 *                        behind them in tiles (a row of any length, 0 to more than n_items anchors); otherwise both rows of every
 *                        chain are read through L2.
 * The input is not trusted.  status (device int64[1], written by the call; K15's convention): -1, or the smallest 4 * row + kind of
 * what was found: kind 0 -- a list id >= n_items ended the row (only the entry that ENDS a row is looked at); 1 -- an anchor column
 * outside [0, n_items) was skipped; 3 -- anchor_ptr does not start at 0, descends at this row, leaves [0, n_anchors] or gives the row
 * 2^31 anchors or more: that row gets padding only and its anchors are not looked at.  Nothing refused is ever used as an index.
 * Arguments are checked before any device access and before any launch (TKR_E_INVAL): a null S / ids / anchor_ptr / output / status,
 * a null anchor_cols when n_anchors > 0, n_items / k / n_rows / t / e < 1, n_anchors < 0.  Deterministic: two calls give the same
 * bits; no float atomics, the only atomic is the status word's minimum.  S and every row of it 16-byte aligned when k % 8 == 0. */
#define TKR_ANCHOR_MAX_E 8
#define TKR_ANCHOR_MAX_T 1024          /* = TKR_MMR_MAX_POOL */
int tkr_nearest_anchors(const float* S, int32_t n_items, int32_t k, const int32_t* ids, int32_t n_rows, int32_t t,
                        const int64_t* anchor_ptr, const int32_t* anchor_cols, int64_t n_anchors,
                        int32_t e, int32_t* best_pos, float* best_sim, int64_t* status, void* stream);

/* ---- K20: the two halves of an ALS step, implicit feedback (csrc/als.hip) -------------------------------------------------------------
 * Replaces the loops of the reference's single/wmf.py:70-97 (np.dot for the shared Gram, np.linalg.solve per row); the semantics are
 * those of dpm.py:36-58, every stored like r = 1 (top-k-rec_amd/als.py).  Y fp32 [n, k] is the table that is
 * held fixed in a half-step, X fp32 [n_x, k] the one that is solved for; 1 <= k <= TKR_ALS_MAX_K (wider: TKR_E_UNSUPPORTED).
 *
 *   tkr_als_gram        G fp32 [k, k]: G[p, q] = fp32(scale * sum_t Y[rows[t], p] * Y[rows[t], q] + (p == q ? ridge : 0)), t < n_listed;
 *                       rows int32 [n_listed], or NULL: all n rows (n_listed is then not looked at).  n_listed = 0 gives ridge * I.  A
 *                       workgroup sums a slab of TKR_ALS_GRAM_SLAB listed rows on the exact-fp32 MFMA (v_mfma_f32_32x32x2_f32 over
 *                       tiles of 32 rows staged in LDS: per element one fp32 fma chain in list order from +0.0) into an fp32 partial in
 *                       the workspace; a second launch adds the partials in ascending slab order in fp64, applies scale and ridge and
 *                       rounds once.  workspace: at least tkr_als_workspace_bytes(0, k, ceil(n_listed / TKR_ALS_GRAM_SLAB)) bytes.
 *                       status: -1, or 4 * t + 1 for the smallest t whose rows[t] lies outside [0, n): that row is skipped.
 *   tkr_als_solve_rows  like_ptr int64 [n_x + 1] from 0, like_cols int32 [n_likes]: row r's likes, rows of Y, in any order; a column
 *                       named twice counts twice.  For every r with m_r > 0 likes, y running over them:
 *                         A = G + w_like * sum y y^T,  rhs = w_rhs * sum y,  X[r] = (A + ridge I)^-1 rhs
 *                         row_loss[r] = 1/2 x^T A x - w_rhs * sum y.x + 1/2 w_rhs m_r        (float64 [n_x], or NULL; the new x, A
 *                                       without ridge; fp32 products added in fp64)
 *                       Rows with m_r = 0: X[r] untouched, row_loss[r] = 0.  One workgroup per row: sum y y^T as in tkr_als_gram, A =
 *                       fp32(G + w_like * sum) in LDS, Cholesky in fp32 with the lower triangle in the workgroup's registers and one
 *                       barrier per column (the right-hand side rides along as row k), the back substitution in one wave, one store
 *                       of the row.  A row with m_r >= heavy_from likes (>= 1) does not sum its own
 *                       likes: a launch before the solve sums its slabs of TKR_ALS_GRAM_SLAB likes, one workgroup each, into the
 *                       workspace, and the solve adds them in ascending order in fp64.  workspace: 16-byte aligned;
 *                       tkr_als_workspace_bytes(n_x, k, n_slabs) bytes hold the heavy rows' n_slabs = sum ceil(m_r / TKR_ALS_GRAM_SLAB)
 *                       slabs; a heavy row whose slabs do not fit sums its own likes after all (same result up to the order of the
 *                       sum).  It may be NULL when heavy_from > n_likes, else it holds at least tkr_als_workspace_bytes(n_x, k, 0).
 *                       status: -1, or the smallest 4 * r + kind: kind 1 -- a like column outside [0, n_y) was skipped (m_r counts the
 *                       others; none left: as m_r = 0); 2 -- a pivot of the factorisation is not positive and finite, or the solution is
 *                       not finite: X[r] is left as it is, no NaN is written, row_loss[r] = 0; 3 -- like_ptr does not start at 0,
 *                       descends at this row, leaves [0, n_likes] or gives the row 2^31 likes or more: left as it is, row_loss[r] = 0.
 *   tkr_als_workspace_bytes  the size above (a multiple of 16), or TKR_E_INVAL.
 * The input is not trusted: nothing refused is ever used as an index.  Arguments are checked before any device access and before any
 * launch (TKR_E_INVAL): a null Y / G / X / like_ptr / status, a null like_cols with n_likes > 0, a misaligned status / row_loss /
 * workspace, k / n / n_y / n_x < 1, n_x >= 2^31, n_listed / n_likes < 0, heavy_from < 1, ridge < 0 (solve), a weight that is not finite,
 * a workspace too small.  Deterministic: two calls give the same bits; no float atomics, the only atomic is the status word's minimum.
 *
 * K21 (CER, the reference's single/cer.py:49-63): the same half-step with a prior on every row, and EVERY row solved.
 *   tkr_als_solve_rows_prior  the arguments of tkr_als_solve_rows, and prior fp32 [n_x, k], w_prior >= 0; p = prior[r].
 *                       Rows with likes (m_r > 0 of them inside [0, n_y)):  A = G + w_like * sum y y^T as above,
 *                         rhs = fp32(w_rhs * sum y + w_prior * p)   (both terms in fp64, rounded once),  X[r] = (A + ridge I)^-1 rhs
 *                         row_loss[r] = tkr_als_solve_rows' expression + 1/2 w_prior * sum_j (x_j - p_j)^2   (differences and sum in fp64)
 *                       With w_prior = 0 and a prior of zeros such a row has the bits of tkr_als_solve_rows, X and row_loss, on the own-sum
 *                       and on the heavy path: the prior is one more term of the right-hand side and of the loss and nothing else.
 *                       Rows without likes (like_ptr[r] == like_ptr[r + 1]):  X[r] = (G + ridge I)^-1 fp32(w_prior * p),
 *                         row_loss[r] = 1/2 w_prior * sum_j (x_j - p_j)^2 only (cer.py:61-63 adds no quadratic term for them).
 *                       They all have ONE matrix: fp32(G + ridge I) is factorised once per call, by one workgroup with the Cholesky of
 *                       the per-row kernel, into the workspace; a second launch substitutes forwards and backwards, a lane per row, 256
 *                       rows per workgroup, the factor in LDS and read wave-uniformly, the row's z and x in registers.  The bits of such a
 *                       row depend on G, ridge, w_prior and its own prior only: not on n_x, on which other rows are cold or on its lane.
 *                       A row whose likes were ALL refused (kind 1) is reported, left as it is, row_loss 0: it is not a cold row.
 *                       status as above; kind 2 on the shared factor refuses every cold row (4 * (the smallest cold row) + 2, none of
 *                       them touched); kind 2 on one row's own solution (a prior holding inf or NaN) refuses that row only.  No NaN is
 *                       ever written to X.  workspace: never NULL, 16-byte aligned, tkr_als_prior_workspace_bytes(n_x, k, n_slabs) =
 *                       tkr_als_workspace_bytes(n_x, k, n_slabs) + room for the factor (k * k + 4 floats, rounded up to 16 bytes).
 *                       TKR_E_INVAL before any device access: prior NULL (the caller wants tkr_als_solve_rows) or not 4-byte aligned,
 *                       w_prior negative or not finite, and everything tkr_als_solve_rows refuses. */
#define TKR_ALS_MAX_K 128
#define TKR_ALS_GRAM_SLAB 1024
int64_t tkr_als_workspace_bytes(int64_t n_x, int32_t k, int64_t n_slabs);
int tkr_als_gram(const float* Y, int32_t n, int32_t k, const int32_t* rows, int64_t n_listed, double scale, double ridge, float* G,
                 void* workspace, int64_t workspace_bytes, int64_t* status, void* stream);
int tkr_als_solve_rows(const float* Y, int32_t n_y, int32_t k, const float* G, const int64_t* like_ptr, const int32_t* like_cols,
                       int64_t n_likes, int64_t n_x, double w_like, double w_rhs, double ridge, int64_t heavy_from, float* X,
                       double* row_loss, void* workspace, int64_t workspace_bytes, int64_t* status, void* stream);
int64_t tkr_als_prior_workspace_bytes(int64_t n_x, int32_t k, int64_t n_slabs);
int tkr_als_solve_rows_prior(const float* Y, int32_t n_y, int32_t k, const float* G, const int64_t* like_ptr, const int32_t* like_cols,
                             int64_t n_likes, int64_t n_x, double w_like, double w_rhs, double ridge, int64_t heavy_from, float* X,
                             double* row_loss, const float* prior, double w_prior, void* workspace, int64_t workspace_bytes, int64_t* status,
                             void* stream);

/* ---- K24: the ALS half-step by conjugate gradients (csrc/als_cg.hip), and the Gram at any width up to 512 (csrc/als.hip) -----------------
 * A second, opt-in solver beside K20 / K21; 1 <= k <= TKR_ALS_CG_MAX_K (wider: TKR_E_UNSUPPORTED).  The
 * notation is tkr_als_solve_rows' and tkr_als_solve_rows_prior's.
 *
 *   tkr_als_cg_rows     For row r with likes y in L_r (m_r of them inside [0, n_y)) and, where prior != NULL, p_r = prior[r]:
 *                         A_r v = G v + w_like * sum_y (y . v) y + ridge * v                  (never stored as a matrix)
 *                         b_r   = fp32(w_rhs * sum_y y + w_prior * p_r)                       (both terms in fp64, rounded once)
 *                         x <- X[r];  r <- b - A x;  p <- r;  rho <- r . r
 *                         `steps` times, unless rho < 1e-20 (the row is done):
 *                           q <- A p;  alpha <- rho / (p . q);  x <- fma(alpha, p, x);  r <- fma(-alpha, q, r);  rho' <- r . r;
 *                           p <- fma(rho' / rho, p, r);  rho <- rho'
 *                         X[r] <- x                                                           (steps = 0 stores nothing)
 *                         row_loss[r] = 1/2 x . q' - w_rhs * sum_y (y . x) + 1/2 w_rhs m_r (+ 1/2 w_prior sum_j (x_j - p_j)^2),
 *                                       q' = fp32(G x + w_like * sum_y (y . x) y) from ONE fresh product with the final x; fp64 sums;
 *                                       only when row_loss != NULL
 *                       A v is fp32(G v + w_like * s + ridge * v) with the three terms in fp64; G v is one fp32 fma chain over the
 *                       columns in ascending order from +0.0 (the exact-fp32 MFMA), s = sum_y t_y y one fma chain per component over the
 *                       likes in stored order, t_y = y . v.  Every dot product is one fixed tree: lane l of 64 chains its elements l,
 *                       l + 64, .. by fma from +0.0, then s += s(lane ^ 32), ^ 16, .. ^ 1.  Divisions are IEEE fp32 divisions.
 *                       prior == NULL: rows with m_r = 0 are left untouched, row_loss 0.  prior != NULL: EVERY row is solved; a row
 *                       without likes is the same recurrence with an empty list and its loss is the prior term alone; a row whose likes
 *                       were ALL refused is reported, left as it is, row_loss 0.
 *                       status: -1, or the smallest 4 * r + kind: 1 -- a like column outside [0, n_y) was skipped; 2 -- p . q is not
 *                       positive and finite, or x is not finite: X[r] is left as it came in, row_loss[r] = 0, no NaN is written; 3 --
 *                       like_ptr is broken at this row (as tkr_als_solve_rows): left as it is, row_loss[r] = 0.
 *                       The bits of row r depend on G, the weights, its likes in stored order, its X[r] and prior, and steps: not on
 *                       n_x or on the other rows of the call.  workspace: not used (tkr_als_cg_workspace_bytes gives 0; NULL is fine).
 *                       TKR_E_INVAL before any device access: a null or misaligned pointer, n_y / n_x < 1, n_x >= 2^31, n_likes < 0,
 *                       steps < 0, ridge < 0, w_prior < 0, a weight that is not finite.
 *   tkr_als_gram_wide   tkr_als_gram's definition, arguments, status word and skipped-row rule for 1 <= k <= TKR_ALS_CG_MAX_K: slabs of
 *                       TKR_ALS_GRAM_SLAB rows, fp32 partials on the exact MFMA, added in ascending slab order in fp64, rounded once.
 *                       For k <= TKR_ALS_MAX_K its output has tkr_als_gram's bits.  workspace: at least
 *                       tkr_als_gram_wide_workspace_bytes(k, ceil(n_listed / TKR_ALS_GRAM_SLAB)) bytes (k * k floats per slab). */
#define TKR_ALS_CG_MAX_K 512
int64_t tkr_als_cg_workspace_bytes(int64_t n_x, int32_t k);
int tkr_als_cg_rows(const float* Y, int32_t n_y, int32_t k, const float* G, const int64_t* like_ptr, const int32_t* like_cols,
                    int64_t n_likes, int64_t n_x, double w_like, double w_rhs, double ridge, int32_t steps, float* X, double* row_loss,
                    const float* prior, double w_prior, void* workspace, int64_t workspace_bytes, int64_t* status, void* stream);
int64_t tkr_als_gram_wide_workspace_bytes(int32_t k, int64_t n_slabs);
int tkr_als_gram_wide(const float* Y, int32_t n, int32_t k, const int32_t* rows, int64_t n_listed, double scale, double ridge, float* G,
                      void* workspace, int64_t workspace_bytes, int64_t* status, void* stream);

/* ---- K22: a dense MLP content encoder, applied and trained (csrc/mlp.hip) ----------------------------------------------------------------
 * Replaces the TensorFlow graph of the reference's single/mlp.py:14-40 (tf.layers.dense, RMSPropOptimizer.minimize, the sess.run of out
 * and fit), the encoder of single/dpm.py (top-k-rec_amd/als.py MLP and DPM).
 *
 *   tkr_mlp_net         n_layers dense layers, 1 <= n_layers <= TKR_MLP_MAX_LAYERS; width[0] = d .. width[n_layers] = k, every width >= 1
 *                       (no tile-multiple requirement; above 2^21: TKR_E_UNSUPPORTED).  Layer l: W[l] fp32 [width[l], width[l + 1]] row-major
 *                       (the layout of a TF dense kernel), bias[l] [width[l + 1]], msW[l] and msb[l] the RMSProp slots of the same shapes
 *                       (tkr_mlp_forward does not look at the slots: they may be NULL there).  Every layer but the last has the sigmoid
 *                       s = 1 / (1 + expf(-x)), the last is linear.
 *   tkr_mlp_forward     out fp32 [m, k] = the network applied to X[rows[t]], t < m; X fp32 [n, d]; rows int32 [m], or NULL: the rows
 *                       0 .. m - 1 (m <= n).  Per layer two launches: the products on the exact-fp32 MFMA (v_mfma_f32_32x32x2_f32: per
 *                       element one fp32 fma chain in input order from +0.0), the contraction cut into slabs of TKR_MLP_SLAB inputs, one
 *                       workgroup per 64 x 64 tile of the output and slab, each slab's sum an fp32 partial in the workspace; then the
 *                       partials are added in ascending slab order in fp64 and rounded once, the bias is added in fp32 and the activation
 *                       applied.  Rows are taken TKR_MLP_FORWARD_CHUNK at a time; a row's bits do not depend on m or on its place.
 *   tkr_mlp_fit         one epoch of mlp.py:32-40: batch t takes the rows order[t * batch .. min((t + 1) * batch, m)) of X [n, d] and
 *                       Y fp32 [n, k] (the last batch may be short), 1 <= batch <= TKR_MLP_MAX_BATCH.  Per batch, every gradient from the
 *                       parameters as they were before the batch (as TF computes them):
 *                         forward through every layer as above, the activations kept;
 *                         batch_loss[t] (float64) = 1/2 sum (y - F)^2, differences and sum in fp64;
 *                         delta_L = F - Y, delta_{l-1} = (delta_l W_l^T) * (h (1 - h)) (the product slabbed over the layer's outputs, as
 *                         above); no delta for the input;
 *                         per layer ONE launch: a workgroup owns a 64 x 64 tile of W_l, forms g[i, j] = sum_b A[b, i] delta[b, j] on the
 *                         MFMA (one fma chain per element in batch order from +0.0; A = the layer's input) and applies dense RMSProp in
 *                         registers -- rho = 0.9, eps = 1e-10 inside the root, momentum 0, every operation rounded on its own in fp32:
 *                           q = g * g;  ms' = ms + (q - ms) * fl(1 - rho);  w' = w - (lr * g) / sqrt(ms' + eps)
 *                         -- W and its slot are read once and stored once, the gradient never exists in memory.  The bias gradient is
 *                         the same chain with A = 1.
 *                       Everything is enqueued on `stream`; nothing synchronises.  lr is rounded to fp32 by the caller.
 *   tkr_mlp_workspace_bytes   what both need for a net of this shape (only n_layers and width are looked at): m rows forwarded, batches
 *                       of `batch` fitted (batch = 0: forward only); a multiple of 16, or TKR_E_INVAL.
 * The input is not trusted: a pre-pass checks rows / order.  status: -1, or 4 * t + 1 for the smallest t whose index lies outside [0, n);
 * then NO parameter, slot, output or batch_loss is written by the call (every kernel reads the status word first).  m = 0 writes status -1
 * and nothing else.  Arguments are checked before any device access and before any launch (TKR_E_INVAL): a null net / X / Y / out / status
 * (order, batch_loss, workspace: with m > 0), a pointer off its alignment (floats 4, status and batch_loss 8, workspace 16), n_layers or a
 * width out of range, a null parameter (fit: or slot), n < 1, m < 0, rows NULL with m > n, batch < 1, lr negative or not finite, a workspace
 * too small; batch > TKR_MLP_MAX_BATCH: TKR_E_UNSUPPORTED.  Deterministic: two calls give the same bits; no float atomics. */
#define TKR_MLP_MAX_LAYERS 5
#define TKR_MLP_MAX_BATCH 256
#define TKR_MLP_SLAB 512          /* inputs of a layer one workgroup sums */
#define TKR_MLP_FORWARD_CHUNK 256 /* rows tkr_mlp_forward takes at a time */
typedef struct tkr_mlp_net {
    int32_t n_layers;
    int32_t width[TKR_MLP_MAX_LAYERS + 1];
    float* W[TKR_MLP_MAX_LAYERS];
    float* bias[TKR_MLP_MAX_LAYERS];
    float* msW[TKR_MLP_MAX_LAYERS];
    float* msb[TKR_MLP_MAX_LAYERS];
} tkr_mlp_net;
int64_t tkr_mlp_workspace_bytes(const tkr_mlp_net* net, int64_t m, int32_t batch);
int tkr_mlp_forward(const tkr_mlp_net* net, const float* X, int32_t n, const int32_t* rows, int64_t m, float* out, void* workspace,
                    int64_t workspace_bytes, int64_t* status, void* stream);
int tkr_mlp_fit(const tkr_mlp_net* net, const float* X, int32_t n, const float* Y, const int32_t* order, int64_t m, int32_t batch, float lr,
                double* batch_loss, void* workspace, int64_t workspace_bytes, int64_t* status, void* stream);

/* ---- K25: the two halves of a logistic-matrix-factorisation half-step (csrc/lmf.hip) ------------------------------------------------------
 * Logistic MF (Johnson 2014; top-k-rec_amd/lmf.py): p(like) = sigma(x_u . y_i + beta_u + beta_i), the objective
 * summed over EVERY (user, item) pair.  Tables are augmented to K = k + 2 columns -- a user row is [x, beta_u, 1], an item row
 * [y, 1, beta_i] -- so a score is s_rc = X[r] . Y[c] over all K columns; 1 <= k <= TKR_LMF_MAX_K (wider: TKR_E_UNSUPPORTED).  Y fp32
 * [n_y, K] is the table held fixed in a half-step, X fp32 [n_x, K] the one that moves.  No multiple-of-anything requirement on k.
 *
 *   tkr_lmf_dense_rows  D fp32 [n_x, K]: D[r] = sum over c = 0 .. n_y - 1 of sigma(s_rc) Y[c]; and, where sp != NULL, sp float64 [n_x]:
 *                       sp[r] = sum_c softplus(s_rc).  The score matrix never exists in memory.  A workgroup owns 128 rows of X (32 per
 *                       wave, in registers) and one slab of TKR_LMF_SLAB rows of Y, which it walks in tiles of 32 rows in ascending
 *                       order: S = Xblk Ytile^T on v_mfma_f32_32x32x2_f32 (the contraction over the K columns in column order),
 *                       P = sigma(S) from the accumulators to LDS in the A-operand layout, D += P Ytile on the same MFMA (the contraction
 *                       over the tile's rows in order).  An MFMA result is a k-ordered fmaf chain: a slab's partial of D[r][j] is ONE fp32
 *                       chain from +0.0 over the slab's rows in row order, of terms sigma(s_rc) * Y[c][j], s_rc one fp32 chain from +0.0
 *                       over the columns.  The slabs' partials are added in ascending slab order in fp64 and rounded once.  sp: fp32
 *                       softplus values added in fp64 -- per slab, the rows c = 0..3, 8..11, 16..19, 24..27 mod 32 in ascending order,
 *                       the others in ascending order, the two added; then the slabs in ascending order.
 *                         sigma(s) = 1 / (1 + exp(-s)) with an IEEE division: exactly 1.0f for s >= 40, exactly +0 for s <= -110,
 *                         0.5f at 0; softplus(s) = max(s, 0) + log1p(exp(-|s|)): softplus(1e4) = 1e4.  Both finite at any finite s.
 *                       Bits are the same run to run, and the bits of row r depend on X[r] and Y only: not on n_x or the other rows.
 *                       workspace: 16-byte aligned, tkr_lmf_workspace_bytes(n_x, k, n_y) bytes; may be NULL for n_y <= TKR_LMF_SLAB.
 *                       No status word: nothing in the input is an index.
 *   tkr_lmf_step_rows   like_ptr int64 [n_x + 1] from 0, like_cols int32 [n_likes]: row r's likes, rows of Y, in any order; a column
 *                       named twice counts twice.  D: what tkr_lmf_dense_rows gave for this X and Y.  For EVERY row r, in place on X and
 *                       on its AdaGrad slot H fp32 [n_x, K] (a row without likes has a gradient too):
 *                         L = sum over the likes c of (1 - sigma(s_rc)) Y[c]
 *                         g = fp32(alpha * L - D[r] - lam * X[r])         (the three terms in fp64, rounded once)
 *                         h' = fma(g, g, h);  x' = x + (lr * g) / sqrt(h')  (fp32, every operation rounded on its own)
 *                         column `fixed` (0 <= fixed < K) is left out: X[r][fixed] and H[r][fixed] keep their bits
 *                         row_loss[r] = alpha * sum_likes softplus(s_rc) - alpha * sum_likes s_rc + 1/2 lam * sum_{j != fixed} X[r][j]^2
 *                                       (float64 [n_x], or NULL; at the X the call found; fp32 values added in fp64)
 *                       One wave per row, the row, its slot and g in registers, whole rows of Y gathered.  s_rc is one fixed tree: lane l
 *                       of 64 chains the columns l, l + 64, l + 128 by fma from +0.0, then the tree of the wave's sum.  L is one fp32
 *                       chain per column from +0.0 over the likes in stored order.  A row with MORE than heavy_from likes (>= 1) is
 *                       summed by one workgroup of TKR_LMF_HEAVY_WAVES waves in a second launch: its likes are cut into slabs of
 *                       TKR_LMF_LIKE_SLAB, slab j is such a chain, summed by wave j mod TKR_LMF_HEAVY_WAVES; a wave adds its slabs in
 *                       ascending order in fp64, the waves are added in ascending order in fp64, L is rounded once (the loss sums alike).
 *                       status: -1, or the smallest 4 * r + kind: 1 -- a like column outside [0, n_y) was skipped; 3 -- like_ptr does
 *                       not start at 0, descends at this row, leaves [0, n_likes] or gives the row 2^31 likes or more: X[r] and H[r] are
 *                       left as they are, row_loss[r] = 0.  workspace: 16-byte aligned, tkr_lmf_workspace_bytes(n_x, k, n_y) bytes; may
 *                       be NULL when heavy_from >= n_likes.
 *   tkr_lmf_workspace_bytes  what either call needs at most (a multiple of 16), TKR_E_INVAL or TKR_E_UNSUPPORTED.
 * The input is not trusted: nothing refused is ever used as an index.  Arguments are checked before any device access and before any
 * launch (TKR_E_INVAL): a null or misaligned pointer (floats 4, like_ptr / sp / row_loss / status 8, workspace 16), a null like_cols with
 * n_likes > 0, n_x / n_y < 1, n_x >= 2^31, n_likes < 0, heavy_from < 1, fixed outside [0, K), lam < 0, a weight that is not finite, a
 * workspace too small.  n_y above 65535 slabs: TKR_E_UNSUPPORTED.  No float atomics: the atomics are the status word's minimum and the
 * integer counter of the list of heavy rows, whose order changes no result. */
#define TKR_LMF_MAX_K 128
#define TKR_LMF_SLAB 4096        /* rows of Y one workgroup of tkr_lmf_dense_rows walks */
#define TKR_LMF_LIKE_SLAB 256    /* likes of a heavy row one wave sums as one chain */
#define TKR_LMF_HEAVY_WAVES 16
int64_t tkr_lmf_workspace_bytes(int64_t n_x, int32_t k, int64_t n_y);
int tkr_lmf_dense_rows(const float* X, int64_t n_x, const float* Y, int64_t n_y, int32_t k, float* D, double* sp, void* workspace,
                       int64_t workspace_bytes, void* stream);
int tkr_lmf_step_rows(const float* Y, int32_t n_y, int32_t k, const float* D, const int64_t* like_ptr, const int32_t* like_cols, int64_t n_likes,
                      int64_t n_x, int32_t fixed, double alpha, double lam, double lr, int64_t heavy_from, float* X, float* H, double* row_loss,
                      void* workspace, int64_t workspace_bytes, int64_t* status, void* stream);

/* ---- K26: a sparse x dense product, and CER's E-step by conjugate gradients on it (csrc/sparse.hip) ------------------------------------------
 * The opt-in estep='cg' of top-k-rec_amd/als.py: the content features stay a CSR on the device, nothing of size
 * d x d or n_items x d is formed.  1 <= k <= TKR_ALS_CG_MAX_K (wider: TKR_E_UNSUPPORTED).
 *
 *   tkr_csr_spmm        A: a CSR of n_rows x n_cols, ptr int64 [n_rows + 1] from 0, col int32 [nnz], val fp32 [nnz]; X fp32 [n_cols, k];
 *                       Z fp32 [n_rows, k] or NULL; out fp32 [n_rows, k], overlapping neither X nor Z.
 *                         out[r][c] = fp32(alpha * s + beta * Z[r][c]),  s = sum over the row's nonzeros e of val[e] * X[col[e]][c]
 *                       (without Z: fp32(alpha * s)); the products and the sum in float64, rounded ONCE.  A row of at most heavy_from
 *                       nonzeros (>= 1): s is ONE fp32 chain per component, s = fma(val[e], X[col[e]][c], s) over its nonzeros in stored
 *                       order from +0.0.  A longer row goes to one workgroup in a second launch: it is cut into slabs of TKR_SPMM_SLAB
 *                       nonzeros in stored order, each slab is that chain, and s is the slab sums added in ascending slab order in
 *                       float64.  A row's bits depend on its own nonzeros, the rows of X they name, Z[r], alpha, beta and heavy_from:
 *                       not on n_rows, on the other rows or on the run.  A row is owned by 8, 16, 32 or 64 lanes (k <= 8, 16, 32, more),
 *                       so narrow tables put several rows on a wave; the rows of X are gathered 16 at a time (8 at k <= 8 and above
 *                       k = 128, 4 above k = 256) ahead of
 *                       the chain, which takes them one by one.  A column named twice counts twice.
 *                       status: -1, or the smallest 4 * r + kind: 0 -- row r holds a column outside [0, n_cols) (never used as an index);
 *                       1 -- it holds a value that is not finite; 3 -- ptr does not start at 0, descends at row r, leaves [0, nnz] or
 *                       gives the row 2^31 nonzeros or more.  A refused row of out is NOT written; the other rows are.
 *                       workspace: 16-byte aligned, tkr_csr_spmm_workspace_bytes(n_rows) bytes; may be NULL when heavy_from >= nnz.
 *   tkr_estep_cg        F: the CSR (f_ptr, f_col, f_val) of n_items x d; its transpose (t_ptr, t_col, t_val) of d x n_items, the same nnz;
 *                       both canonical (ascending columns, no duplicates -- not checked: the result is what the stored order gives).
 *                       V fp32 [n_items, k]; E fp32 [d, k], in and out.  `steps` (>= 1) steps of conjugate gradients on
 *                       (lv F^T F + le I) E = lv F^T V from the E given, lv, le > 0, the k columns side by side:
 *                         B = lv F^T V;  R = B - (lv F^T (F E) + le E);  P = R;  rho_c = R_c . R_c
 *                         `steps` times, in the columns with rho_c >= 1e-20:  T = F P;  Q = lv F^T T + le P;  alpha_c = rho_c / (P_c . Q_c);
 *                           E_c = fma(alpha_c, P_c, E_c);  R_c = fma(-alpha_c, Q_c, R_c);  rho'_c = R_c . R_c;
 *                           P_c = fma(rho'_c / rho_c, P_c, R_c);  rho_c = rho'_c
 *                       Every product is tkr_csr_spmm (lv F^T T + le P is one: alpha = lv, beta = le, Z = P); R = B - W is an fp32
 *                       subtraction; the divisions are IEEE fp32.  A dot product of column c is ONE tree: the d rows are cut into slabs
 *                       of TKR_ESTEP_SLAB rows, a slab into 16 runs of 64 rows; a run is an fma chain from +0.0 over its rows in ascending
 *                       order, the 16 run sums are added in ascending order in fp32 (a run past d is +0.0), and the slabs' partials are
 *                       added in ascending slab order in float64 and rounded once.  alpha, beta and rho stay on the device.
 *                       status: -1, or the smallest 4 * where + kind.  Of the input: kinds 0, 1, 3 of tkr_csr_spmm with where = the row
 *                       of F, or n_items + the row of F^T; kind 1 also for row `where` of V holding a value that is not finite.  Any of
 *                       these: E is left as it came in, all of it.  Of the recurrence: 4 * c + 2 -- P_c . Q_c is not positive and
 *                       finite at some step: column c of E is left as it came in, the other columns are solved.
 *                       workspace: 16-byte aligned, tkr_estep_cg_workspace_bytes(n_items, d, k) bytes: T, five tables of E's shape
 *                       (B, R, P, Q and the E being built), two [slabs, k] tables of partials, the list of heavy rows.
 * The input is not trusted: nothing refused is ever used as an index.  Arguments are checked before any device access and before any
 * launch (TKR_E_INVAL): a null or misaligned pointer (floats and col 4, ptr / status 8, workspace 16), a null col or val with nnz > 0,
 * n_rows / n_cols / n_items / d < 1 or >= 2^31, nnz < 0, heavy_from < 1, steps < 1, lv or le not positive and finite, alpha or beta
 * not finite, a workspace too small.  tkr_estep_cg and its size call: n_items * k or d * k above (2^31 - 1) * 256 - 255 elements (a table
 * of 2 TB: the one-thread-per-element launches would leave the grid) is TKR_E_UNSUPPORTED.  No float atomics: the atomics are the
 * status word's minimum and the integer counter of the list of heavy rows, whose order changes no result. */
#define TKR_SPMM_SLAB 256        /* nonzeros of a heavy row one group of lanes sums as one chain */
#define TKR_SPMM_HEAVY_FROM 2048 /* what the bindings pass for heavy_from by default */
#define TKR_ESTEP_SLAB 1024      /* rows of E whose part of a dot product is one fp32 partial */
int64_t tkr_csr_spmm_workspace_bytes(int64_t n_rows);
int tkr_csr_spmm(const int64_t* ptr, const int32_t* col, const float* val, int64_t nnz, int64_t n_rows, int32_t n_cols, const float* X, int32_t k,
                 double alpha, const float* Z, double beta, float* out, int64_t heavy_from, void* workspace, int64_t workspace_bytes,
                 int64_t* status, void* stream);
int64_t tkr_estep_cg_workspace_bytes(int64_t n_items, int64_t d, int32_t k);
int tkr_estep_cg(const int64_t* f_ptr, const int32_t* f_col, const float* f_val, const int64_t* t_ptr, const int32_t* t_col, const float* t_val,
                 int64_t nnz, int64_t n_items, int64_t d, const float* V, int32_t k, float* E, double lv, double le, int32_t steps,
                 int64_t heavy_from, void* workspace, int64_t workspace_bytes, int64_t* status, void* stream);

/* ---- K27: the three parts of a softmax-matrix-factorisation half-step (csrc/smf.hip) --------------------------------------------------------
 * Softmax MF (the multinomial likelihood of Mult-DAE / Mult-VAE; top-k-rec_amd/smf.py): p(i | u) =
 * softmax_i(x_u . y_i + beta_i) over the WHOLE catalogue.  Tables are augmented to K = k + 1 columns -- a user row is [x, 1], an item row
 * [y, beta_i] -- so a score is s_rc = X[r] . Y[c] over all K columns, one fp32 chain from +0.0 in column order;
 * 1 <= k <= TKR_SMF_MAX_K (wider: TKR_E_UNSUPPORTED).  Y fp32 [n_y, K] is the table held fixed in a half-step, X fp32 [n_x, K] the one
 * that moves.  No multiple-of-anything requirement on k.
 *
 *   tkr_smf_lse_rows    lse fp32 [n_x]: lse[r] = log sum over c = 0 .. n_y - 1 of exp(s_rc); finite at any finite scores (|s| = 1e4
 *                       included).  K25's shape: a workgroup owns 128 rows of X (32 per wave, in registers) and one slab of TKR_SMF_SLAB
 *                       rows of Y, walked in tiles of 32 rows in ascending order, S from v_mfma_f32_32x32x2_f32.  Per (row, slab) a pair
 *                       (m, l = sum exp(s - m)): the rows c mod 8 < 4 of every tile and the others are followed apart, each by a running
 *                       maximum -- a tile that raises it scales l by exp(m - m') first, then adds its scores' terms in ascending row
 *                       order -- and joined at the slab's end: M = max(m0, m1), l = l0 exp(m0 - M) + l1 exp(m1 - M), all in fp32.  The
 *                       slabs are joined in ascending order in fp64: M = max m, sum l exp(m - M), lse = fp32(M + log sum).
 *                       workspace: 16-byte aligned, tkr_smf_workspace_bytes(n_x, k, n_y) bytes; may be NULL for n_y <= TKR_SMF_SLAB.
 *   tkr_smf_dense_rows  row_off fp32 [n_x] or NULL, col_off fp32 [n_y] or NULL (a NULL offset is 0).  D fp32 [n_x, K]:
 *                         D[r] = sum over c = 0 .. n_y - 1 of P_rc Y[c],   P_rc = exp(fl(fl(s_rc - row_off[r]) - col_off[c]))
 *                       K25's dense kernel with this P in place of sigma: P goes from the accumulators into LDS in the A-operand layout,
 *                       D += P Ytile runs on the same MFMA; a slab's partial of D[r][j] is ONE fp32 chain from +0.0 over the slab's rows
 *                       in row order; the slabs are added in ascending order in fp64 and rounded once.  exp(+0.0) is exactly 1.0f,
 *                       exp(-inf) exactly +0: an offset of +inf is legal and gives P = +0, whatever finite values that row of Y holds.
 *                       s_rc has the bits tkr_smf_lse_rows formed for the same X and Y.  No status word: nothing here is an index.
 *                       workspace: as above.
 *   tkr_smf_step_rows   like_ptr, like_cols, heavy_from, the status word, the refusals (kinds 1 and 3) and the heavy rows are
 *                       tkr_lmf_step_rows's: the same code (csrc/lmf_rows.h).  For EVERY row r, in place on X and its AdaGrad slot H:
 *                         L = sum over the likes c of Y[c]                 (one fp32 chain per column from +0.0 in stored order)
 *                         g = fp32(L - w * D[r] - lam * X[r])              (the three terms in fp64, rounded once;
 *                                                                           w: the likes row r stores where scale_by_likes = 1, else 1)
 *                         h' = fma(g, g, h);  x' = x + (lr * g) / sqrt(h')  (fp32, every operation rounded on its own)
 *                         column `fixed` (-1 <= fixed < K; -1: none) is left out: X[r][fixed] and H[r][fixed] keep their bits
 *                         row_loss[r] = -sum_likes s_rc + 1/2 lam * sum_{j != fixed} X[r][j]^2
 *                                       (float64 [n_x], or NULL; at the X the call found; fp32 values added in fp64)
 *                       A refused row (kind 3) keeps X and H, and its row_loss is 0.
 *   tkr_smf_workspace_bytes  what any of the three calls needs at most (a multiple of 16), TKR_E_INVAL or TKR_E_UNSUPPORTED.
 * A user half-step is lse, dense with row_off = lse, step with fixed = k and scale_by_likes = 1; an item half-step is dense with
 * col_off[u] = lse_u - log n_u (+inf for a user without likes) and step with fixed = -1 and scale_by_likes = 0.
 * Arguments are checked before any device access and before any launch (TKR_E_INVAL), the same things as K25: a null or misaligned
 * pointer (floats 4, like_ptr / row_loss / status 8, workspace 16), a null like_cols with n_likes > 0, n_x / n_y < 1, n_x >= 2^31,
 * n_likes < 0, heavy_from < 1, fixed outside [-1, K), scale_by_likes not 0 or 1, lam < 0, lam or lr not finite, a workspace too small.
 * n_y above 65535 slabs: TKR_E_UNSUPPORTED.  No float atomics.  Bits are the same run to run, and the bits of row r depend on X[r], Y,
 * the offsets and heavy_from only: not on n_x or on the other rows. */
#define TKR_SMF_MAX_K 128
#define TKR_SMF_SLAB 4096        /* rows of Y one workgroup of tkr_smf_lse_rows / tkr_smf_dense_rows walks */
int64_t tkr_smf_workspace_bytes(int64_t n_x, int32_t k, int64_t n_y);
int tkr_smf_lse_rows(const float* X, int64_t n_x, const float* Y, int64_t n_y, int32_t k, float* lse, void* workspace, int64_t workspace_bytes,
                     void* stream);
int tkr_smf_dense_rows(const float* X, int64_t n_x, const float* Y, int64_t n_y, int32_t k, const float* row_off, const float* col_off, float* D,
                       void* workspace, int64_t workspace_bytes, void* stream);
int tkr_smf_step_rows(const float* Y, int32_t n_y, int32_t k, const float* D, const int64_t* like_ptr, const int32_t* like_cols, int64_t n_likes,
                      int64_t n_x, int32_t fixed, int32_t scale_by_likes, double lam, double lr, int64_t heavy_from, float* X, float* H,
                      double* row_loss, void* workspace, int64_t workspace_bytes, int64_t* status, void* stream);

/* ---- K28 / K29: the item-neighbourhood model, built from the likes and served from histories (csrc/knn.hip) ----------------------------------
 * ItemKNN (top-k-rec_amd/knn.py): no factors, no iteration, no seed.  The n_items x n_items matrix of
 * co-occurrence counts is never in memory.
 *
 *   tkr_knn_build       The training likes as sets, twice: the CSR over users (u_ptr int64 [n_users + 1] from 0, u_cols int32, the columns
 *                       of a row ascending and unique) and its transpose over items (i_ptr int64 [n_items + 1], i_rows int32);
 *                       n_u_entries / n_i_entries: the lengths of u_cols / i_rows (at least u_ptr[n_users] / i_ptr[n_items]).
 *                       norm float64 [n_items], finite and positive; shrink >= 0, finite; 1 <= N <= TKR_KNN_MAX_N.
 *                         c_ij     = the number of users who like both i and j                                   (an exact integer)
 *                         sim(i,j) = fp32( (double)c_ij / ( fl64(norm[i] * norm[j]) + shrink ) )
 *                       in IEEE fp64, the product rounded first, then the sum, ONE division, rounded once to fp32 -- no fma.  Only a
 *                       multiply, an add and a divide run on the device, so NumPy restates every bit.  The candidates of row i are the
 *                       j != i with c_ij > 0.  nbr_ids int32 [n_items, N]: the N best candidates in K4's canonical order (sim
 *                       descending, ties -> the higher column first); nbr_w fp32 [n_items, N]: their sim; a row with fewer than N
 *                       candidates is padded with -1 / +0.0.
 *                       heavy_from (0: TKR_KNN_HEAVY_FROM): a row's work is the sum of n_u over its likers u; a row whose work is above
 *                       heavy_from is cut over its likers into up to 64 workgroups, whose partial counters are added as integers in a
 *                       row of the workspace.  slab_cols (0: TKR_KNN_MAX_SLAB, the most one workgroup's LDS holds): a wider catalogue is
 *                       walked once per slab of that many columns, and the slabs' winners are merged.  The result depends on neither.
 *                       status: -1, or the smallest 4 * where + kind, found by a pre-pass before anything is written -- a refused call
 *                       leaves nbr_ids and nbr_w untouched:
 *                         0  u_ptr (where = the row) or i_ptr (where = n_users + 1 + the row) does not start at 0, decreases or leaves
 *                            [0, its array's length]
 *                         1  u_cols[where] is outside [0, n_items), or i_rows[where - n_u_entries] outside [0, n_users)
 *                         2  u_ptr[n_users] != i_ptr[n_items], both inside their arrays: the two CSRs hold different numbers of entries (where = 0)
 *                         3  norm[where] is not finite and positive
 *                       workspace: 16-byte aligned, tkr_knn_build_workspace_bytes(n_items) bytes.
 *   tkr_knn_score       n_rows lines.  hist_ptr int64 [n_rows + 1] from 0, hist_cols int32 (n_hist of them): the liked catalogue items
 *                       of every line, ascending and unique.  The table of tkr_knn_build: nbr_ids, nbr_w [n_items, N].  col_of_item
 *                       int32 [n_items] or NULL: the scenario column of a catalogue item, or -1; NULL is the identity and needs
 *                       n_cols == n_items.  mask / mask_pitch: K4's (nullable).  For line r and column c, with j the item mapped to c:
 *                         s(r,c) = the fp32 chain acc = fl(acc + nbr_w[i][p]) from +0.0 over the history items i of the line in stored
 *                                  order, item i contributing when nbr_ids[i][p] == j for some p (j is among the N nearest of i)
 *                       A column nobody contributes to scores +0.0; an entry that maps to -1 is dropped.  out_ids [n_rows, K] and
 *                       out_scores (nullable) are tkr_score_topk's with this s: the K best unmasked columns in the canonical order,
 *                       padded -1 / -inf, 1 <= K <= TKR_KNN_MAX_K (out_ids NULL: no lists, K is ignored).  like_ptr int64
 *                       [n_rows + 1], like_cols int32 (n_likes of them), rank_out int32 [n_likes], all three or none: tkr_like_ranks's
 *                       definition with this s (-1 for a masked or out-of-range like; a like at position p of the list has rank p).
 *                       slab_cols as above (the history is walked once per slab; the result does not depend on it).
 *                       status: -1, or the smallest 4 * where + kind of the pre-pass; a refused call writes nothing:
 *                         0  hist_ptr does not start at 0, decreases or leaves [0, n_hist] at row `where`
 *                         1  hist_cols[where] is outside [0, n_items)
 *                         2  like_ptr does not start at 0, decreases or leaves [0, n_likes] at row `where`
 *                       A neighbour id outside [0, n_items) (the -1 padding included) names nothing and is never used as an index, a
 *                       mapped column outside [0, n_cols) neither.  Weights must be finite (knn.py import_model checks); on a table
 *                       that breaks the rule nothing is indexed out of range and nothing more is promised.
 * One workgroup owns a line from the first add to the last rank, and its first wave alone walks the history, so a column's chain is in
 * history order; no atomics but LDS histogram counters whose order changes no result: two runs
 * give the same bits, and a block of lines ranked alone gives what it gives inside a larger call.  Arguments are checked before any launch
 * (TKR_E_INVAL): a null or misaligned pointer, a negative length, n_users / n_items / n_rows / n_cols < 1 or >= 2^31, shrink negative or
 * not finite, heavy_from or slab_cols < 0, a workspace too small, mask_pitch < n_rows, likes given in part.  N, K or slab_cols above their
 * limits: TKR_E_UNSUPPORTED. */
#define TKR_KNN_MAX_N 512        /* neighbours kept per item */
#define TKR_KNN_MAX_K 32         /* columns one launch of tkr_knn_score lists per line */
#define TKR_KNN_MAX_SLAB 36864   /* columns whose counters (K28) or accumulators (K29) one workgroup keeps in LDS */
#define TKR_KNN_HEAVY_FROM 262144 /* what heavy_from = 0 means */
int64_t tkr_knn_build_workspace_bytes(int64_t n_items);
int tkr_knn_build(const int64_t* u_ptr, const int32_t* u_cols, int64_t n_u_entries, const int64_t* i_ptr, const int32_t* i_rows,
                  int64_t n_i_entries, int64_t n_users, int64_t n_items, const double* norm, double shrink, int32_t N, int64_t heavy_from,
                  int32_t slab_cols, int32_t* nbr_ids, float* nbr_w, void* workspace, int64_t workspace_bytes, int64_t* status, void* stream);
int tkr_knn_score(const int64_t* hist_ptr, const int32_t* hist_cols, int64_t n_hist, int64_t n_rows, const int32_t* nbr_ids,
                  const float* nbr_w, int32_t n_items, int32_t N, const int32_t* col_of_item, int32_t n_cols, const uint32_t* mask,
                  int32_t mask_pitch, int32_t K, int32_t* out_ids, float* out_scores, const int64_t* like_ptr, const int32_t* like_cols,
                  int64_t n_likes, int32_t* rank_out, int32_t slab_cols, int64_t* status, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* TKR_H */
