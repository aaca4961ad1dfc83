"""ctypes binding of libtkr_hip.so (C ABI in include/tkr.h).

PyTorch is plumbing here: it owns device memory and the stream; every compute call goes
through the C ABI with raw device pointers.  There is NO fallback: if the library is
missing or a call fails, this module raises.
"""
from __future__ import annotations

import ctypes as C
import warnings
import os

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get('TKR_HIP_LIB') or os.path.join(_HERE, 'libtkr_hip.so')      # the override is for A/B builds of the kernels (scripts/)

_lib = None
VERSION = 120          # TKR_VERSION of include/tkr.h this binding was written against


class TkrError(RuntimeError):
    pass


class StepGaveUp(TkrError):
    """a bounded spin of a persistent step kernel ran out: the tables of the run are invalid, the engine has stepped down to the
    next kernel (K2o -> K2f -> K2) and works again once valid tables are put back (BPR.train does)"""


class BprState(C.Structure):
    """mirror of tkr_bpr_state (include/tkr.h)"""
    _fields_ = [('U', C.c_void_p), ('msU', C.c_void_p),
                ('V', C.c_void_p), ('msV', C.c_void_p), ('b', C.c_void_p), ('msb', C.c_void_p),
                ('n_users', C.c_int32), ('n_items', C.c_int32), ('k', C.c_int32), ('mode', C.c_int32),
                ('lu', C.c_float), ('li', C.c_float), ('lj', C.c_float), ('lb', C.c_float),
                ('lr', C.c_float), ('rho', C.c_float), ('eps', C.c_float), ('opt', C.c_int32)]


class PlanCall(C.Structure):
    """tkr_plan_call of include/tkr.h: the arguments of tkr_sample_plan_owned"""
    _fields_ = [(n, C.c_void_p) for n in ('tr_users', 'row_ptr', 'pos_cols', 'cols_sorted', 'ucnt', 'icnt', 'touch_u', 'touch_i', 'out_u', 'out_i',
                                           'out_j', 'task', 'occ', 'occt', 'prec', 'pocc', 'ohdr')] + \
               [('seed', C.c_uint64), ('first_triplet', C.c_uint64)] + \
               [(n, C.c_int32) for n in ('n_tr', 'n_users', 'n_items', 'n_batches', 'batch_size', 'n_owner', 'ohdr_stride', 'reserved')]


def plan_call(csr, n_users, n_items, seed, B, cnt, plan):
    """-> PlanCall for K1 into `plan` (an owner-ordered dataflow plan buffer); first_triplet / n_batches are the caller's to set"""
    assert plan.owners > 0
    for t in (csr.tr_users, csr.row_ptr, csr.pos_cols, csr.cols_sorted, cnt.ucnt, cnt.icnt, cnt.touch_u, cnt.touch_i, plan.u, plan.task):
        assert t.is_cuda and t.is_contiguous()
    assert cnt.ucnt.numel() == n_users and cnt.icnt.numel() == n_items
    pc = PlanCall()
    for name, t in (('tr_users', csr.tr_users), ('row_ptr', csr.row_ptr), ('pos_cols', csr.pos_cols), ('cols_sorted', csr.cols_sorted),
                    ('ucnt', cnt.ucnt), ('icnt', cnt.icnt), ('touch_u', cnt.touch_u), ('touch_i', cnt.touch_i), ('out_u', plan.u),
                    ('out_i', plan.i), ('out_j', plan.j), ('task', plan.task), ('occ', plan.occ), ('occt', plan.occt), ('prec', plan.prec),
                    ('pocc', plan.pocc), ('ohdr', plan.ohdr)):
        setattr(pc, name, t.data_ptr())
    pc.seed, pc.n_tr, pc.n_users, pc.n_items, pc.batch_size = seed, int(csr.tr_users.numel()), n_users, n_items, B
    pc.n_owner, pc.ohdr_stride = plan.owners, plan.cap
    pc.keep = (csr, cnt)                  # the tensors behind the pointers live as long as the struct
    return pc


class FlowState(C.Structure):
    """mirror of tkr_flow_state (include/tkr.h): granule tables of the persistent dataflow step"""
    _fields_ = [(n, C.c_void_p) for n in ('U', 'msU', 'tailU', 'rdU', 'V', 'msV', 'tailV', 'rdV')] + \
               [(n, C.c_int32) for n in ('n_users', 'n_items', 'k', 'mode')] + \
               [(n, C.c_float) for n in ('lu', 'li', 'lj', 'lb', 'lr', 'rho', 'eps')] + [('opt', C.c_int32), ('item_bufs', C.c_int32)]


class VbprState(C.Structure):
    """mirror of tkr_vbpr_state (include/tkr.h)"""
    _fields_ = [(n, C.c_void_p) for n in ('U', 'msU', 'I', 'msI', 'irb', 'msirb', 'cem', 'mscem', 'icb', 'msicb', 'feat')] + \
               [(n, C.c_int32) for n in ('n_users', 'n_items', 'kh', 'd', 'mode')] + \
               [(n, C.c_float) for n in ('lu', 'li', 'lj', 'lb', 'le', 'lr', 'rho', 'eps')] + \
               [(n, C.c_void_p) for n in ('f_ptr', 'f_col', 'f_val', 'c_ptr', 'c_item', 'c_val', 'item_tag')]


EXPORTS = ('tkr_version', 'tkr_plan_team', 'tkr_plan_max_blocks', 'tkr_sample_plan', 'tkr_sample_plan_owned', 'tkr_plan_rollback', 'tkr_bpr_run', 'tkr_bpr_flow_run', 'tkr_bpr_own_run', 'tkr_bpr_own_run_between', 'tkr_bpr_own_plan_run', 'tkr_bpr_own_owners', 'tkr_bpr_own_owners_shared', 'tkr_flow_row_granules', 'tkr_flow_ctl_words',
           'tkr_vbpr_run', 'tkr_vbpr_colplan', 'tkr_vbpr_run_cols', 'tkr_build_rated_mask', 'tkr_score_topk', 'tkr_count_hits', 'tkr_calib_rowcopy',
           'tkr_idmap_create', 'tkr_idmap_destroy', 'tkr_ratings_parse', 'tkr_ratings_sizes', 'tkr_ratings_copy',
           'tkr_ratings_destroy', 'tkr_matrix_read', 'tkr_matrix_sizes', 'tkr_matrix_copy', 'tkr_matrix_destroy',
           'tkr_matrix_write', 'tkr_raw_ranks', 'tkr_count_hits_rr', 'tkr_topk_set_math', 'tkr_vbpr_set_pairs', 'tkr_lab_build',
           'tkr_sync_snapshot', 'tkr_sync_pack', 'tkr_sync_unpack', 'tkr_sync_flow_snapshot', 'tkr_sync_flow_pack',
           'tkr_sync_flow_unpack', 'tkr_like_ranks', 'tkr_bpr_foldin', 'tkr_bpr_foldin_items', 'tkr_idtable_build', 'tkr_ratings_count_dev',
           'tkr_ratings_emit_dev', 'tkr_rank_candidates', 'tkr_lists_format_sizes_dev', 'tkr_lists_format_emit_dev',
           'tkr_matrix_format_sizes_dev', 'tkr_matrix_format_emit_dev', 'tkr_matrix_count_dev', 'tkr_matrix_emit_dev', 'tkr_matrix_token_host',
           'tkr_matrix_tokens_host', 'tkr_group_count_dev', 'tkr_group_emit_dev', 'tkr_last_line_of_user_dev', 'tkr_compact_rows_count_dev',
           'tkr_compact_rows_emit_dev', 'tkr_fusion_features', 'tkr_fusion_sgd', 'tkr_fusion_user_weights', 'tkr_fusion_svm_sums',
           'tkr_mmr_select', 'tkr_list_pair_sums', 'tkr_line_metrics', 'tkr_bootstrap_sums', 'tkr_nearest_anchors', 'tkr_als_gram',
           'tkr_als_solve_rows', 'tkr_als_solve_rows_prior', 'tkr_mlp_forward', 'tkr_mlp_fit', 'tkr_als_cg_rows', 'tkr_als_gram_wide',
           'tkr_lmf_dense_rows', 'tkr_lmf_step_rows', 'tkr_csr_spmm', 'tkr_estep_cg', 'tkr_smf_lse_rows', 'tkr_smf_dense_rows', 'tkr_smf_step_rows',
           'tkr_knn_build', 'tkr_knn_score', 'tkr_topk_last_report')
EXPORTS_I64 = ('tkr_vbpr_workspace_floats', 'tkr_vbpr_colplan_lds_bytes', 'tkr_topk_workspace_bytes_for', 'tkr_topk_workspace_bytes', 'tkr_plan_workspace_bytes', 'tkr_like_ranks_workspace_bytes',
               'tkr_parse_dev_workspace_bytes', 'tkr_idtable_slots', 'tkr_scan_dev_workspace_bytes', 'tkr_als_workspace_bytes',
               'tkr_als_prior_workspace_bytes', 'tkr_mlp_workspace_bytes', 'tkr_fusion_svm_partial_bytes', 'tkr_als_cg_workspace_bytes',
               'tkr_als_gram_wide_workspace_bytes', 'tkr_lmf_workspace_bytes', 'tkr_csr_spmm_workspace_bytes', 'tkr_estep_cg_workspace_bytes',
               'tkr_smf_workspace_bytes', 'tkr_knn_build_workspace_bytes')


def lib():
    """Load libtkr_hip.so once; raise if it has not been built (python __graft_entry__.py build)."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise TkrError('%s not found: build it with `make -C top-k-rec_amd/csrc` '
                           '(or __graft_entry__.build()); there is no CPU fallback' % LIB_PATH)
        _lib = C.CDLL(LIB_PATH)
        for name in EXPORTS:
            getattr(_lib, name).restype = C.c_int
        for name in EXPORTS_I64:
            getattr(_lib, name).restype = C.c_int64
        if _lib.tkr_version() != VERSION:
            raise TkrError('%s is version %d, this binding expects %d: rebuild it (make -C top-k-rec_amd/csrc)'
                           % (LIB_PATH, _lib.tkr_version(), VERSION))
    return _lib


def _check(rc, what):
    if rc != 0:
        kind = 'hipError_t' if rc > 0 else 'tkr error'
        raise TkrError('%s failed: %s %d' % (what, kind, rc))


def _p(t):
    if t is None:
        return C.c_void_p(0)
    assert t.is_cuda and t.is_contiguous(), 'device-resident contiguous tensor required'
    return C.c_void_p(t.data_ptr())


def _call(name, anchor, *args):
    """lib().<name>(*args, stream) on the device that owns tensor `anchor` and on torch's current stream OF THAT
    DEVICE: a kernel launched while another device is current would run there against this device's pointers"""
    dev = anchor.device.index
    prev = torch.cuda.current_device()
    if prev != dev:
        torch.cuda.set_device(dev)
    try:
        _check(getattr(lib(), name)(*args, C.c_void_p(torch.cuda.current_stream(anchor.device).cuda_stream)), name)
    finally:
        if prev != dev:
            torch.cuda.set_device(prev)


def version():
    return lib().tkr_version()


PLAN_MAX_BATCHES = 512      # per tkr_sample_plan call (16 bitmap words per row)


def plan_team(B):
    return lib().tkr_plan_team(C.c_int32(B))


def plan_workspace_bytes(B, n_batches):
    return int(lib().tkr_plan_workspace_bytes(C.c_int32(B), C.c_int32(n_batches)))


def plan_max_blocks(B):
    return lib().tkr_plan_max_blocks(C.c_int32(B))


def sample_plan(csr, n_users, n_items, seed, first_triplet, n_batches, B, cnt, plan, ctl=None):
    """csr: tensors tr_users,row_ptr,pos_cols,cols_sorted; cnt: ucnt,icnt,touch_u,touch_i;
    plan: u,i,j,task,occ,occt + either rec,hdr,tpar (one launch per batch, K2/K3) or prec,pocc (dataflow form, K2f; with
    plan.owners > 0 and plan.ohdr the owner-ordered form of K2o); all int32 device tensors."""
    assert n_batches <= PLAN_MAX_BATCHES
    assert plan.u.numel() >= n_batches * B and plan.task.numel() >= n_batches * 3 * B * 4
    prec, pocc = getattr(plan, 'prec', None), getattr(plan, 'pocc', None)
    if getattr(plan, 'owners', 0) > 0:
        assert ctl is None and prec.numel() >= n_batches * 3 * B * 32 and pocc.numel() >= n_batches * 3 * B * 4
        assert plan.ohdr.numel() >= plan.owners * plan.cap and plan.cap >= n_batches
        _call('tkr_sample_plan_owned', plan.u, _p(csr.tr_users), C.c_int32(csr.tr_users.numel()), _p(csr.row_ptr), _p(csr.pos_cols),
              _p(csr.cols_sorted), C.c_int32(n_users), C.c_int32(n_items), C.c_uint64(seed), C.c_uint64(first_triplet),
              C.c_int32(n_batches), C.c_int32(B), _p(cnt.ucnt), _p(cnt.icnt), _p(cnt.touch_u), _p(cnt.touch_i), _p(plan.u), _p(plan.i),
              _p(plan.j), _p(plan.task), _p(plan.occ), _p(plan.occt), _p(prec), _p(pocc), C.c_int32(plan.owners), _p(plan.ohdr),
              C.c_int32(plan.cap))
        return
    ws = getattr(plan, 'ws', None)                      # device scratch of the grid-wide planner (B > 8192)
    assert ws is None or ws.numel() >= plan_workspace_bytes(B, n_batches)
    assert B <= 8192 or ws is not None
    if prec is not None:
        assert prec.numel() >= n_batches * 3 * B * 32 and pocc.numel() >= n_batches * 3 * B * 4
    else:
        assert plan.rec.numel() >= n_batches * plan_max_blocks(B) * plan_team(B) * 16 and plan.hdr.numel() >= n_batches * 4
    assert cnt.ucnt.numel() == n_users and cnt.touch_u.numel() == n_users * 16
    assert cnt.icnt.numel() == n_items and cnt.touch_i.numel() == n_items * 16
    _call('tkr_sample_plan', plan.u, _p(csr.tr_users), C.c_int32(csr.tr_users.numel()), _p(csr.row_ptr), _p(csr.pos_cols),
                                 _p(csr.cols_sorted), C.c_int32(n_users), C.c_int32(n_items), C.c_uint64(seed),
                                 C.c_uint64(first_triplet), _p(ctl), C.c_int32(n_batches), C.c_int32(B),
                                 _p(cnt.ucnt), _p(cnt.icnt), _p(cnt.touch_u), _p(cnt.touch_i),
                                 _p(plan.u), _p(plan.i), _p(plan.j), _p(plan.task), _p(plan.occ), _p(getattr(plan, 'rec', None)),
                                 _p(getattr(plan, 'hdr', None)), _p(plan.occt), _p(getattr(plan, 'tpar', None)), _p(prec), _p(pocc),
                                 _p(ws), C.c_int64(ws.numel() if ws is not None else 0))


_PLAN_ARGTYPES = [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_uint64, C.c_uint64, C.c_void_p,
                  C.c_int32, C.c_int32] + [C.c_void_p] * 15 + [C.c_void_p, C.c_int64, C.c_void_p]


def plan_caller(csr, n_users, n_items, seed, B, cnt, plan):
    """-> call(first_triplet, n_batches): sample_plan with everything that does not change between calls checked and marshalled
    ONCE (a short run_batches call is ~150 us of device time; building ~30 ctypes arguments and their assertions per call sat in
    front of its first launch with the GPU idle)."""
    sample_plan.__doc__                                  # same contract
    prec, pocc = getattr(plan, 'prec', None), getattr(plan, 'pocc', None)
    ws = getattr(plan, 'ws', None)
    assert B <= 8192 or ws is not None
    assert cnt.ucnt.numel() == n_users and cnt.touch_u.numel() == n_users * 16
    assert cnt.icnt.numel() == n_items and cnt.touch_i.numel() == n_items * 16
    cap = plan.u.numel() // B
    fn = lib().tkr_sample_plan
    fn.argtypes = _PLAN_ARGTYPES
    ptr = lambda t: None if t is None else t.data_ptr()
    for t in (csr.tr_users, csr.row_ptr, csr.pos_cols, csr.cols_sorted, cnt.ucnt, cnt.icnt, cnt.touch_u, cnt.touch_i, plan.u, plan.task):
        assert t.is_cuda and t.is_contiguous()
    fixed_a = (ptr(csr.tr_users), int(csr.tr_users.numel()), ptr(csr.row_ptr), ptr(csr.pos_cols), ptr(csr.cols_sorted), n_users, n_items, seed)
    fixed_b = (ptr(cnt.ucnt), ptr(cnt.icnt), ptr(cnt.touch_u), ptr(cnt.touch_i), ptr(plan.u), ptr(plan.i), ptr(plan.j), ptr(plan.task), ptr(plan.occ),
               ptr(getattr(plan, 'rec', None)), ptr(getattr(plan, 'hdr', None)), ptr(plan.occt), ptr(getattr(plan, 'tpar', None)), ptr(prec), ptr(pocc),
               ptr(ws), int(ws.numel()) if ws is not None else 0)
    device = plan.u.device
    keep = (csr, cnt)                                    # these live as long as the closure; the closure itself is kept ON the plan buffer
                                                         # (no reference back to it: a cycle would delay the release of a replaced buffer)
    owners = getattr(plan, 'owners', 0)
    if owners > 0:                                       # the owner-ordered dataflow form (K2o)
        fo = lib().tkr_sample_plan_owned
        fo.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_uint64, C.c_uint64, C.c_int32,
                       C.c_int32] + [C.c_void_p] * 12 + [C.c_int32, C.c_void_p, C.c_int32, C.c_void_p]
        tail = (ptr(cnt.ucnt), ptr(cnt.icnt), ptr(cnt.touch_u), ptr(cnt.touch_i), ptr(plan.u), ptr(plan.i), ptr(plan.j), ptr(plan.task),
                ptr(plan.occ), ptr(plan.occt), ptr(prec), ptr(pocc), owners, ptr(plan.ohdr), plan.cap)

        def call_owned(first_triplet, n_batches):
            assert 0 < n_batches <= min(cap, PLAN_MAX_BATCHES) and keep
            prev = torch.cuda.current_device()
            if prev != device.index:
                torch.cuda.set_device(device.index)
            try:
                rc = fo(*fixed_a, first_triplet, n_batches, B, *tail, torch.cuda.current_stream(device).cuda_stream)
            finally:
                if prev != device.index:
                    torch.cuda.set_device(prev)
            if rc:
                _check(rc, 'tkr_sample_plan_owned')
        return call_owned

    def call(first_triplet, n_batches):
        assert 0 < n_batches <= min(cap, PLAN_MAX_BATCHES) and keep
        if torch.cuda.current_device() != device.index:
            prev = torch.cuda.current_device()
            torch.cuda.set_device(device.index)
            try:
                rc = fn(*fixed_a, first_triplet, None, n_batches, B, *fixed_b, torch.cuda.current_stream(device).cuda_stream)
            finally:
                torch.cuda.set_device(prev)
            if rc:
                _check(rc, 'tkr_sample_plan')
            return
        rc = fn(*fixed_a, first_triplet, None, n_batches, B, *fixed_b, torch.cuda.current_stream(device).cuda_stream)
        if rc:
            _check(rc, 'tkr_sample_plan')
    return call


def plan_rollback(plan, B, first_batch, n_batches, cnt):
    """take batches [first_batch, first_batch + n_batches) of a plan out of the update counters again"""
    _call('tkr_plan_rollback', plan.task, _p(plan.task), C.c_int32(B), C.c_int32(first_batch), C.c_int32(n_batches),
                                   _p(cnt.ucnt), _p(cnt.icnt))


def _at(t, offset):
    """device pointer `offset` elements into tensor t (None -> NULL)"""
    if t is None:
        return C.c_void_p(0)
    assert t.is_cuda and t.is_contiguous() and 0 <= offset <= t.numel()
    return C.c_void_p(t.data_ptr() + offset * t.element_size())


def bpr_run(state, plan, B, n_batches, loss_out=None, first=0):
    """batches [first, first + n_batches) of a plan"""
    rs = plan_max_blocks(B) * plan_team(B) * 16
    _call('tkr_bpr_run', plan.rec, C.byref(state), _at(plan.rec, first * rs), _at(plan.occ, first * 6 * B), _at(plan.hdr, first * 4),
                             C.c_int32(B), C.c_int32(n_batches), _at(loss_out, first))


FLOW_MAX_K = 256         # K2f holds a row in 2 x (k / 128) registers per lane: csrc/bpr_flow.hip


def flow_row_granules(k):
    return int(lib().tkr_flow_row_granules(C.c_int32(k)))


def flow_ctl_words():
    return int(lib().tkr_flow_ctl_words())


FLOW_CTL_ARRIVE, FLOW_CTL_STATUS, FLOW_CTL_SPINS = 1024, 1026, 1027      # TKR_FLOW_CTL_* of include/tkr.h (32 ticket counters, 32 words apart, come first)
FLOW_CTL_DEBUG, FLOW_CTL_PROF = 1032, 1056       # post-mortem of a timed-out wait (16 words); TKR_FLOW_PROFILE=1 cycle sums (8 x uint64)


def bpr_flow_run(state, plan, B, n_batches, ctl, loss_out=None, first=0, waves_per_cu=0):
    """batches [first, first + n_batches) of a dataflow plan in ONE persistent launch"""
    _call('tkr_bpr_flow_run', plan.prec, C.byref(state), _at(plan.prec, first * 3 * B * 32), _p(plan.pocc), C.c_int32(B),
          C.c_int32(n_batches), _p(ctl), _p(loss_out), C.c_int32(waves_per_cu))


def flow_stepper(state, B, ctl, waves_per_cu=0):
    """-> step(plan, first, n_batches, loss_out): bpr_flow_run with everything that does not change between calls bound once
    (a 20-batch call is ~70 us of device time: the argument marshalling of the general path is a tenth of that)"""
    fn = lib().tkr_bpr_flow_run
    fn.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p]
    device, st = ctl.device, C.addressof(state)
    ctl_ptr, rec_bytes = ctl.data_ptr(), 3 * B * 32 * 4

    def step(plan, first, n_batches, loss_out):
        if torch.cuda.current_device() != device.index:            # the guarded path of _call
            return bpr_flow_run(state, plan, B, n_batches, ctl, loss_out, first, waves_per_cu)
        rc = fn(st, plan.prec.data_ptr() + first * rec_bytes, plan.pocc.data_ptr(), B, n_batches, ctl_ptr,
                None if loss_out is None else loss_out.data_ptr(), waves_per_cu, torch.cuda.current_stream(device).cuda_stream)
        if rc:
            _check(rc, 'tkr_bpr_flow_run')
    step.state = state                                              # the struct lives as long as the closure
    return step


def bpr_own_owners(n_items, k, device=None, share=1):
    """workgroups (= owners of item rows) of the persistent step K2o on the current device when `share` processes split its CUs,
    0 = the rows do not fit the owners' LDS"""
    if device is not None and torch.cuda.current_device() != device.index:
        with torch.cuda.device(device):
            return int(lib().tkr_bpr_own_owners_shared(C.c_int32(n_items), C.c_int32(k), C.c_int32(share)))
    return int(lib().tkr_bpr_own_owners_shared(C.c_int32(n_items), C.c_int32(k), C.c_int32(share)))


def bpr_own_run(state, plan, B, n_batches, ctl, loss_out=None, first=0, owner_waves=0):
    """batches [first, first + n_batches) of an owner-ordered dataflow plan in ONE persistent launch of K2o"""
    plan.epoch += 1                       # no two launches on one plan buffer's scalar slots share an epoch
    _call('tkr_bpr_own_run', plan.prec, C.byref(state), _p(plan.prec), _p(plan.pocc), _p(plan.occt), _p(plan.ohdr), C.c_int32(plan.cap), C.c_int32(plan.owners),
          C.c_int32(B), C.c_int32(first), C.c_int32(n_batches), _p(ctl), _p(loss_out), C.c_int32(owner_waves), _p(plan.xch),
          C.c_uint32(plan.epoch & 0xffffffff or 1))


def own_stepper(state, B, ctl, owner_waves=0):
    """-> step(plan, first, n_batches, loss_out, events=None): bpr_own_run with the fixed arguments bound once (as flow_stepper);
    events = (before, after): two torch events that have been recorded once (so they exist), recorded around the launch in C"""
    fn = lib().tkr_bpr_own_run_between
    fn.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32,
                   C.c_int32, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_uint32, C.c_void_p]
    device, st, ctl_ptr = ctl.device, C.addressof(state), ctl.data_ptr()

    def step(plan, first, n_batches, loss_out, events=None):
        if torch.cuda.current_device() != device.index:
            assert events is None
            return bpr_own_run(state, plan, B, n_batches, ctl, loss_out, first, owner_waves)
        plan.epoch += 1
        rc = fn(None if events is None else events[0].cuda_event, None if events is None else events[1].cuda_event,
                st, plan.prec.data_ptr(), plan.pocc.data_ptr(), plan.occt.data_ptr(), plan.ohdr.data_ptr(), plan.cap, plan.owners, B, first, n_batches,
                ctl_ptr, None if loss_out is None else loss_out.data_ptr(), owner_waves, plan.xch.data_ptr(), plan.epoch & 0xffffffff or 1,
                torch.cuda.current_stream(device).cuda_stream)
        if rc:
            _check(rc, 'tkr_bpr_own_run_between')
    fused = lib().tkr_bpr_own_plan_run
    fused.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_uint32, C.c_void_p,
                      C.c_void_p, C.c_void_p]

    raw_stream = getattr(torch._C, '_cuda_getCurrentRawStream', None)          # the stream's handle without a Stream object around it (~1 us)
    dev_index = device.index

    def plan_and_run(plan, call, first, n_batches, loss_out, events=None):
        """K1 of the chunk described by `call` (a PlanCall into `plan`) and the step on its batches [first, first + n_batches): one C call"""
        assert torch.cuda.current_device() == dev_index and 0 < call.n_batches <= min(plan.cap, PLAN_MAX_BATCHES)
        plan.epoch += 1
        stream = raw_stream(dev_index) if raw_stream is not None else torch.cuda.current_stream(device).cuda_stream
        rc = fused(C.addressof(call), st, first, n_batches, ctl_ptr, None if loss_out is None else loss_out.data_ptr(), owner_waves,
                   plan.xch.data_ptr(), plan.epoch & 0xffffffff or 1, None if events is None else events[0].cuda_event,
                   None if events is None else events[1].cuda_event, stream)
        if rc:
            _check(rc, 'tkr_bpr_own_plan_run')
    step.state = state
    step.takes_events = True
    step.plan_and_run = plan_and_run
    step.assigns_loss = True          # loss_out[b] is written, not added to (csrc/bpr_own.hip own_loss_kernel)
    return step


def set_vbpr_pairs(mode):
    """where tkr_vbpr_run_cols forms a batch's pair sums: 0 own launch, the only placement; 1 and 2 were removed (include/tkr.h)"""
    _check(lib().tkr_vbpr_set_pairs(C.c_int32(int(mode))), 'tkr_vbpr_set_pairs')


def vbpr_workspace_floats(B, kh, d):
    return int(lib().tkr_vbpr_workspace_floats(C.c_int32(B), C.c_int32(kh), C.c_int32(d)))


def _vbpr_plan_at(plan, B, first):
    """tri_i, tri_j, rec, occ, hdr, occt, tri_u, tpar of a plan at batch `first` (tpar: NULL for a plan without K1's parities)"""
    rs = plan_max_blocks(B) * plan_team(B) * 16
    return (_at(plan.i, first * B), _at(plan.j, first * B), _at(plan.rec, first * rs), _at(plan.occ, first * 6 * B), _at(plan.hdr, first * 4),
            _at(plan.occt, first * 3 * B), _at(plan.u, first * B), _at(getattr(plan, 'tpar', None), first * B))


def vbpr_run(state, plan, B, n_batches, workspace, loss_out=None, first=0):
    _call('tkr_vbpr_run', plan.rec, C.byref(state), *_vbpr_plan_at(plan, B, first), C.c_int32(B), C.c_int32(n_batches), _p(workspace),
          _at(loss_out, first))


def vbpr_colplan_lds_bytes(B, d):
    return int(lib().tkr_vbpr_colplan_lds_bytes(C.c_int32(B), C.c_int32(d)))


def vbpr_colplan(sparse, d, plan, B, n_batches, row_cap):
    """K1-side preparation of the column-plan VBPR step: plan.colh / cent / tcnt / tent from plan.i / plan.j and the CSR of feat"""
    tcap = 2 * row_cap
    assert plan.colh.numel() >= n_batches * d * 8 and plan.cent.numel() >= n_batches * B * tcap * 2
    assert plan.tcnt.numel() >= n_batches * B and plan.tent.numel() >= n_batches * B * tcap * 2
    _call('tkr_vbpr_colplan', plan.i, _p(sparse['f_ptr']), _p(sparse['f_col']), _p(sparse['f_val']), C.c_int32(d), _p(plan.i), _p(plan.j),
          C.c_int32(B), C.c_int32(n_batches), C.c_int32(row_cap), _p(plan.colh), _p(plan.cent), _p(plan.tcnt), _p(plan.tent))


def vbpr_run_cols(state, plan, B, n_batches, workspace, d, row_cap, cols_per_block=0, loss_out=None, first=0):
    ent = B * 2 * row_cap * 2
    _call('tkr_vbpr_run_cols', plan.rec, C.byref(state), *_vbpr_plan_at(plan, B, first), _at(plan.colh, first * d * 8), _at(plan.cent, first * ent),
          _at(plan.tcnt, first * B), _at(plan.tent, first * ent), C.c_int32(row_cap), C.c_int32(cols_per_block), C.c_int32(B), C.c_int32(n_batches),
          _p(workspace), _at(loss_out, first))


# ---- K4 / K5 -------------------------------------------------------------------------------------
def build_rated_mask(rated_ptr, rated_cols, n_rows, n_cols):
    """CSR (int64 ptr, int32 ascending cols; both on device) -> bitmask [ceil(n_cols/32)][pitch] uint32"""
    assert rated_ptr.dtype == torch.int64 and rated_cols.dtype == torch.int32
    pitch = (n_rows + 31) // 32 * 32
    mask = torch.zeros(((n_cols + 31) // 32) * pitch, dtype=torch.int32, device=rated_ptr.device)
    if rated_cols.numel() == 0:
        rated_cols = torch.zeros(1, dtype=torch.int32, device=rated_ptr.device)
    _call('tkr_build_rated_mask', mask, _p(rated_ptr), _p(rated_cols), C.c_int32(n_rows), C.c_int32(n_cols), _p(mask), C.c_int32(pitch))
    return mask, pitch


_topk_ws = {}


def _topk_workspace(n_rows, K, device, n_cols=0, k=0):
    """cached scratch for the item-range split and the pre-converted item factors (grows on demand, per device)"""
    need = int(lib().tkr_topk_workspace_bytes_for(C.c_int32(n_rows), C.c_int32(n_cols), C.c_int32(k), C.c_int32(K)))
    ws = _topk_ws.get(device)
    if ws is None or ws.numel() < need:
        ws = _topk_ws[device] = torch.empty(need, dtype=torch.uint8, device=device)
    return ws


TOPK_MAX_K = 32      # one launch of K4 ranks at most this many columns per row


def _score_topk_once(U, Vt, K, bias, user_idx, mask, mask_pitch, want_scores, split):
    n_rows = int(user_idx.numel()) if user_idx is not None else int(U.shape[0])
    ids = torch.empty((n_rows, K), dtype=torch.int32, device=U.device)
    scores = torch.empty((n_rows, K), dtype=torch.float32, device=U.device) if want_scores else None
    ws = _topk_workspace(n_rows, K, U.device, int(Vt.shape[0]), int(U.shape[1])) if split else None
    _call('tkr_score_topk', U, _p(U), _p(user_idx), C.c_int32(n_rows), _p(Vt), _p(bias), C.c_int32(Vt.shape[0]),
                                C.c_int32(U.shape[1]), _p(mask), C.c_int32(mask_pitch), C.c_int32(K), _p(ids),
                                _p(scores), _p(ws), C.c_int64(ws.numel() if ws is not None else 0))
    return ids, scores


TOPK_MATH_DEFAULT = 'refine'


def set_topk_math(mode):
    """'refine' (default: one scaled fp16 pass with a rigorous error bound picks the candidates, the arithmetic of 'fp32' ranks
    them -- same lists and score bits as 'fp32'; k <= 128) or 'fp32' (fp32 MFMA) -- see include/tkr.h.  'bf16x3' was removed: the
    library refuses it (TKR_E_UNSUPPORTED)"""
    _check(lib().tkr_topk_set_math(C.c_int32({'bf16x3': 0, 'fp32': 1, 'refine': 2}[mode])), 'tkr_topk_set_math')


def topk_last_report(max_blocks=4096):
    """A diagnostic (include/tkr.h tkr_topk_last_report): what the last score_topk launch of the process did -> dict with
    form (0 no bound-and-refine pass, 1 first form, 2 second), id_bits, image, blocks, pieces, flagged (user blocks the fp32 kernel
    had to redo) and flags (0 / 1 per block, the first max_blocks).  Synchronises the launch's stream.  Valid until the next
    score_topk (the workspace _topk_workspace caches per device keeps the flag words alive); for K > TOPK_MAX_K it speaks of the last
    pass."""
    out = (C.c_int32 * (6 + max_blocks))()
    _check(lib().tkr_topk_last_report(out, C.c_int32(len(out))), 'tkr_topk_last_report')
    return dict(form=out[0], id_bits=out[1], image=bool(out[2]), blocks=out[3], pieces=out[4], flagged=out[5],
                flags=list(out[6:6 + min(out[3], max_blocks)]))


def lab():
    """False: the `make LAB=1` build with the kernel forms that were measured and dropped (K2o scalar exchange / scout / 8 and 16
    waves / loader ring, K4 bf16x3, the VBPR pair-sum placements 1 and 2) is removed; tkr_lab_build() stays in the ABI and returns 0"""
    return bool(lib().tkr_lab_build())


def score_topk(U, Vt, K, bias=None, user_idx=None, mask=None, mask_pitch=0, want_scores=False, split=True):
    """-> ids int32 [n_rows, K] (and scores fp32 [n_rows, K]).

    K > 32 (evaluate.py -t above 32) is served exactly by several launches: the best 32, then the best 32
    of what is left (the columns already found are added to a copy of the rated mask), and so on."""
    assert U.dtype == torch.float32 and Vt.dtype == torch.float32 and U.shape[1] == Vt.shape[1]
    if U.shape[1] > 768 and not getattr(score_topk, '_warned_wide', False):
        score_topk._warned_wide = True
        warnings.warn('K4: factor width %d is above 768, where a workgroup\'s users no longer stay resident as MFMA operands: the generic '
                      'form runs (one wave per row, every lane gathers its own item row: csrc/topk.hip score_topk_wide_kernel)' % U.shape[1])
    if K <= TOPK_MAX_K:
        ids, scores = _score_topk_once(U, Vt, K, bias, user_idx, mask, mask_pitch, want_scores, split)
        return (ids, scores) if want_scores else ids
    n_rows = int(user_idx.numel()) if user_idx is not None else int(U.shape[0])
    n_cols = int(Vt.shape[0])
    pitch = mask_pitch if mask is not None else (n_rows + 31) // 32 * 32
    work = mask.clone() if mask is not None else torch.zeros(((n_cols + 31) // 32) * pitch, dtype=torch.int32, device=U.device)
    ptr = torch.arange(0, (n_rows + 1) * TOPK_MAX_K, TOPK_MAX_K, dtype=torch.int64, device=U.device)
    parts_i, parts_s, left = [], [], K
    while left > 0:
        ids, scores = _score_topk_once(U, Vt, TOPK_MAX_K, bias, user_idx, work, pitch, want_scores, split)
        take = min(left, TOPK_MAX_K)
        parts_i.append(ids[:, :take])
        if want_scores:
            parts_s.append(scores[:, :take])
        left -= take
        if left > 0:      # found columns join the mask (negative ids = padding are skipped by the kernel)
            _call('tkr_build_rated_mask', work, _p(ptr), _p(ids.reshape(-1)), C.c_int32(n_rows), C.c_int32(n_cols), _p(work), C.c_int32(pitch))
    ids = torch.cat(parts_i, dim=1).contiguous()
    return (ids, torch.cat(parts_s, dim=1).contiguous()) if want_scores else ids


def count_hits(ids, like_ptr, like_cols, step, interval):
    """-> int64[interval]: hits per bucket as evaluate.py accumulates them (cumulative over buckets)"""
    assert ids.dtype == torch.int32 and like_ptr.dtype == torch.int64 and like_cols.dtype == torch.int32
    first = torch.zeros(max(interval, 1), dtype=torch.int64, device=ids.device)
    if like_cols.numel() == 0:
        like_cols = torch.zeros(1, dtype=torch.int32, device=ids.device)
    _call('tkr_count_hits', ids, _p(ids), C.c_int32(ids.shape[0]), C.c_int32(ids.shape[1]), _p(like_ptr), _p(like_cols),
                                C.c_int32(step), C.c_int32(interval), _p(first))
    return torch.cumsum(first[:interval], 0)


def raw_ranks(U, Vt, ids, rated_ptr, rated_cols, bias=None, user_idx=None):
    """K6 -> int32 [n_rows, K]: rank of every kept column among ALL columns of its row (utils.py:113)"""
    assert ids.dtype == torch.int32 and rated_ptr.dtype == torch.int64 and rated_cols.dtype == torch.int32
    n_rows, K = int(ids.shape[0]), int(ids.shape[1])
    out = torch.empty((n_rows, K), dtype=torch.int32, device=ids.device)
    if rated_cols.numel() == 0:
        rated_cols = torch.zeros(1, dtype=torch.int32, device=ids.device)
    _call('tkr_raw_ranks', ids, _p(U), _p(user_idx), C.c_int32(n_rows), _p(Vt), _p(bias), C.c_int32(U.shape[1]), _p(rated_ptr),
                               _p(rated_cols), _p(ids), C.c_int32(K), _p(out))
    return out


def count_hits_rr(ids, raw_rank, like_ptr, like_cols, step, interval):
    """K7 -> (hits int64[interval], trrs float64[interval]) accumulated over buckets like utils.py:115-117"""
    n_rows = int(ids.shape[0])
    hit = torch.zeros((n_rows, max(interval, 1)), dtype=torch.int32, device=ids.device)
    rr = torch.zeros((n_rows, max(interval, 1)), dtype=torch.float64, device=ids.device)
    if like_cols.numel() == 0:
        like_cols = torch.zeros(1, dtype=torch.int32, device=ids.device)
    if interval > 0:
        _call('tkr_count_hits_rr', ids, _p(ids), _p(raw_rank), C.c_int32(n_rows), C.c_int32(ids.shape[1]), _p(like_ptr),
                                       _p(like_cols), C.c_int32(step), C.c_int32(interval), _p(hit), _p(rr))
    return torch.cumsum(hit.sum(0, dtype=torch.int64)[:interval], 0), torch.cumsum(rr.sum(0)[:interval], 0)


def like_ranks(U, Vt, like_ptr, like_cols, bias=None, user_idx=None, mask=None, mask_pitch=0):
    """K8 -> int32 [n_likes] (device): for every entry of the like CSR (int64 ptr from 0, int32 ascending cols) the number of unmasked
    columns in front of it in K4's canonical order, -1 where the liked column itself is masked (include/tkr.h)"""
    assert U.dtype == torch.float32 and Vt.dtype == torch.float32 and U.shape[1] == Vt.shape[1]
    assert like_ptr.dtype == torch.int64 and like_cols.dtype == torch.int32
    n_rows = int(user_idx.numel()) if user_idx is not None else int(U.shape[0])
    assert like_ptr.numel() == n_rows + 1
    n_likes, n_cols, k = int(like_cols.numel()), int(Vt.shape[0]), int(U.shape[1])
    out = torch.empty(n_likes, dtype=torch.int32, device=U.device)
    if n_likes == 0:
        return out
    need = int(lib().tkr_like_ranks_workspace_bytes(C.c_int32(n_rows), C.c_int32(n_cols), C.c_int32(k), C.c_int64(n_likes)))
    ws = torch.empty(need, dtype=torch.uint8, device=U.device)
    _call('tkr_like_ranks', U, _p(U), _p(user_idx), C.c_int32(n_rows), _p(Vt), _p(bias), C.c_int32(n_cols), C.c_int32(k), _p(mask),
          C.c_int32(mask_pitch), _p(like_ptr), _p(like_cols), _p(out), _p(ws), C.c_int64(need))
    return out


# ---- what the bindings of K12 and every family after it share: one operand check, one reader of the status word, one size call ------
_STD = (TypeError, ValueError)     # what an operand check raises in K12 / K15 style: (not a tensor or a wrong dtype, the rest)
_TKR = (TkrError, TkrError)        # ... and in every other family
_LATER = object()                  # on=_LATER: the entry point has rules of its own to check first and calls _on_gpu itself


def _on_gpu(what, name, t, on=None, raises=_TKR):
    """the last check of an operand: on a GPU, and on the GPU `on` where the entry point has an anchor"""
    if not t.is_cuda or (on is not None and t.device != on):
        raise raises[1]('%s: %s must live on the GPU, one GPU for every operand of the call, not on %s' % (what, name, t.device))


def _operand(what, name, t, dtype, dim=None, numel=None, at_least=None, on=None, optional=False, raises=_TKR):
    """refuse the tensor operand `name` of the entry point `what` by its properties alone (no device access), always in this order:
    a tensor, the dtype, contiguous, `dim` dimensions, `numel` values (or `at_least` that many), on the GPU (_on_gpu)"""
    if t is None and optional:
        return
    if not isinstance(t, torch.Tensor):
        raise raises[0]('%s: %s must be a tensor' % (what, name))
    if t.dtype != dtype:
        raise raises[0]('%s: %s must be %s, not %s' % (what, name, dtype, t.dtype))
    if not t.is_contiguous():
        raise raises[1]('%s: %s must be contiguous' % (what, name))
    if dim is not None and t.dim() != dim:
        raise raises[1]('%s: %s must have %d dimensions, not %d' % (what, name, dim, t.dim()))
    if numel is not None and t.numel() != numel:
        raise raises[1]('%s: %s must hold %d values, not %d' % (what, name, numel, t.numel()))
    if at_least is not None and t.numel() < at_least:
        raise raises[1]('%s: %s must hold at least %d values, not %d' % (what, name, at_least, t.numel()))
    if on is not _LATER:
        _on_gpu(what, name, t, on, raises)


def status_check(what, messages, raises, word):
    """the one reader of a status word in the convention of K15 (include/tkr.h): -1 is clean; anything else is 4 * row + kind and
    raises `raises` (a class, or one class per kind) with messages[kind] about the row, and .word, .row and .kind set.  A kind the
    family does not write is a TkrError that names the word."""
    if word == -1:
        return
    row, kind = word >> 2, word & 3
    if kind >= len(messages) or messages[kind] is None:
        raise TkrError('%s: status word %d (row %d, kind %d) is none of the refusals this entry point knows' % (what, word, row, kind))
    error = (raises[kind] if isinstance(raises, tuple) else raises)('%s: %s' % (what, messages[kind] % row))
    error.word, error.row, error.kind = word, row, kind
    raise error


def _done(what, result, status, check, messages, raises):
    """the tail of every wrapper with a check= argument: check=False hands the status word on unread, else it is read and a refusal
    raised"""
    if not check:
        return result, status
    status_check(what, messages, raises, int(status.item()))
    return result


def _size(entry, types, values, shown=None):
    """a *_workspace_bytes / *_partial_bytes export called with `values` (`shown`: how the message writes them) -> bytes"""
    need = int(getattr(lib(), entry)(*(t(v) for t, v in zip(types, values))))
    if need < 0:
        raise TkrError('%s(%s) failed: tkr error %d' % (entry, ', '.join('%d' % v for v in values) if shown is None else shown, need))
    return need


def _chunked_size(entry, what, n_bytes, chunk_bytes):
    try:
        return _size(entry, (C.c_int64, C.c_int64), (n_bytes, chunk_bytes))
    except TkrError:
        raise ValueError('%s on the device: chunk_bytes must be a power of two in [%d, %d], got %r'
                         % (what, PARSE_CHUNK_MIN, PARSE_CHUNK_MAX, chunk_bytes)) from None


# ---- K12: per-user candidate lists (csrc/candidates.hip) ----------------------------------------------------------------------------
CANDIDATES_RESIDENT = 2048   # TKR_CANDIDATES_RESIDENT of include/tkr.h: a longer row is ranked by the slow whole-workgroup form


def _cand_args(U, Vt, cand_ptr, cand_cols, bias, user_idx, mask, mask_pitch):
    """refuse what tkr_rank_candidates cannot take, the tensors' properties first (no device access), then the row pointer
    -> (n_rows, n_cols, k, nnz)"""
    what = 'rank_candidates'
    named = (('U', U, torch.float32), ('Vt', Vt, torch.float32), ('cand_ptr', cand_ptr, torch.int64), ('cand_cols', cand_cols, torch.int32),
             ('bias', bias, torch.float32), ('user_idx', user_idx, torch.int32), ('mask', mask, torch.int32))
    for name, t, dtype in named:
        _operand(what, name, t, dtype, on=_LATER, optional=name in ('bias', 'user_idx', 'mask'), raises=_STD)
    for name, t, _ in named:
        if t is not None:
            _on_gpu(what, name, t, U.device, _STD)
    if U.dim() != 2 or Vt.dim() != 2 or U.shape[1] != Vt.shape[1] or U.shape[1] < 1 or Vt.shape[0] < 1:
        raise ValueError('rank_candidates: U [*, k] and Vt [n_cols, k] must share k >= 1')
    n_rows = int(user_idx.numel()) if user_idx is not None else int(U.shape[0])
    n_cols, k, nnz = int(Vt.shape[0]), int(U.shape[1]), int(cand_cols.numel())
    if cand_ptr.dim() != 1 or cand_cols.dim() != 1 or cand_ptr.numel() != n_rows + 1:
        raise ValueError('rank_candidates: cand_ptr must hold n_rows + 1 = %d entries' % (n_rows + 1))
    if bias is not None and bias.numel() != n_cols:
        raise ValueError('rank_candidates: bias must hold one value per column')
    if mask is not None and (mask_pitch < n_rows or mask.numel() < ((n_cols + 31) // 32) * mask_pitch):
        raise ValueError('rank_candidates: the mask is not the bitmap of build_rated_mask for %d rows and %d columns' % (n_rows, n_cols))
    if n_rows and not (int(cand_ptr[0]) == 0 and int(cand_ptr[-1]) == nnz and bool((cand_ptr[1:] >= cand_ptr[:-1]).all())):
        raise ValueError('rank_candidates: cand_ptr must run from 0 to len(cand_cols) = %d and never decrease' % nnz)
    return n_rows, n_cols, k, nnz


def rank_candidates(U, Vt, cand_ptr, cand_cols, bias=None, user_idx=None, mask=None, mask_pitch=0):
    """K12 -> (scores fp32 [nnz], ranks int32 [nnz]) on the device: for every entry of the candidate CSR (int64 ptr from 0, int32 columns
    strictly ascending inside a row and in [0, n_cols) -- evaluate._group builds such rows) the score of K4's fp32 arithmetic and the
    number of unmasked candidates of the same row in front of it in K4's canonical order, -1 where the candidate itself is masked
    (include/tkr.h).  Rows longer than CANDIDATES_RESIDENT are right but slow: rank most of a catalogue with score_topk / like_ranks."""
    n_rows, n_cols, k, nnz = _cand_args(U, Vt, cand_ptr, cand_cols, bias, user_idx, mask, mask_pitch)
    scores = torch.empty(nnz, dtype=torch.float32, device=U.device)
    ranks = torch.empty(nnz, dtype=torch.int32, device=U.device)
    if nnz == 0 or n_rows == 0:
        return scores, ranks
    _call('tkr_rank_candidates', U, _p(U), _p(user_idx), C.c_int32(n_rows), _p(Vt), _p(bias), C.c_int32(n_cols), C.c_int32(k),
          _p(cand_ptr), _p(cand_cols), _p(mask), C.c_int32(mask_pitch), _p(scores), _p(ranks))
    return scores, ranks


def topk_from_ranks(cand_ptr, cand_cols, scores, ranks, K):
    """the K best candidates of every row from rank_candidates' output -> (ids int32 [n_rows, K], -1 padded; scores fp32 [n_rows, K],
    -inf padded), the padding of score_topk: the entry with rank p < K goes to position p (a torch scatter, no kernel)"""
    n_rows = int(cand_ptr.numel()) - 1
    dev = cand_cols.device
    ids = torch.full((n_rows, K), -1, dtype=torch.int32, device=dev)
    out = torch.full((n_rows, K), float('-inf'), dtype=torch.float32, device=dev)
    keep = (ranks >= 0) & (ranks < K)
    row = torch.repeat_interleave(torch.arange(n_rows, device=dev), cand_ptr[1:] - cand_ptr[:-1])[keep]
    at = row * K + ranks[keep].long()
    ids.view(-1)[at] = cand_cols[keep]
    out.view(-1)[at] = scores[keep]
    return ids, out


# ---- K9, K10: fold-in of users (csrc/foldin.hip) and of items (csrc/foldin_items.hip), one kernel body (csrc/fold_rows.h) ---------
FOLDIN_MAX_TRIPLETS = 64     # one lane of a wave draws one triplet of a step
FOLDIN_REG_MAX_K = 512       # rows up to here stay in registers
ROLE_ALWAYS_POSITIVE = 0xffffffff     # K10 role_thresh value: every triplet carries the item as the positive of a liker


def _fold_csr(ptr, idx, bound, what):
    """a CSR whose indices the kernel gathers rows by, checked once per call: the pointer runs from 0 to idx.numel() and never
    decreases, the indices lie in [0, bound).  -> idx, an empty one padded to one element (the kernel is handed no null pointer)"""
    assert ptr.dtype == torch.int64 and idx.dtype == torch.int32
    assert int(ptr[0]) == 0 and int(ptr[-1]) == idx.numel() and bool((ptr[1:] >= ptr[:-1]).all()), 'the row pointer does not describe %s' % what
    assert idx.numel() == 0 or (0 <= int(idx.min()) and int(idx.max()) < bound), '%s holds an index outside [0, %d)' % (what, bound)
    return idx if idx.numel() else torch.zeros(1, dtype=torch.int32, device=idx.device)


def _fold_warn_wide(name, row, k):
    """once per process and kernel: rows wider than the register form holds"""
    if k > FOLDIN_REG_MAX_K and name not in _fold_warn_wide.seen:
        _fold_warn_wide.seen.add(name)
        warnings.warn('%s: factor width %d is above %d, where a wave no longer holds its %s row in registers: the generic form runs '
                      '(row, slot and gradient sum in LDS, two passes over the gathered rows per triplet: csrc/fold_rows.h fold_wide_kernel)'
                      % (name, k, FOLDIN_REG_MAX_K, row))


_fold_warn_wide.seen = set()


def _fold_outputs(m, steps, triplets, width, want_loss, want_triplets, device):
    """-> (loss fp32 [m] zeros, trip int32 [m, steps, triplets, width] of -1), None where not asked for"""
    loss = torch.zeros(m, dtype=torch.float32, device=device) if want_loss else None
    trip = torch.full((m, steps, triplets, width), -1, dtype=torch.int32, device=device) if want_triplets else None
    return loss, trip


def fold_in(V, b, hist_ptr, hist_cols, *, lu, lr, mode='l2', steps, triplets, seed, first_row=0, U0=None, want_loss=False,
            want_triplets=False):
    """K9 -> U fp32 [m, k] (and loss fp32 [m], trip int32 [m, steps, triplets, 2] when asked for, in that order): the user vectors
    of m histories folded in against the frozen item factors V [n_items, k] / biases b [n_items] or None (include/tkr.h
    tkr_bpr_foldin).  hist_ptr int64 [m+1] from 0, hist_cols int32 ascending and unique per row; all tensors on V's device.
    Rows without a triplet (empty, or the whole catalogue) return U0 (zeros), loss 0 and -1 in trip."""
    assert V.dtype == torch.float32 and V.dim() == 2
    m, (n_items, k) = int(hist_ptr.numel()) - 1, V.shape
    if not 1 <= triplets <= FOLDIN_MAX_TRIPLETS or steps < 1 or m < 0:
        raise ValueError('fold_in: 1 <= triplets <= %d and steps >= 1 required' % FOLDIN_MAX_TRIPLETS)
    assert b is None or (b.dtype == torch.float32 and b.numel() == n_items)
    assert U0 is None or (U0.dtype == torch.float32 and tuple(U0.shape) == (m, k))
    hist_cols = _fold_csr(hist_ptr, hist_cols, n_items, 'hist_cols')
    _fold_warn_wide('K9', 'user', k)
    U = torch.empty((m, k), dtype=torch.float32, device=V.device)
    loss, trip = _fold_outputs(m, steps, triplets, 2, want_loss, want_triplets, V.device)
    if m:
        _call('tkr_bpr_foldin', V, _p(V), _p(b), C.c_int32(n_items), C.c_int32(k), _p(hist_ptr), _p(hist_cols), C.c_int32(m), _p(U0),
              C.c_float(lu), C.c_float(lr), C.c_int32({'l2': 0, 'l1': 1}[mode]), C.c_int32(steps), C.c_int32(triplets),
              C.c_uint64(seed & 0xffffffffffffffff), C.c_uint64(first_row), _p(U), _p(loss), _p(trip))
    out = (U,) + ((loss,) if want_loss else ()) + ((trip,) if want_triplets else ())
    return out[0] if len(out) == 1 else out


def fold_in_items(U, V, b, user_ptr, user_cols, liker_ptr, liker_rows, role_thresh, *, li, lj, lb, lr, mode='l2', steps, triplets, seed,
                  first_row=0, V0=None, b0=None, want_loss=False, want_triplets=False):
    """K10 -> (Vn fp32 [m, k], bn fp32 [m]) (then loss fp32 [m], trip int32 [m, steps, triplets, 3] = (role, u, other item) when asked
    for): rows and biases of m new items folded in against the frozen user factors U [n_users, k], item factors V [n_items, k]
    and biases b [n_items] or None (include/tkr.h tkr_bpr_foldin_items).  user_ptr int64 [n_users+1] / user_cols int32: the users'
    training positives; liker_ptr int64 [m+1] / liker_rows int32: the user rows that like each new item; both from 0, ascending and
    unique per row.  role_thresh [m]: integers in [0, 2^32) (any integer tensor or sequence).  All tensors on V's device."""
    assert U.dtype == torch.float32 and V.dtype == torch.float32 and U.dim() == 2 and V.dim() == 2 and U.shape[1] == V.shape[1]
    (n_users, k), n_items, m = U.shape, int(V.shape[0]), int(liker_ptr.numel()) - 1
    if not 1 <= triplets <= FOLDIN_MAX_TRIPLETS or steps < 1 or m < 0:
        raise ValueError('fold_in_items: 1 <= triplets <= %d and steps >= 1 required' % FOLDIN_MAX_TRIPLETS)
    assert int(user_ptr.numel()) == n_users + 1
    assert b is None or (b.dtype == torch.float32 and b.numel() == n_items)
    assert V0 is None or (V0.dtype == torch.float32 and tuple(V0.shape) == (m, k))
    assert b0 is None or (b0.dtype == torch.float32 and b0.numel() == m)
    user_cols = _fold_csr(user_ptr, user_cols, n_items, 'user_cols')
    liker_rows = _fold_csr(liker_ptr, liker_rows, n_users, 'liker_rows')
    thresh = torch.as_tensor(role_thresh, dtype=torch.int64).reshape(-1)
    assert thresh.numel() == m and (m == 0 or (0 <= int(thresh.min()) and int(thresh.max()) <= ROLE_ALWAYS_POSITIVE))
    thresh = torch.where(thresh >= 2 ** 31, thresh - 2 ** 32, thresh).to(torch.int32).to(V.device)     # the same 32 bits
    _fold_warn_wide('K10', 'item', k)
    Vn = torch.empty((m, k), dtype=torch.float32, device=V.device)
    bn = torch.empty(m, dtype=torch.float32, device=V.device)
    loss, trip = _fold_outputs(m, steps, triplets, 3, want_loss, want_triplets, V.device)
    if m:
        _call('tkr_bpr_foldin_items', V, _p(U), _p(V), _p(b), C.c_int32(n_users), C.c_int32(n_items), C.c_int32(k), _p(user_ptr), _p(user_cols),
              _p(liker_ptr), _p(liker_rows), _p(thresh), C.c_int32(m), _p(V0), _p(b0), C.c_float(li), C.c_float(lj), C.c_float(lb),
              C.c_float(lr), C.c_int32({'l2': 0, 'l1': 1}[mode]), C.c_int32(steps), C.c_int32(triplets), C.c_uint64(seed & 0xffffffffffffffff),
              C.c_uint64(first_row), _p(Vn), _p(bn), _p(loss), _p(trip))
    return (Vn, bn) + ((loss,) if want_loss else ()) + ((trip,) if want_triplets else ())


# ---- K11: the ratings parser on the device (csrc/parse_dev.hip) ------------------------------------------------------------------
PARSE_CHUNK_MIN, PARSE_CHUNK_MAX = 64, 1 << 20      # chunk_bytes: a power of two in this range


def idtable_build(blob, index):
    """-> int32 [n_slots, 4] host array: the open-addressing table of the len(index) '\\n'-separated tokens of `blob` (bytes) in the
    layout tkr_ratings_emit_dev probes (include/tkr.h); a host call"""
    import numpy as np
    n = int(index.shape[0])
    n_slots = int(lib().tkr_idtable_slots(C.c_int64(n)))
    if n_slots < 0:
        raise TkrError('tkr_idtable_slots failed: tkr error %d' % n_slots)
    slots = np.empty((n_slots, 4), dtype=np.int32)
    _check(lib().tkr_idtable_build(blob, C.c_int64(len(blob)), index.ctypes.data_as(C.c_void_p), C.c_int64(n),
                                   slots.ctypes.data_as(C.c_void_p), C.c_int64(n_slots)), 'tkr_idtable_build')
    return slots


def parse_dev_workspace_bytes(n_bytes, chunk_bytes):
    return _chunked_size('tkr_parse_dev_workspace_bytes', 'parse', n_bytes, chunk_bytes)


def ratings_count_dev(text, chunk_bytes, workspace, totals):
    """first half of K11: totals (device int64[2]) = (n_lines, n_entries) of the ratings text in `text` (device uint8)"""
    assert text.dtype == torch.uint8 and totals.dtype == torch.int64 and totals.numel() == 2 and workspace.dtype == torch.uint8
    _call('tkr_ratings_count_dev', workspace, _p(text), C.c_int64(text.numel()), C.c_int64(chunk_bytes), _p(workspace), C.c_int64(workspace.numel()),
          _p(totals))


def ratings_emit_dev(text, chunk_bytes, workspace, n_lines, n_entries, user_table, item_table, status):
    """second half of K11 -> (line_user, line_ptr, item, like) on text's device; *_table = (slots int32 [n_slots, 4], blob uint8,
    blob_len) on that device; status (device int64[1]) = -1 or the offset of a malformed field"""
    dev = workspace.device
    line_start = torch.empty(n_lines, dtype=torch.int64, device=dev)
    line_user = torch.empty(n_lines, dtype=torch.int32, device=dev)
    line_ptr = torch.empty(n_lines + 1, dtype=torch.int64, device=dev)
    item = torch.empty(n_entries, dtype=torch.int32, device=dev)
    like = torch.empty(n_entries, dtype=torch.int32, device=dev)
    (us, ub, ul), (vs, vb, vl) = user_table, item_table
    assert us.dtype == torch.int32 and vs.dtype == torch.int32 and ub.dtype == torch.uint8 and vb.dtype == torch.uint8 and status.dtype == torch.int64
    _call('tkr_ratings_emit_dev', workspace, _p(text), C.c_int64(text.numel()), C.c_int64(chunk_bytes), _p(workspace), C.c_int64(workspace.numel()),
          C.c_int64(n_lines), C.c_int64(n_entries), _p(us), C.c_int64(us.shape[0]), _p(ub), C.c_int64(ul), _p(vs), C.c_int64(vs.shape[0]), _p(vb),
          C.c_int64(vl), _p(line_start), _p(line_user), _p(line_ptr), _p(item), _p(like), _p(status))
    return line_user, line_ptr, item, like


# ---- K13: the text writers on the device (csrc/format_dev.hip) -------------------------------------------------------------------
def format_totals(totals, what):
    """what the host reads between the two calls, (size of the text, status) as a pair of ints -> the size; an index that names no token
    raises"""
    size, bad = (int(v) for v in totals)
    if bad != -1:
        raise TkrError('%s: row %d holds an index that names no token of its table' % (what, bad))
    return size


def _list_args(ids, scores, row_user, user_tokens, item_tokens):
    assert ids.dtype == torch.int32 and scores.dtype == torch.float32 and row_user.dtype == torch.int32
    assert ids.dim() == 2 and ids.shape == scores.shape and row_user.numel() == ids.shape[0]
    args = [_p(ids), _p(scores), _p(row_user), C.c_int64(ids.shape[0]), C.c_int32(ids.shape[1])]
    for blob, blob_len, start, length in (user_tokens, item_tokens):
        assert blob.dtype == torch.uint8 and start.dtype == torch.int64 and length.dtype == torch.int32 and start.numel() == length.numel()
        assert blob_len <= blob.numel()
        args += [_p(blob), C.c_int64(blob_len), _p(start), _p(length), C.c_int64(length.numel())]
    return args


def lists_format_sizes(ids, scores, row_user, user_tokens, item_tokens):
    """first half of K13 for the top-k lists -> (line_ptr int64 [n + 1], totals int64 [2]) on the device, nothing read back yet
    (format_totals(totals.tolist(), ...) is the round trip); *_tokens = (blob uint8, blob_len, start int64, length int32) on ids' device
    (textio.IdMap.device_tokens)"""
    n = int(ids.shape[0])
    line_ptr = torch.empty(n + 1, dtype=torch.int64, device=ids.device)
    totals = torch.empty(2, dtype=torch.int64, device=ids.device)
    _call('tkr_lists_format_sizes_dev', line_ptr, *_list_args(ids, scores, row_user, user_tokens, item_tokens), _p(line_ptr), _p(totals))
    return line_ptr, totals


def format_emit_check(status, what):
    """the status word of an emit call, read after the block's text has been used or downloaded"""
    bad = int(status.item())
    if bad != -1:
        raise TkrError('%s: line_ptr does not describe the text of row %d' % (what, bad))


def lists_format_emit(ids, scores, row_user, user_tokens, item_tokens, line_ptr, first_row, n_rows, out):
    """second half: rows [first_row, first_row + n_rows) of the text into `out` (device uint8, at least their bytes)"""
    assert out.dtype == torch.uint8 and line_ptr.dtype == torch.int64 and line_ptr.numel() == ids.shape[0] + 1
    status = torch.empty(1, dtype=torch.int64, device=ids.device)
    _call('tkr_lists_format_emit_dev', line_ptr, *_list_args(ids, scores, row_user, user_tokens, item_tokens), _p(line_ptr),
          C.c_int64(first_row), C.c_int64(n_rows), _p(out), C.c_int64(out.numel()), _p(status))
    return status


def matrix_format_sizes(data):
    """first half of K13 for a '%f ' matrix (fp32 [rows, cols] on the device) -> (line_ptr int64 [rows + 1], totals int64 [2])"""
    assert data.dtype == torch.float32 and data.dim() == 2
    line_ptr = torch.empty(data.shape[0] + 1, dtype=torch.int64, device=data.device)
    totals = torch.empty(2, dtype=torch.int64, device=data.device)
    _call('tkr_matrix_format_sizes_dev', line_ptr, _p(data) if data.numel() else C.c_void_p(0), C.c_int64(data.shape[0]), C.c_int64(data.shape[1]),
          _p(line_ptr), _p(totals))
    return line_ptr, totals


def matrix_format_emit(data, line_ptr, first_row, n_rows, out):
    assert out.dtype == torch.uint8 and line_ptr.dtype == torch.int64 and line_ptr.numel() == data.shape[0] + 1
    status = torch.empty(1, dtype=torch.int64, device=data.device)
    _call('tkr_matrix_format_emit_dev', line_ptr, _p(data) if data.numel() else C.c_void_p(0), C.c_int64(data.shape[0]), C.c_int64(data.shape[1]),
          _p(line_ptr), C.c_int64(first_row), C.c_int64(n_rows), _p(out), C.c_int64(out.numel()), _p(status))
    return status


# ---- K14: the matrix reader on the device (csrc/scan_dev.hip) --------------------------------------------------------------------
def scan_dev_workspace_bytes(n_bytes, chunk_bytes):
    return _chunked_size('tkr_scan_dev_workspace_bytes', 'read', n_bytes, chunk_bytes)


def matrix_count_dev(text, chunk_bytes, workspace, totals):
    """first half of K14: totals (device int64[3]) = (n_lines, n_tokens, layout status) of the matrix text in `text` (device uint8)"""
    assert text.dtype == torch.uint8 and totals.dtype == torch.int64 and totals.numel() == 3 and workspace.dtype == torch.uint8
    _call('tkr_matrix_count_dev', workspace, _p(text), C.c_int64(text.numel()), C.c_int64(chunk_bytes), _p(workspace), C.c_int64(workspace.numel()),
          _p(totals))


def matrix_emit_dev(text, chunk_bytes, workspace, n_lines, n_tokens, cols):
    """second half of K14 -> (tok_start int64 [n_tokens], data fp32 [n_tokens], hard int64 [(n_tokens + 63) // 64] (bit i & 63 of word
    i >> 6: token i is left to the host), counts int64 [2] = (layout status, n_hard)) on text's device, nothing read back yet"""
    dev = workspace.device
    tok_start = torch.empty(n_tokens, dtype=torch.int64, device=dev)
    data = torch.empty(n_tokens, dtype=torch.float32, device=dev)
    hard = torch.empty((n_tokens + 63) // 64, dtype=torch.int64, device=dev)
    counts = torch.empty(2, dtype=torch.int64, device=dev)
    _call('tkr_matrix_emit_dev', workspace, _p(text), C.c_int64(text.numel()), C.c_int64(chunk_bytes), _p(workspace), C.c_int64(workspace.numel()),
          C.c_int64(n_lines), C.c_int64(n_tokens), C.c_int64(cols), _p(tok_start), _p(data), _p(hard), _p(counts))
    return tok_start, data, hard, counts


def matrix_token_host(token: bytes):
    """the device's classify-and-convert routine of K14 run on the CPU -> the fp32 as 4 little-endian bytes, or None for a hard token"""
    out = C.c_float()
    rc = lib().tkr_matrix_token_host(token, C.c_int64(len(token)), C.byref(out))
    if rc < 0:
        raise TkrError('tkr_matrix_token_host failed: tkr error %d' % rc)
    return bytes(memoryview(out).cast('B')) if rc == 1 else None


def matrix_tokens_host(text, start):
    """the host reader's own check on the tokens of `text` (host uint8 array) that start at `start` (host int64 array) -> (rc, fp32
    array): rc -4 where tkr_matrix_read would refuse the file"""
    import numpy as np
    out = np.empty(len(start), dtype=np.float32)
    rc = lib().tkr_matrix_tokens_host(C.c_void_p(text.ctypes.data), C.c_int64(text.size), C.c_void_p(start.ctypes.data), C.c_int64(len(start)),
                                      C.c_void_p(out.ctypes.data))
    return rc, out


# ---- K15: parsed ratings -> CSR rows on the device (csrc/group_dev.hip) ----------------------------------------------------------
GROUP_WAVE_COLS = 32768      # TKR_GROUP_WAVE_COLS of include/tkr.h: up to here a wave builds a row, above it a workgroup
GROUP_MAX_COLS = 1308672     # TKR_GROUP_MAX_COLS: the bitmap of one row must fit the LDS of one workgroup
_GROUP_REFUSED = ('seg_of_row[%d] is outside [-1, n_seg)', 'seg_ptr decreases or leaves [0, len(item)] at segment / row %d',
                  'row %d holds an item >= n_cols', 'ptr does not describe the sources at row %d')


class DeviceGroupTooLarge(TkrError):
    """more columns than the bitmap of one row can hold in LDS (GROUP_MAX_COLS), or arrays that do not fit the free memory of the
    device ('auto' then groups on the host)"""


class GroupSource(C.Structure):
    """mirror of tkr_group_source (include/tkr.h)"""
    _fields_ = [('seg_ptr', C.c_void_p), ('item', C.c_void_p), ('like', C.c_void_p), ('seg_of_row', C.c_void_p), ('n_seg', C.c_int64),
                ('n_entries', C.c_int64)]


def group_segments(sources, n_rows, n_cols, like_only=False):
    """K15 -> (ptr int64 [n_rows + 1], cols int32 [ptr[-1]]) on the device: row r is the ascending, duplicate-free union of the counted
    items of its segments.  sources: one or two tuples (seg_ptr int64 [n_seg + 1], item int32, like int32 | None, seg_of_row int64
    [n_rows] | None) of device tensors; seg_of_row[r] is the segment that feeds row r, -1 none, None the identity.  An entry counts
    when item >= 0 and, with like_only, like == 1 (include/tkr.h).  Input the kernels refuse raises ValueError, more than
    GROUP_MAX_COLS columns DeviceGroupTooLarge"""
    what = 'group_segments'
    sources = list(sources)
    if not 1 <= len(sources) <= 2:
        raise ValueError('%s: one or two sources required, got %d' % (what, len(sources)))
    n_rows, n_cols = int(n_rows), int(n_cols)
    if n_rows < 0 or n_cols < 1:
        raise ValueError('%s: n_rows >= 0 and n_cols >= 1 required' % what)
    device = None
    structs = (GroupSource * len(sources))()
    for k, source in enumerate(sources):
        if not isinstance(source, (tuple, list)) or len(source) != 4:
            raise TypeError('%s: a source is (seg_ptr, item, like | None, seg_of_row | None)' % what)
        seg_ptr, item, like, seg_of_row = source
        _operand(what, 'seg_ptr', seg_ptr, torch.int64, 1, at_least=1, on=device, raises=_STD)      # n_seg + 1 entries
        device = seg_ptr.device
        _operand(what, 'item', item, torch.int32, 1, on=device, raises=_STD)
        _operand(what, 'like', like, torch.int32, 1, on=device, optional=True, raises=_STD)
        _operand(what, 'seg_of_row', seg_of_row, torch.int64, 1, on=device, optional=True, raises=_STD)
        n_seg, n_entries = int(seg_ptr.numel()) - 1, int(item.numel())
        if like is None and like_only:
            raise ValueError('%s: like_only needs the like array of every source' % what)
        if like is not None and like.numel() != n_entries:
            raise ValueError('%s: item and like must have one length' % what)
        if seg_of_row is None and n_seg < n_rows:
            raise ValueError('%s: without seg_of_row a source needs a segment per row (%d < %d)' % (what, n_seg, n_rows))
        if seg_of_row is not None and seg_of_row.numel() != n_rows:
            raise ValueError('%s: seg_of_row must hold n_rows = %d entries' % (what, n_rows))
        structs[k] = GroupSource(seg_ptr.data_ptr(), item.data_ptr() if n_entries else None, like.data_ptr() if like is not None and n_entries else None,
                                 seg_of_row.data_ptr() if seg_of_row is not None and n_rows else None, n_seg, n_entries)
    if n_cols > GROUP_MAX_COLS:
        raise DeviceGroupTooLarge('%s: %d columns, the bitmap of a row holds at most %d' % (what, n_cols, GROUP_MAX_COLS))
    ptr = torch.zeros(n_rows + 1, dtype=torch.int64, device=device)
    if n_rows == 0:
        return ptr, torch.empty(0, dtype=torch.int32, device=device)
    totals = torch.empty(2, dtype=torch.int64, device=device)
    args = (C.byref(structs), C.c_int32(len(sources)), C.c_int64(n_rows), C.c_int32(n_cols), C.c_int32(1 if like_only else 0))
    _call('tkr_group_count_dev', ptr, *args, _p(ptr), _p(totals))
    total, word = totals.tolist()                                   # the one round trip: cols is sized by it
    status_check(what, _GROUP_REFUSED, ValueError, word)
    cols = torch.empty(total, dtype=torch.int32, device=device)
    status = torch.empty(1, dtype=torch.int64, device=device)
    _call('tkr_group_emit_dev', ptr, *args, _p(ptr), _p(cols) if total else C.c_void_p(0), C.c_int64(total), _p(status))
    status_check(what, _GROUP_REFUSED, ValueError, int(status.item()))
    return ptr, cols


def last_line_of_user(line_user, n_users):
    """-> int64 [n_users] on the device: the last line of every user in line_user (int32 [n_lines], -1 = unknown user), -1 = no line"""
    what = 'last_line_of_user'
    _operand(what, 'line_user', line_user, torch.int32, 1, raises=_STD)
    n_users = int(n_users)
    if n_users < 0:
        raise ValueError('%s: n_users >= 0 required' % what)
    last = torch.full((n_users,), -1, dtype=torch.int64, device=line_user.device)
    if n_users and line_user.numel():
        _call('tkr_last_line_of_user_dev', line_user, _p(line_user), C.c_int64(line_user.numel()), C.c_int64(n_users), _p(last))
    return last


def scenario_lines(ptr):
    """the rows of the CSR `ptr` (device int64 [n_rows + 1]) with at least one element -> (rows int64 [n_kept], ascending; the ptr
    int64 [n_kept + 1] of the CSR that keeps only them -- its cols are the same array)"""
    what = 'scenario_lines'
    _operand(what, 'ptr', ptr, torch.int64, 1, at_least=1, raises=_STD)      # n_rows + 1 entries
    n_rows = int(ptr.numel()) - 1
    dev = ptr.device
    if n_rows == 0:
        return torch.empty(0, dtype=torch.int64, device=dev), ptr.clone()
    pos = torch.empty(n_rows + 1, dtype=torch.int64, device=dev)
    _call('tkr_compact_rows_count_dev', ptr, _p(ptr), C.c_int64(n_rows), _p(pos))
    n_kept = int(pos[-1].item())                                    # the one round trip
    rows = torch.empty(n_kept, dtype=torch.int64, device=dev)
    out_ptr = torch.empty(n_kept + 1, dtype=torch.int64, device=dev)
    status = torch.empty(1, dtype=torch.int64, device=dev)
    _call('tkr_compact_rows_emit_dev', ptr, _p(ptr), _p(pos), C.c_int64(n_rows), C.c_int64(n_kept), _p(rows) if n_kept else C.c_void_p(0),
          _p(out_ptr), _p(status))
    status_check(what, _GROUP_REFUSED, ValueError, int(status.item()))
    return rows, out_ptr


# ---- K16: the weights of a linear fusion of several models (csrc/fusion.hip) -------------------------------------------------------
FUSION_MAX_MODELS = 16       # TKR_FUSION_MAX_MODELS of include/tkr.h


class FusionModel(C.Structure):
    """mirror of tkr_fusion_model (include/tkr.h)"""
    _fields_ = [('U', C.c_void_p), ('V', C.c_void_p), ('bias', C.c_void_p), ('k', C.c_int32), ('reserved', C.c_int32)]


class FusionModels(C.Structure):
    """mirror of tkr_fusion_models (include/tkr.h)"""
    _fields_ = [('m', FusionModel * FUSION_MAX_MODELS), ('n_models', C.c_int32), ('n_users', C.c_int32), ('n_items', C.c_int32),
                ('reserved', C.c_int32)]


def fusion_models(what, models):
    """a list of (U [n_users, k_m], V [n_items, k_m], bias [n_items] | [n_items, 1] | None) -> (FusionModels, n_users, n_items, device).
    Refuses with TkrError, the tensors' properties first (no device access): more than FUSION_MAX_MODELS models, a table that is not
    fp32 or not contiguous, row counts or widths that do not match, tensors that are not on one GPU."""
    models = list(models)
    if not 1 <= len(models) <= FUSION_MAX_MODELS:
        raise TkrError('%s: 1 .. %d models required, got %d' % (what, FUSION_MAX_MODELS, len(models)))
    st = FusionModels()
    n_users = n_items = None
    for m, model in enumerate(models):
        if not isinstance(model, (tuple, list)) or len(model) != 3:
            raise TkrError('%s: a model is (U, V, bias | None)' % what)
        U, V, b = model
        _operand(what, 'U of model %d' % m, U, torch.float32, 2, on=_LATER)
        _operand(what, 'V of model %d' % m, V, torch.float32, 2, on=_LATER)
        _operand(what, 'bias of model %d' % m, b, torch.float32, on=_LATER, optional=True)
        if U.shape[1] != V.shape[1] or U.shape[1] < 1:
            raise TkrError('%s: U and V of model %d must share k >= 1 (%d, %d)' % (what, m, U.shape[1], V.shape[1]))
        if n_users is None:
            n_users, n_items = int(U.shape[0]), int(V.shape[0])
        if int(U.shape[0]) != n_users or int(V.shape[0]) != n_items or n_users < 1 or n_items < 1:
            raise TkrError('%s: model %d has %d user and %d item rows, model 0 has %d and %d' % (what, m, U.shape[0], V.shape[0], n_users, n_items))
        if b is not None and b.numel() != n_items:
            raise TkrError('%s: the bias of model %d must hold one value per item' % (what, m))
    device = models[0][0].device
    for m, (U, V, b) in enumerate(models):
        for name, t in (('U', U), ('V', V), ('bias', b)):
            if t is not None:
                _on_gpu(what, '%s of model %d' % (name, m), t, device)
        st.m[m] = FusionModel(U.data_ptr(), V.data_ptr(), b.data_ptr() if b is not None else None, int(U.shape[1]), 0)
    st.n_models, st.n_users, st.n_items = len(models), n_users, n_items
    return st, n_users, n_items, device


def fusion_features(models, csr, n_items, seed, first_triplet, count, want_triplets=False):
    """K16 -> D fp32 [count, M] on the device (with want_triplets also int32 [count, 3]): triplet first_triplet + t of K1's stream
    under `seed` on the training CSR `csr` (tr_users, row_ptr, pos_cols, cols_sorted: single/_engine.py TrainingCSR),
    D[t, m] = fl(s_m(u, i) - s_m(u, j)) on the score bits of rank_candidates (include/tkr.h tkr_fusion_features)"""
    what = 'fusion_features'
    st, n_users, n_items_m, device = fusion_models(what, models)
    count = int(count)
    if int(n_items) != n_items_m:
        raise TkrError('%s: n_items = %d, the models have %d item rows' % (what, n_items, n_items_m))
    if count < 1:
        raise TkrError('%s: count >= 1 required' % what)
    for name in ('tr_users', 'row_ptr', 'pos_cols', 'cols_sorted'):
        _operand(what, name, getattr(csr, name), torch.int32, 1, on=device)
    if csr.row_ptr.numel() != n_users + 1 or csr.tr_users.numel() < 1:
        raise TkrError('%s: the CSR must describe the models\' %d users and hold at least one row' % (what, n_users))
    M = st.n_models
    D = torch.empty((count, M), dtype=torch.float32, device=device)
    trip = torch.empty((count, 3), dtype=torch.int32, device=device) if want_triplets else None
    _call('tkr_fusion_features', D, C.byref(st), _p(csr.tr_users), C.c_int32(csr.tr_users.numel()), _p(csr.row_ptr), _p(csr.pos_cols),
          _p(csr.cols_sorted), C.c_int32(n_items), C.c_uint64(int(seed) & 0xFFFFFFFFFFFFFFFF), C.c_uint64(int(first_triplet)),
          C.c_int64(count), _p(D), _p(trip))
    return (D, trip) if want_triplets else D


def fusion_sgd(D, batch, n_batches, lr, lambda_w, W, want_loss=False):
    """K16: n_batches steps of ranking_fusion.py:48-54 on the rows of D [n_rows, M], batch after batch from row 0; W fp32 [M] is
    updated in place -> W (with want_loss: (W, loss fp32 [n_batches])).  One workgroup, bitwise repeatable, and the same bits whether
    the batches run in one call or in several with W carried across (include/tkr.h tkr_fusion_sgd)"""
    what = 'fusion_sgd'
    _operand(what, 'D', D, torch.float32, 2, on=_LATER)
    _operand(what, 'W', W, torch.float32, 1, on=_LATER)
    n_rows, M = int(D.shape[0]), int(D.shape[1])
    batch, n_batches = int(batch), int(n_batches)
    if not 1 <= M <= FUSION_MAX_MODELS:
        raise TkrError('%s: 1 .. %d models required, D has %d columns' % (what, FUSION_MAX_MODELS, M))
    if batch < 1:
        raise TkrError('%s: batch >= 1 required, got %d' % (what, batch))
    if W.numel() != M:
        raise TkrError('%s: W must hold one weight per column of D (%d, %d)' % (what, W.numel(), M))
    if n_batches < 0 or n_batches * batch > n_rows:
        raise TkrError('%s: %d batches of %d rows do not fit the %d rows of D' % (what, n_batches, batch, n_rows))
    _on_gpu(what, 'D', D)
    _on_gpu(what, 'W', W, D.device)
    loss =torch.empty(n_batches, dtype=torch.float32, device=D.device) if want_loss else None
    if n_batches:
        _call('tkr_fusion_sgd', D, _p(D), C.c_int64(n_rows), C.c_int32(M), C.c_int32(batch), C.c_int64(n_batches), C.c_float(lr),
              C.c_float(lambda_w), _p(W), _p(loss))
    return (W, loss) if want_loss else W


def fusion_user_weights(models, like_ptr, like_cols):
    """K16 -> (rmse fp32 [n_users, M], w fp32 [n_users, M]) on the device: efusion.py:57-82 on the CSR of the users' training likes
    (like_ptr int64 [n_users + 1] from 0, like_cols int32, a set per row: foldin.liked_csr) -- include/tkr.h tkr_fusion_user_weights"""
    what = 'fusion_user_weights'
    st, n_users, n_items, device = fusion_models(what, models)
    _operand(what, 'like_ptr', like_ptr, torch.int64, 1, on=device)
    _operand(what, 'like_cols', like_cols, torch.int32, 1, on=device)
    if like_ptr.numel() != n_users + 1:
        raise TkrError('%s: like_ptr must hold n_users + 1 = %d entries' % (what, n_users + 1))
    nnz = int(like_cols.numel())
    if not (int(like_ptr[0]) == 0 and int(like_ptr[-1]) == nnz and bool((like_ptr[1:] >= like_ptr[:-1]).all())):
        raise TkrError('%s: like_ptr must run from 0 to len(like_cols) = %d and never decrease' % (what, nnz))
    if nnz == 0:
        like_cols = torch.zeros(1, dtype=torch.int32, device=device)      # never read: every row is empty
    M = st.n_models
    rmse = torch.empty((n_users, M), dtype=torch.float32, device=device)
    w = torch.empty((n_users, M), dtype=torch.float32, device=device)
    _call('tkr_fusion_user_weights', rmse, C.byref(st), _p(like_ptr), _p(like_cols), C.c_int32(n_users), _p(rmse), _p(w))
    return rmse, w


# ---- K23: the sums of one Newton pass of the SVM fusion (csrc/fusion_svm.hip) ------------------------------------------------------
FUSION_SVM_SLAB = 4096       # TKR_FUSION_SVM_SLAB of include/tkr.h


def fusion_svm_words(M):
    """the eight-byte words of one slab's partial and of the result: S (upper triangle) | r | q | count"""
    return (M + 1) * (M + 2) // 2 + M + 3


def fusion_svm_slabs(n_rows, first_row=0):
    """the slabs that the rows [first_row, first_row + n_rows) touch: slabs are cut at multiples of FUSION_SVM_SLAB"""
    return (first_row + n_rows - 1) // FUSION_SVM_SLAB - first_row // FUSION_SVM_SLAB + 1


def fusion_svm_partial_bytes(n_rows, M, first_row=0):
    return _size('tkr_fusion_svm_partial_bytes', (C.c_int64, C.c_int32, C.c_int64), (n_rows, M, first_row))


def fusion_svm_unpack(out, M):
    """the result of fusion_svm_sums on the host (numpy fp64 [fusion_svm_words(M)]) -> (S fp64 [M + 1, M + 1] symmetric, r fp64 [M + 1],
    q, count)"""
    import numpy as np
    out = np.ascontiguousarray(out, dtype=np.float64)
    X = M + 1
    nS = X * (X + 1) // 2
    S = np.zeros((X, X), dtype=np.float64)
    S[np.triu_indices(X)] = out[:nS]
    S = S + np.triu(S, 1).T
    return S, out[nS:nS + X].copy(), float(out[nS + X]), int(out[nS + X + 1:nS + X + 2].view(np.int64)[0])


def fusion_svm_sums(D, W, first_row=0, *, partial=None, slab_offset=0, reduce=True, out=None, status=None, check=True):
    """K23 -> out, device fp64 [fusion_svm_words(M)] (fusion_svm_unpack reads it): over the active rows of D fp32 [n_rows, M] under
    W fp64 [M + 1] (weights, then intercept) the sums S, r, q and the count of include/tkr.h tkr_fusion_svm_sums; row t of D is row
    first_row + t of the run.  A run cut into calls of whole slabs shares ``partial`` (fusion_svm_partial_bytes of the whole run),
    carries ``slab_offset`` and reduces in its last call only (reduce=False before it: None is returned); the status word is set by the
    call with slab_offset 0.  A row that is not finite raises TkrError naming it and leaves ``out`` as it is; check=False reads
    nothing back (the caller reads ``status``: -1 or the row)."""
    what = 'fusion_svm_sums'
    _operand(what, 'D', D, torch.float32, 2, on=_LATER)
    n_rows, M = int(D.shape[0]), int(D.shape[1])
    first_row, slab_offset = int(first_row), int(slab_offset)
    if not 1 <= M <= FUSION_MAX_MODELS:
        raise TkrError('%s: 1 .. %d models required, D has %d columns' % (what, FUSION_MAX_MODELS, M))
    if n_rows < 1:
        raise TkrError('%s: D must hold at least one row' % what)
    if first_row < 0 or slab_offset < 0:
        raise TkrError('%s: first_row and slab_offset must not be negative (%d, %d)' % (what, first_row, slab_offset))
    _on_gpu(what, 'D', D)
    words = fusion_svm_words(M)
    _operand(what, 'W', W, torch.float64, numel=M + 1, on=D.device)
    need = (slab_offset + fusion_svm_slabs(n_rows, first_row)) * words
    if partial is None:
        partial = torch.empty(need, dtype=torch.float64, device=D.device)
    _operand(what, 'partial', partial, torch.float64, at_least=need, on=D.device)
    if reduce:
        if out is None:
            out = torch.empty(words, dtype=torch.float64, device=D.device)
        _operand(what, 'out', out, torch.float64, numel=words, on=D.device)
    else:
        out = None
    if status is None:
        status = torch.empty(1, dtype=torch.int64, device=D.device)
    if status.dtype != torch.int64 or status.numel() != 1 or not status.is_contiguous() or status.device != D.device:
        raise TkrError('%s: status must be one torch.int64 word on the GPU that holds D' % what)
    _call('tkr_fusion_svm_sums', D, _p(D), C.c_int64(n_rows), C.c_int32(M), C.c_int64(first_row), _p(W), _p(partial),
          C.c_int64(partial.numel() * 8), C.c_int64(slab_offset), _p(out), _p(status))
    if check and reduce:
        fusion_svm_check(int(status.item()))
    return out


def fusion_svm_check(word):
    """the status word of a run of fusion_svm_sums, read on the host"""
    if word != -1:
        raise TkrError('fusion_svm_sums: row %d of the features holds a value that is not finite (fusion_features writes NaN for an id '
                       'outside the tables); nothing was summed' % word)


# ---- K17: diversify a pool into a list, the pair sums of list diversity (csrc/diversity.hip) -------------------------------------------
MMR_MAX_POOL = 1024          # TKR_MMR_MAX_POOL of include/tkr.h: a thread per pool entry
_DIV_REFUSED = (None, 'row %d holds an id outside [0, n_items) in front of its padding')


def _div_args(what, S, ids, rel=None):
    """refuse what the K17 entry points cannot take, the tensors' properties only (no device access) -> (n_items, k, n_rows, width)"""
    named = [('S', S, torch.float32), ('ids', ids, torch.int32)] + ([] if rel is None else [('rel', rel, torch.float32)])
    for name, t, dtype in named:
        _operand(what, name, t, dtype, 2, on=_LATER)
    for name, t, _ in named:
        _on_gpu(what, name, t, S.device)
    if S.shape[0] < 1 or S.shape[1] < 1:
        raise TkrError('%s: S [n_items, k] needs n_items >= 1 and k >= 1' % what)
    if rel is not None and rel.shape != ids.shape:
        raise TkrError('%s: ids and rel must have one shape' % what)
    if ids.shape[1] > MMR_MAX_POOL:
        raise TkrError('%s: %d entries per row, at most %d are supported' % (what, ids.shape[1], MMR_MAX_POOL))
    return int(S.shape[0]), int(S.shape[1]), int(ids.shape[0]), int(ids.shape[1])


def mmr_select(S, ids, rel, lam, t):
    """K17 -> sel_pos int32 [n_rows, t] on the device: greedy Maximal Marginal Relevance over the pool `ids` (int32 [n_rows, N], valid up
    to the first negative id) with relevance `rel` (fp32 [n_rows, N]) and similarity chain(S[a], S[b]) -- the pool positions in pick
    order, -1 where a row has fewer than t valid entries (include/tkr.h tkr_mmr_select).  An id >= n_items raises TkrError"""
    what = 'mmr_select'
    n_items, k, n_rows, N = _div_args(what, S, ids, rel)
    lam, t = float(lam), int(t)
    if not 0.0 <= lam <= 1.0:                                        # (a NaN fails both comparisons)
        raise TkrError('%s: lambda must lie in [0, 1], got %r' % (what, lam))
    if not 1 <= t <= N:
        raise TkrError('%s: 1 <= t <= N = %d required, got %d' % (what, N, t))
    sel = torch.empty((n_rows, t), dtype=torch.int32, device=S.device)
    if n_rows == 0:
        return sel
    status = torch.empty(1, dtype=torch.int64, device=S.device)
    _call('tkr_mmr_select', S, _p(S), C.c_int32(n_items), C.c_int32(k), _p(ids), _p(rel), C.c_int32(n_rows), C.c_int32(N), C.c_double(lam),
          C.c_int32(t), _p(sel), _p(status))
    status_check(what, _DIV_REFUSED, TkrError, int(status.item()))
    return sel


def list_pair_sums(S, ids):
    """K17 -> pair_sum float64 [n_rows, t] on the device: pair_sum[r, b] = sum over a < b of 1 - chain(S[ids[r, a]], S[ids[r, b]]) inside
    the valid prefix of row r (up to the first negative id), 0 behind it (include/tkr.h tkr_list_pair_sums)"""
    what = 'list_pair_sums'
    n_items, k, n_rows, t = _div_args(what, S, ids)
    out = torch.zeros((n_rows, t), dtype=torch.float64, device=S.device)
    if n_rows == 0 or t == 0:
        return out
    status = torch.empty(1, dtype=torch.int64, device=S.device)
    _call('tkr_list_pair_sums', S, _p(S), C.c_int32(n_items), C.c_int32(k), _p(ids), C.c_int32(n_rows), C.c_int32(t), _p(out), _p(status))
    status_check(what, _DIV_REFUSED, TkrError, int(status.item()))
    return out


# ---- K19: the nearest anchors of every list entry (csrc/explain.hip) ---------------------------------------------------------------------
ANCHOR_MAX_E = 8             # TKR_ANCHOR_MAX_E of include/tkr.h: the best anchors kept per entry
ANCHOR_MAX_T = MMR_MAX_POOL  # TKR_ANCHOR_MAX_T
_ANCHOR_REFUSED = ('row %d holds an id outside [0, n_items) in front of its padding', 'row %d holds an anchor outside [0, n_items)', None,
                   'anchor_ptr does not start at 0, decreases or leaves [0, len(anchor_cols)] at row %d')
_ANCHOR_RAISES = (TkrError, TkrError, None, ValueError)          # by kind: a bad row pointer is a ValueError, as a bad argument is


def nearest_anchors(S, ids, anchor_ptr, anchor_cols, e):
    """K19 -> (pos int32 [n_rows, t, e], sim fp32 [n_rows, t, e]) on the device: for every entry of the lists `ids` (int32 [n_rows, t],
    valid up to the first negative id) the e anchors of its row -- anchor_cols[anchor_ptr[r] : anchor_ptr[r + 1]], int64 / int32, any
    order, repeats allowed -- that are most similar to it under chain(S[a], S[b]) and are not the entry's own item: their positions
    from the row's start, best first, ties to the lower position, and the similarities; -1 / -inf where fewer than e exist and behind
    a row's end (include/tkr.h tkr_nearest_anchors).  An id or an anchor outside the table raises TkrError, a bad anchor_ptr ValueError"""
    what = 'nearest_anchors'
    n_items, k, n_rows, t = _div_args(what, S, ids)
    e = int(e)
    if not 1 <= e <= ANCHOR_MAX_E:
        raise TkrError('%s: 1 <= e <= %d required, got %d' % (what, ANCHOR_MAX_E, e))
    if t < 1:
        raise TkrError('%s: ids [n_rows, t] needs t >= 1' % what)
    _operand(what, 'anchor_ptr', anchor_ptr, torch.int64, 1, on=S.device, raises=_STD)
    _operand(what, 'anchor_cols', anchor_cols, torch.int32, 1, on=S.device, raises=_STD)
    if anchor_ptr.numel() != n_rows + 1:
        raise ValueError('%s: anchor_ptr must hold n_rows + 1 = %d entries, not %d' % (what, n_rows + 1, anchor_ptr.numel()))
    pos = torch.empty((n_rows, t, e), dtype=torch.int32, device=S.device)
    sim = torch.empty((n_rows, t, e), dtype=torch.float32, device=S.device)
    if n_rows == 0:
        return pos, sim
    n_anchors = int(anchor_cols.numel())
    status = torch.empty(1, dtype=torch.int64, device=S.device)
    _call('tkr_nearest_anchors', S, _p(S), C.c_int32(n_items), C.c_int32(k), _p(ids), C.c_int32(n_rows), C.c_int32(t), _p(anchor_ptr),
          _p(anchor_cols) if n_anchors else C.c_void_p(0), C.c_int64(n_anchors), C.c_int32(e), _p(pos), _p(sim), _p(status))
    status_check(what, _ANCHOR_REFUSED, _ANCHOR_RAISES, int(status.item()))
    return pos, sim


# ---- K20: the two halves of an ALS step (csrc/als.hip) -------------------------------------------------------------------------------------
ALS_MAX_K = 128              # TKR_ALS_MAX_K of include/tkr.h: A (k x k) lives in the LDS of one workgroup
ALS_GRAM_SLAB = 1024         # TKR_ALS_GRAM_SLAB: the listed rows one workgroup sums
ALS_NO_HEAVY = 1 << 62       # heavy_from: no row is heavy
_ALS_REFUSED = (None, 'row %d holds a like outside [0, n_y) (kind 1)', 'the system of row %d is not positive definite in fp32 (kind 2)',
                'like_ptr does not start at 0, decreases or leaves [0, len(like_cols)] at row %d (kind 3)')


class AlsRefused(TkrError):
    """a status word of K20 that is not -1; .word, .row and .kind say what it holds (include/tkr.h; raised by status_check)"""


def _als_table(what, name, t, k_max, k=None):
    """the shape rules of a factor table of the ALS family -> (rows, k)"""
    _operand(what, name, t, torch.float32, 2)
    if t.shape[0] < 1 or (k is not None and t.shape[1] != k):
        raise TkrError('%s: %s has shape %s' % (what, name, tuple(t.shape)))
    if not 1 <= t.shape[1] <= k_max:
        raise ValueError('%s: k = %d, 1 <= k <= %d is supported' % (what, t.shape[1], k_max))
    return int(t.shape[0]), int(t.shape[1])


def als_workspace_bytes(n_x, k, n_slabs):
    return _size('tkr_als_workspace_bytes', (C.c_int64, C.c_int32, C.c_int64), (n_x, k, n_slabs))


def als_heavy_slabs(like_ptr, heavy_from):
    """the slabs the heavy rows of a like CSR have together (like_ptr: a host array or a tensor)"""
    import numpy as np
    m = np.diff(like_ptr.cpu().numpy() if isinstance(like_ptr, torch.Tensor) else np.asarray(like_ptr, dtype=np.int64))
    m = m[(m >= heavy_from) & (m > 0)]
    return int(((m + ALS_GRAM_SLAB - 1) // ALS_GRAM_SLAB).sum())


def workspace_room(workspace, need, device):
    """-> `workspace` where it holds `need` bytes on `device`, else a new one that does: the one grower of the ALS and MLP workspaces
    (here, als.Work and als.MLP keep what it returns)"""
    if workspace is not None and workspace.numel() * workspace.element_size() >= need and workspace.device == device:
        return workspace
    return torch.empty((max(need, 16) + 7) // 8, dtype=torch.int64, device=device)


def _als_gram(what, entry, k_max, sizer, Y, rows, scale, ridge, workspace, out, check):
    n, k = _als_table(what, 'Y', Y, k_max)
    if rows is not None:
        _operand(what, 'rows', rows, torch.int32, 1, on=Y.device, raises=_STD)
    n_listed = n if rows is None else int(rows.numel())
    workspace = workspace_room(workspace, sizer(k, (n_listed + ALS_GRAM_SLAB - 1) // ALS_GRAM_SLAB), Y.device)
    G = torch.empty((k, k), dtype=torch.float32, device=Y.device) if out is None else out
    status = torch.empty(1, dtype=torch.int64, device=Y.device)
    # (an empty list is still a list: its tensor may have no address, so any that is not null stands in for it)
    rows_p = C.c_void_p(0) if rows is None else _p(rows if n_listed else Y)
    _call(entry, Y, _p(Y), C.c_int32(n), C.c_int32(k), rows_p, C.c_int64(n_listed), C.c_double(scale), C.c_double(ridge), _p(G), _p(workspace),
          C.c_int64(workspace.numel() * workspace.element_size()), _p(status))
    return _done(what, G, status, check, _ALS_REFUSED, AlsRefused)


def als_gram(Y, rows=None, scale=1.0, ridge=0.0, workspace=None, out=None, check=True):
    """K20 -> G fp32 [k, k] on the device: scale * sum over the listed rows (int32 tensor; None: all) of y y^T + ridge I
    (include/tkr.h tkr_als_gram).  A listed row outside [0, n) raises AlsRefused (after G is written without it); check=False
    returns (G, status tensor) and reads nothing back"""
    return _als_gram('als_gram', 'tkr_als_gram', ALS_MAX_K, lambda k, n_slabs: als_workspace_bytes(0, k, n_slabs), Y, rows, scale, ridge,
                     workspace, out, check)


def _als_rows(what, k_max, Y, G, like_ptr, like_cols, X, priors=None):
    """what the three row solvers check alike -> (n_y, k, n_x, n_likes).  priors: None where the call takes no prior, else the list of
    those handed in (none or one)"""
    n_y, k = _als_table(what, 'Y', Y, k_max)
    n_x, _ = _als_table(what, 'X', X, k_max, k)
    _als_table(what, 'G', G, k_max, k)
    for prior in priors or ():
        _als_table(what, 'prior', prior, k_max, k)
    if G.shape[0] != k or X.device != Y.device or G.device != Y.device or any(p.device != Y.device or p.shape[0] != n_x for p in priors or ()):
        raise TkrError('%s: G must be [k, k], %s on one GPU' % (what, 'and Y, G and X' if priors is None else 'prior [n_x, k], and Y, G, X and prior'))
    _operand(what, 'like_ptr', like_ptr, torch.int64, 1, on=Y.device, raises=_STD)
    _operand(what, 'like_cols', like_cols, torch.int32, 1, on=Y.device, raises=_STD)
    if like_ptr.numel() != n_x + 1:
        raise ValueError('%s: like_ptr must hold n_x + 1 = %d entries, not %d' % (what, n_x + 1, like_ptr.numel()))
    return n_y, k, n_x, int(like_cols.numel())


def als_solve_rows(Y, G, like_ptr, like_cols, X, *, w_like, w_rhs, ridge, heavy_from=None, want_loss=False, workspace=None, heavy_slabs=None,
                   check=True):
    """K20, in place on X fp32 [n_x, k]: X[r] = (G + w_like sum y y^T + ridge I)^-1 (w_rhs sum y) over row r's likes, rows of Y; rows
    without likes are left as they are (include/tkr.h tkr_als_solve_rows).  -> row_loss float64 [n_x] with want_loss, else None.
    heavy_from: None = ALS_HEAVY_FROM; heavy_slabs: what als_heavy_slabs gives for this CSR (computed when it is not handed in).
    A refusal raises AlsRefused naming row and kind; check=False returns (row_loss, status tensor) instead and reads nothing back"""
    what = 'als_solve_rows'
    n_y, k, n_x, n_likes = _als_rows(what, ALS_MAX_K, Y, G, like_ptr, like_cols, X)
    heavy_from = ALS_HEAVY_FROM if heavy_from is None else int(heavy_from)
    need = 0
    if heavy_from <= n_likes:
        need = als_workspace_bytes(n_x, k, als_heavy_slabs(like_ptr, heavy_from) if heavy_slabs is None else heavy_slabs)
    workspace = workspace_room(workspace, need, Y.device)
    loss = torch.empty(n_x, dtype=torch.float64, device=Y.device) if want_loss else None
    status = torch.empty(1, dtype=torch.int64, device=Y.device)
    _call('tkr_als_solve_rows', Y, _p(Y), C.c_int32(n_y), C.c_int32(k), _p(G), _p(like_ptr), _p(like_cols) if n_likes else C.c_void_p(0),
          C.c_int64(n_likes), C.c_int64(n_x), C.c_double(w_like), C.c_double(w_rhs), C.c_double(ridge), C.c_int64(heavy_from), _p(X), _p(loss),
          _p(workspace), C.c_int64(workspace.numel() * workspace.element_size()), _p(status))
    return _done(what, loss, status, check, _ALS_REFUSED, AlsRefused)


def als_prior_workspace_bytes(n_x, k, n_slabs):
    return _size('tkr_als_prior_workspace_bytes', (C.c_int64, C.c_int32, C.c_int64), (n_x, k, n_slabs))


def als_solve_rows_prior(Y, G, like_ptr, like_cols, X, prior, *, w_like, w_rhs, w_prior, ridge, heavy_from=None, want_loss=False, workspace=None,
                         heavy_slabs=None, check=True):
    """K21, in place on X fp32 [n_x, k]: als_solve_rows with w_prior * prior[r] added to row r's right-hand side and 1/2 w_prior
    |x - prior[r]|^2 to its loss, and the rows WITHOUT likes solved too: X[r] = (G + ridge I)^-1 (w_prior prior[r]), against one factor
    computed once per call (include/tkr.h tkr_als_solve_rows_prior).  prior: fp32 [n_x, k] on X's device.  The other arguments, the
    result, AlsRefused and check=False as als_solve_rows"""
    what = 'als_solve_rows_prior'
    n_y, k, n_x, n_likes = _als_rows(what, ALS_MAX_K, Y, G, like_ptr, like_cols, X, [prior])
    heavy_from = ALS_HEAVY_FROM if heavy_from is None else int(heavy_from)
    slabs = 0
    if heavy_from <= n_likes:
        slabs = als_heavy_slabs(like_ptr, heavy_from) if heavy_slabs is None else heavy_slabs
    need = als_prior_workspace_bytes(n_x if heavy_from <= n_likes else 0, k, slabs)
    workspace = workspace_room(workspace, need, Y.device)
    loss = torch.empty(n_x, dtype=torch.float64, device=Y.device) if want_loss else None
    status = torch.empty(1, dtype=torch.int64, device=Y.device)
    _call('tkr_als_solve_rows_prior', Y, _p(Y), C.c_int32(n_y), C.c_int32(k), _p(G), _p(like_ptr), _p(like_cols) if n_likes else C.c_void_p(0),
          C.c_int64(n_likes), C.c_int64(n_x), C.c_double(w_like), C.c_double(w_rhs), C.c_double(ridge), C.c_int64(heavy_from), _p(X), _p(loss),
          _p(prior), C.c_double(w_prior), _p(workspace), C.c_int64(workspace.numel() * workspace.element_size()), _p(status))
    return _done(what, loss, status, check, _ALS_REFUSED, AlsRefused)


ALS_HEAVY_FROM = 4 * ALS_GRAM_SLAB       # a row with this many likes is shared by several workgroups (scripts/time_als.py)


# ---- K24: the half-step by conjugate gradients (csrc/als_cg.hip), the Gram at any width up to 512 (csrc/als.hip) ---------------------------
ALS_CG_MAX_K = 512           # TKR_ALS_CG_MAX_K of include/tkr.h: a row's x and r are 8 registers per lane each
ALS_CG_STEPS = 3             # the steps per half-step als.py takes by default


class AlsCgRefused(AlsRefused):
    """a status word of K24 that is not -1 (the kinds of K20; kind 2 is conjugate gradients' own)"""


_ALS_CG_REFUSED = (None, _ALS_REFUSED[1], 'p.q of row %d is not positive and finite, or its solution is not finite (kind 2)', _ALS_REFUSED[3])


def als_cg_workspace_bytes(n_x, k):
    return _size('tkr_als_cg_workspace_bytes', (C.c_int64, C.c_int32), (n_x, k))


def als_gram_wide_workspace_bytes(k, n_slabs):
    return _size('tkr_als_gram_wide_workspace_bytes', (C.c_int32, C.c_int64), (k, n_slabs))


def als_gram_wide(Y, rows=None, scale=1.0, ridge=0.0, workspace=None, out=None, check=True):
    """K24 -> G fp32 [k, k]: als_gram's definition, arguments and result for 1 <= k <= ALS_CG_MAX_K (include/tkr.h tkr_als_gram_wide)"""
    return _als_gram('als_gram_wide', 'tkr_als_gram_wide', ALS_CG_MAX_K, als_gram_wide_workspace_bytes, Y, rows, scale, ridge, workspace, out, check)


def als_cg_rows(Y, G, like_ptr, like_cols, X, *, w_like, w_rhs, ridge, steps=ALS_CG_STEPS, prior=None, w_prior=0.0, want_loss=False, check=True):
    """K24, in place on X fp32 [n_x, k]: `steps` steps of conjugate gradients on (G + w_like sum y y^T + ridge I) x = w_rhs sum y
    (+ w_prior prior[r]) from the value X[r] holds; without a prior the rows without likes are left as they are, with one every row is
    solved (include/tkr.h tkr_als_cg_rows).  -> row_loss float64 [n_x] with want_loss, else None.  A refusal raises AlsCgRefused naming
    row and kind; check=False returns (row_loss, status tensor) instead and reads nothing back"""
    what = 'als_cg_rows'
    n_y, k, n_x, n_likes = _als_rows(what, ALS_CG_MAX_K, Y, G, like_ptr, like_cols, X, [] if prior is None else [prior])
    if not isinstance(steps, (int,)) or isinstance(steps, bool) or steps < 0:
        raise ValueError('%s: steps = %r must be an integer, at least 0' % (what, steps))
    loss = torch.empty(n_x, dtype=torch.float64, device=Y.device) if want_loss else None
    status = torch.empty(1, dtype=torch.int64, device=Y.device)
    _call('tkr_als_cg_rows', Y, _p(Y), C.c_int32(n_y), C.c_int32(k), _p(G), _p(like_ptr), _p(like_cols) if n_likes else C.c_void_p(0),
          C.c_int64(n_likes), C.c_int64(n_x), C.c_double(w_like), C.c_double(w_rhs), C.c_double(ridge), C.c_int32(steps), _p(X), _p(loss),
          _p(prior), C.c_double(w_prior), C.c_void_p(0), C.c_int64(0), _p(status))
    return _done(what, loss, status, check, _ALS_CG_REFUSED, AlsCgRefused)


# ---- what K25 and K27 share: tables augmented by a few columns, D of X's shape beside a workspace, the step over a like CSR -------------------
def _ws_bytes(workspace):
    return C.c_int64(workspace.numel() * workspace.element_size())


def _aug_tables(what, pairs, extra, max_k):
    """pairs: (name, tensor), all fp32 [., k + extra] on one GPU -> k"""
    k = None
    for name, t in pairs:
        _, K = _als_table(what, name, t, max_k + extra, None if k is None else k + extra)
        if K < extra + 1:
            raise ValueError('%s: %s has %d columns; a table holds k + %d of them, k >= 1' % (what, name, K, extra))
        k = K - extra
        _on_gpu(what, name, t, pairs[0][1].device)
    return k


def _aug_dense_out(what, X, Y, k, sizer, workspace, out):
    """behind the operand checks of a *_dense_rows call -> (workspace, D): room for sizer(n_x, k, n_y) bytes; D of X's shape, `out` or new"""
    workspace = workspace_room(workspace, sizer(int(X.shape[0]), k, int(Y.shape[0])), X.device)
    D = torch.empty(tuple(X.shape), dtype=torch.float32, device=X.device) if out is None else out
    _operand(what, 'out', D, torch.float32, 2, on=X.device)
    if D.shape != X.shape:
        raise TkrError('%s: out must have the shape of X, %s' % (what, tuple(X.shape)))
    return workspace, D


def _aug_step_rows(what, family, Y, D, like_ptr, like_cols, X, H, fixed, weight, lam, lr, heavy_from, want_loss, workspace, check):
    """the body of lmf_step_rows and smf_step_rows, which call tkr_<what>.  family: (extra columns, max k, lowest `fixed`, the C type
    of `weight`, the scalar between fixed and lam, the workspace's size call, heavy_from's default, the refusals' messages, their class)"""
    extra, max_k, fixed_min, weight_type, sizer, heavy_default, messages, raises = family
    k = _aug_tables(what, [('Y', Y), ('X', X), ('D', D), ('H', H)], extra, max_k)
    n_y, n_x = int(Y.shape[0]), int(X.shape[0])
    if D.shape != X.shape or H.shape != X.shape:
        raise TkrError('%s: D and H must have the shape of X, %s' % (what, tuple(X.shape)))
    _operand(what, 'like_ptr', like_ptr, torch.int64, 1, on=Y.device, raises=_STD)
    _operand(what, 'like_cols', like_cols, torch.int32, 1, on=Y.device, raises=_STD)
    if like_ptr.numel() != n_x + 1:
        raise ValueError('%s: like_ptr must hold n_x + 1 = %d entries, not %d' % (what, n_x + 1, like_ptr.numel()))
    if not isinstance(fixed, (int,)) or isinstance(fixed, bool) or not fixed_min <= fixed < k + extra:
        raise ValueError('%s: fixed = %r must be a column, 0 <= fixed < %d%s' % (what, fixed, k + extra, ', or -1 for none' if fixed_min < 0 else ''))
    n_likes = int(like_cols.numel())
    heavy_from = heavy_default if heavy_from is None else int(heavy_from)
    workspace = workspace_room(workspace, sizer(n_x, k, 1) if heavy_from < n_likes else 0, Y.device)
    loss = torch.empty(n_x, dtype=torch.float64, device=Y.device) if want_loss else None
    status = torch.empty(1, dtype=torch.int64, device=Y.device)
    _call('tkr_' + what, Y, _p(Y), C.c_int32(n_y), C.c_int32(k), _p(D), _p(like_ptr), _p(like_cols) if n_likes else C.c_void_p(0),
          C.c_int64(n_likes), C.c_int64(n_x), C.c_int32(fixed), weight_type(weight), C.c_double(lam), C.c_double(lr), C.c_int64(heavy_from), _p(X), _p(H),
          _p(loss), _p(workspace), _ws_bytes(workspace), _p(status))
    return _done(what, loss, status, check, messages, raises)


# ---- K25: the two halves of a logistic-MF half-step (csrc/lmf.hip) --------------------------------------------------------------------------
LMF_MAX_K = 128              # TKR_LMF_MAX_K of include/tkr.h: the tables hold k + 2 columns
LMF_SLAB = 4096              # TKR_LMF_SLAB: the rows of Y one workgroup of lmf_dense_rows walks
LMF_LIKE_SLAB = 256          # TKR_LMF_LIKE_SLAB: the likes of a heavy row one wave sums as one chain
LMF_HEAVY_WAVES = 16         # TKR_LMF_HEAVY_WAVES
LMF_HEAVY_FROM = 2048        # a row with more likes than this is summed by a whole workgroup
LMF_NO_HEAVY = 1 << 62       # heavy_from: no row is heavy


class LmfRefused(AlsRefused):
    """a status word of K25 that is not -1 (the kinds 1 and 3 of K20)"""


_LMF_REFUSED = (None, _ALS_REFUSED[1], None, _ALS_REFUSED[3])


def lmf_workspace_bytes(n_x, k, n_y):
    return _size('tkr_lmf_workspace_bytes', (C.c_int64, C.c_int32, C.c_int64), (n_x, k, n_y))


_LMF_FAMILY = (2, LMF_MAX_K, 0, C.c_double, lmf_workspace_bytes, LMF_HEAVY_FROM, _LMF_REFUSED, LmfRefused)


def lmf_dense_rows(X, Y, want_loss=False, workspace=None, out=None):
    """K25 -> D fp32 [n_x, K] on the device: D[r] = sum over ALL rows c of Y of sigma(X[r] . Y[c]) Y[c], the score matrix never stored
    (include/tkr.h tkr_lmf_dense_rows).  X fp32 [n_x, K], Y fp32 [n_y, K], K = k + 2 <= LMF_MAX_K + 2.  want_loss: -> (D, sp), sp
    float64 [n_x] = sum_c softplus(X[r] . Y[c]).  Nothing is read back"""
    what = 'lmf_dense_rows'
    k = _aug_tables(what, [('X', X), ('Y', Y)], 2, LMF_MAX_K)
    n_x, n_y = int(X.shape[0]), int(Y.shape[0])
    workspace, D = _aug_dense_out(what, X, Y, k, lmf_workspace_bytes, workspace, out)
    sp = torch.empty(n_x, dtype=torch.float64, device=X.device) if want_loss else None
    _call('tkr_lmf_dense_rows', X, _p(X), C.c_int64(n_x), _p(Y), C.c_int64(n_y), C.c_int32(k), _p(D), _p(sp), _p(workspace), _ws_bytes(workspace))
    return (D, sp) if want_loss else D


def lmf_step_rows(Y, D, like_ptr, like_cols, X, H, *, fixed, alpha, lam, lr, heavy_from=None, want_loss=False, workspace=None, check=True):
    """K25, in place on X and its AdaGrad slot H (both fp32 [n_x, K]): for every row r the sum over its likes, rows of Y, of
    (1 - sigma(s)) y, the gradient g = alpha L - D[r] - lam x, h += g^2, x += lr g / sqrt(h); column `fixed` keeps its bits
    (include/tkr.h tkr_lmf_step_rows).  D: lmf_dense_rows(X, Y).  -> row_loss float64 [n_x] with want_loss, else None.  heavy_from:
    None = LMF_HEAVY_FROM.  A refusal raises LmfRefused naming row and kind; check=False returns (row_loss, status tensor) instead
    and reads nothing back"""
    return _aug_step_rows('lmf_step_rows', _LMF_FAMILY, Y, D, like_ptr, like_cols, X, H, fixed, alpha, lam, lr, heavy_from, want_loss, workspace, check)


# ---- K27: the three parts of a softmax-MF half-step (csrc/smf.hip) ---------------------------------------------------------------------------
SMF_MAX_K = 128              # TKR_SMF_MAX_K of include/tkr.h: the tables hold k + 1 columns
SMF_SLAB = 4096              # TKR_SMF_SLAB: the rows of Y one workgroup of smf_lse_rows / smf_dense_rows walks
SMF_HEAVY_FROM = LMF_HEAVY_FROM      # the heavy rows are K25's: slabs of LMF_LIKE_SLAB likes, LMF_HEAVY_WAVES waves
SMF_NO_HEAVY = 1 << 62       # heavy_from: no row is heavy


class SmfRefused(AlsRefused):
    """a status word of K27 that is not -1 (the kinds 1 and 3 of K20)"""


_SMF_REFUSED = _LMF_REFUSED


def smf_workspace_bytes(n_x, k, n_y):
    return _size('tkr_smf_workspace_bytes', (C.c_int64, C.c_int32, C.c_int64), (n_x, k, n_y))


_SMF_FAMILY = (1, SMF_MAX_K, -1, C.c_int32, smf_workspace_bytes, SMF_HEAVY_FROM, _SMF_REFUSED, SmfRefused)


def smf_lse_rows(X, Y, workspace=None, out=None):
    """K27 -> lse fp32 [n_x] on the device: lse[r] = log sum over ALL rows c of Y of exp(X[r] . Y[c]), finite at any finite scores
    (include/tkr.h tkr_smf_lse_rows).  X fp32 [n_x, K], Y fp32 [n_y, K], K = k + 1 <= SMF_MAX_K + 1.  Nothing is read back"""
    what = 'smf_lse_rows'
    k = _aug_tables(what, [('X', X), ('Y', Y)], 1, SMF_MAX_K)
    n_x, n_y = int(X.shape[0]), int(Y.shape[0])
    workspace = workspace_room(workspace, smf_workspace_bytes(n_x, k, n_y), X.device)
    lse = torch.empty(n_x, dtype=torch.float32, device=X.device) if out is None else out
    _operand(what, 'out', lse, torch.float32, 1, numel=n_x, on=X.device)
    _call('tkr_smf_lse_rows', X, _p(X), C.c_int64(n_x), _p(Y), C.c_int64(n_y), C.c_int32(k), _p(lse), _p(workspace), _ws_bytes(workspace))
    return lse


def smf_dense_rows(X, Y, row_off=None, col_off=None, workspace=None, out=None):
    """K27 -> D fp32 [n_x, K] on the device: D[r] = sum over ALL rows c of Y of exp((X[r] . Y[c] - row_off[r]) - col_off[c]) Y[c], the
    score matrix never stored (include/tkr.h tkr_smf_dense_rows).  row_off fp32 [n_x], col_off fp32 [n_y]; None is 0, +inf is legal
    and makes the term +0.  Nothing is read back"""
    what = 'smf_dense_rows'
    k = _aug_tables(what, [('X', X), ('Y', Y)], 1, SMF_MAX_K)
    n_x, n_y = int(X.shape[0]), int(Y.shape[0])
    _operand(what, 'row_off', row_off, torch.float32, 1, numel=n_x, on=X.device, optional=True)
    _operand(what, 'col_off', col_off, torch.float32, 1, numel=n_y, on=X.device, optional=True)
    workspace, D = _aug_dense_out(what, X, Y, k, smf_workspace_bytes, workspace, out)
    _call('tkr_smf_dense_rows', X, _p(X), C.c_int64(n_x), _p(Y), C.c_int64(n_y), C.c_int32(k), _p(row_off), _p(col_off), _p(D), _p(workspace),
          _ws_bytes(workspace))
    return D


def smf_step_rows(Y, D, like_ptr, like_cols, X, H, *, fixed, scale_by_likes, lam, lr, heavy_from=None, want_loss=False, workspace=None, check=True):
    """K27, in place on X and its AdaGrad slot H (both fp32 [n_x, K]): for every row r the sum L over its likes, rows of Y, the gradient
    g = L - w D[r] - lam x (w: the row's like count with scale_by_likes, else 1), h += g^2, x += lr g / sqrt(h); column `fixed` keeps
    its bits, -1 fixes none (include/tkr.h tkr_smf_step_rows).  D: smf_dense_rows(X, Y, ...).  -> row_loss float64 [n_x] with
    want_loss, else None.  heavy_from: None = SMF_HEAVY_FROM.  A refusal raises SmfRefused naming row and kind; check=False returns
    (row_loss, status tensor) instead and reads nothing back"""
    return _aug_step_rows('smf_step_rows', _SMF_FAMILY, Y, D, like_ptr, like_cols, X, H, fixed, 1 if scale_by_likes else 0, lam, lr, heavy_from, want_loss,
                          workspace, check)


# ---- K26: a sparse x dense product and CER's E-step by conjugate gradients (csrc/sparse.hip) ------------------------------------------------
SPMM_SLAB = 256              # TKR_SPMM_SLAB of include/tkr.h: the nonzeros of a heavy row summed as one chain
SPMM_HEAVY_FROM = 2048       # TKR_SPMM_HEAVY_FROM: a row with more nonzeros than this is summed by a whole workgroup
SPMM_NO_HEAVY = 1 << 62      # heavy_from: no row is heavy
ESTEP_SLAB = 1024            # TKR_ESTEP_SLAB: the rows of E whose part of a dot product is one fp32 partial
ESTEP_STEPS = 8              # the steps per E-step als.py takes by default
_SPMM_REFUSED = ('row %d holds a column outside [0, n_cols) (kind 0)', 'row %d holds a value that is not finite (kind 1)', None,
                 'ptr does not start at 0, decreases or leaves [0, nnz] at row %d (kind 3)')
_ESTEP_REFUSED = ('row %d of F (from n_items on: row - n_items of F^T) holds a column outside the matrix (kind 0)',
                  'row %d of F (from n_items on: row - n_items of F^T), or that row of V, holds a value that is not finite (kind 1)',
                  'p.q of column %d of E is not positive and finite: the column keeps the value it came in with (kind 2)',
                  'ptr does not start at 0, decreases or leaves [0, nnz] at row %d of F (from n_items on: row - n_items of F^T) (kind 3)')


class EstepRefused(TkrError):
    """a status word of K26 that is not -1; .word, .row and .kind say what it holds (include/tkr.h; raised by status_check)"""


class Csr:
    """a CSR matrix on one GPU: ptr int64 [n_rows + 1], col int32 [nnz], val fp32 [nnz], shape (n_rows, n_cols)"""
    __slots__ = ('ptr', 'col', 'val', 'shape')

    def __init__(self, ptr, col, val, shape):
        self.ptr, self.col, self.val, self.shape = ptr, col, val, (int(shape[0]), int(shape[1]))

    @property
    def nnz(self):
        return int(self.col.numel())

    @property
    def device(self):
        return self.ptr.device


def csr_upload(matrix, device):
    """a scipy.sparse matrix (any format, any dtype) -> Csr on `device`, as the matrix stores it once it is a CSR"""
    import numpy as np
    m = matrix.tocsr()
    up = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a, dtype=dt)).to(device)
    return Csr(up(m.indptr, np.int64), up(m.indices, np.int32), up(m.data, np.float32), m.shape)


def _csr(what, name, A):
    if not isinstance(A, Csr):
        raise TypeError('%s: %s must be a tkr_hip.Csr (csr_upload makes one of a scipy matrix)' % (what, name))
    n_rows, n_cols = A.shape
    if n_rows < 1 or n_cols < 1:
        raise ValueError('%s: %s has shape %s' % (what, name, A.shape))
    _operand(what, name + '.ptr', A.ptr, torch.int64, 1, numel=n_rows + 1, raises=_STD)
    _operand(what, name + '.col', A.col, torch.int32, 1, on=A.ptr.device, raises=_STD)
    _operand(what, name + '.val', A.val, torch.float32, 1, numel=A.nnz, on=A.ptr.device, raises=_STD)
    return n_rows, n_cols


def _spmm_table(what, name, t, rows, k, device):
    _operand(what, name, t, torch.float32, 2, on=device)
    if tuple(t.shape) != (rows, k):
        raise TkrError('%s: %s has shape %s, the call needs (%d, %d)' % (what, name, tuple(t.shape), rows, k))


def _heavy_from(what, heavy_from):
    heavy_from = SPMM_HEAVY_FROM if heavy_from is None else heavy_from
    if not isinstance(heavy_from, int) or isinstance(heavy_from, bool) or heavy_from < 1:
        raise ValueError('%s: heavy_from = %r must be an integer, at least 1' % (what, heavy_from))
    return heavy_from


def csr_spmm_workspace_bytes(n_rows):
    return _size('tkr_csr_spmm_workspace_bytes', (C.c_int64,), (n_rows,))


def csr_spmm(A, X, *, alpha=1.0, Z=None, beta=0.0, heavy_from=None, workspace=None, out=None, check=True):
    """K26 -> out fp32 [n_rows, k] on the device: out[r] = alpha * sum over row r's nonzeros of val * X[col] (+ beta * Z[r]), one fma
    chain per component in stored order, rounded once (include/tkr.h tkr_csr_spmm).  A: a Csr; X fp32 [n_cols, k], 1 <= k <=
    ALS_CG_MAX_K; Z fp32 [n_rows, k] or None.  heavy_from: None = SPMM_HEAVY_FROM.  A refusal raises EstepRefused naming row and kind
    (the refused row of out is not written); check=False returns (out, status tensor) instead and reads nothing back"""
    what = 'csr_spmm'
    n_rows, n_cols = _csr(what, 'A', A)
    _operand(what, 'X', X, torch.float32, 2, on=A.device)
    k = int(X.shape[1])
    if X.shape[0] != n_cols:
        raise TkrError('%s: X has shape %s, A has %d columns' % (what, tuple(X.shape), n_cols))
    if not 1 <= k <= ALS_CG_MAX_K:
        raise ValueError('%s: k = %d, 1 <= k <= %d is supported' % (what, k, ALS_CG_MAX_K))
    if Z is not None:
        _spmm_table(what, 'Z', Z, n_rows, k, A.device)
    if out is None:
        out = torch.empty((n_rows, k), dtype=torch.float32, device=A.device)
    _spmm_table(what, 'out', out, n_rows, k, A.device)
    heavy_from = _heavy_from(what, heavy_from)
    workspace = workspace_room(workspace, csr_spmm_workspace_bytes(n_rows) if heavy_from < A.nnz else 0, A.device)
    status = torch.empty(1, dtype=torch.int64, device=A.device)
    _call('tkr_csr_spmm', X, _p(A.ptr), _p(A.col) if A.nnz else C.c_void_p(0), _p(A.val) if A.nnz else C.c_void_p(0), C.c_int64(A.nnz),
          C.c_int64(n_rows), C.c_int32(n_cols), _p(X), C.c_int32(k), C.c_double(alpha), _p(Z), C.c_double(beta), _p(out), C.c_int64(heavy_from),
          _p(workspace), C.c_int64(workspace.numel() * workspace.element_size()), _p(status))
    return _done(what, out, status, check, _SPMM_REFUSED, EstepRefused)


def estep_cg_workspace_bytes(n_items, d, k):
    return _size('tkr_estep_cg_workspace_bytes', (C.c_int64, C.c_int64, C.c_int32), (n_items, d, k))


def estep_cg(F, Ft, V, E, *, lv, le, steps=ESTEP_STEPS, heavy_from=None, workspace=None, check=True):
    """K26, in place on E fp32 [d, k]: `steps` steps of conjugate gradients on (lv F^T F + le I) E = lv F^T V from the value E holds
    (include/tkr.h tkr_estep_cg).  F: the Csr of the features [n_items, d]; Ft: the Csr of its transpose; both canonical.  V fp32
    [n_items, k].  -> E.  A refusal raises EstepRefused naming what and where (of the input: E is untouched; of a column: that column
    is); check=False returns (E, status tensor) instead and reads nothing back"""
    what = 'estep_cg'
    n_items, d = _csr(what, 'F', F)
    if _csr(what, 'Ft', Ft) != (d, n_items) or Ft.nnz != F.nnz or Ft.device != F.device:
        raise TkrError('%s: Ft must be the transpose of F, %d x %d with %d nonzeros, on the same GPU' % (what, d, n_items, F.nnz))
    _operand(what, 'V', V, torch.float32, 2, on=F.device)
    k = int(V.shape[1])
    if V.shape[0] != n_items:
        raise TkrError('%s: V has shape %s, F has %d rows' % (what, tuple(V.shape), n_items))
    if not 1 <= k <= ALS_CG_MAX_K:
        raise ValueError('%s: k = %d, 1 <= k <= %d is supported' % (what, k, ALS_CG_MAX_K))
    _spmm_table(what, 'E', E, d, k, F.device)
    if not isinstance(steps, int) or isinstance(steps, bool) or steps < 1:
        raise ValueError('%s: steps = %r must be an integer, at least 1' % (what, steps))
    if not (0 < lv < float('inf') and 0 < le < float('inf')):
        raise ValueError('%s: lv = %r and le = %r must be positive and finite' % (what, lv, le))
    heavy_from = _heavy_from(what, heavy_from)
    workspace = workspace_room(workspace, estep_cg_workspace_bytes(n_items, d, k), F.device)
    status = torch.empty(1, dtype=torch.int64, device=F.device)
    nil = C.c_void_p(0)
    _call('tkr_estep_cg', V, _p(F.ptr), _p(F.col) if F.nnz else nil, _p(F.val) if F.nnz else nil, _p(Ft.ptr), _p(Ft.col) if F.nnz else nil,
          _p(Ft.val) if F.nnz else nil, C.c_int64(F.nnz), C.c_int64(n_items), C.c_int64(d), _p(V), C.c_int32(k), _p(E), C.c_double(lv),
          C.c_double(le), C.c_int32(steps), C.c_int64(heavy_from), _p(workspace), C.c_int64(workspace.numel() * workspace.element_size()), _p(status))
    return _done(what, E, status, check, _ESTEP_REFUSED, EstepRefused)


# ---- K28 / K29: the item-neighbourhood model, built and served (csrc/knn.hip) -----------------------------------------------------------------
KNN_MAX_N = 512              # TKR_KNN_MAX_N of include/tkr.h: neighbours kept per item
KNN_MAX_K = 32               # TKR_KNN_MAX_K: columns one launch of K29 lists per line
KNN_MAX_SLAB = 36864         # TKR_KNN_MAX_SLAB: columns one workgroup keeps in LDS
KNN_HEAVY_FROM = 262144      # TKR_KNN_HEAVY_FROM: a row with more work than this is shared by several workgroups
_KNN_BUILD_REFUSED = ('u_ptr does not start at 0, decreases or leaves its array at row %d (from n_users + 1 on: row - n_users - 1 of i_ptr) (kind 0)',
                      'entry %d of u_cols (from len(u_cols) on: entry - len(u_cols) of i_rows) is outside the matrix (kind 1)',
                      'the two CSRs hold different numbers of entries (kind 2, word %d)', 'norm[%d] is not finite and positive (kind 3)')
_KNN_SCORE_REFUSED = ('hist_ptr does not start at 0, decreases or leaves [0, len(hist_cols)] at row %d (kind 0)',
                      'entry %d of hist_cols is outside [0, n_items) (kind 1)',
                      'like_ptr does not start at 0, decreases or leaves [0, len(like_cols)] at row %d (kind 2)')


class KnnRefused(TkrError):
    """a status word of K28 or K29 that is not -1; .word, .row and .kind say what it holds (include/tkr.h; raised by status_check)"""


def _knn_slab(what, slab_cols):
    slab_cols = 0 if slab_cols is None else slab_cols
    if not isinstance(slab_cols, int) or isinstance(slab_cols, bool) or not 0 <= slab_cols <= KNN_MAX_SLAB:
        raise ValueError('%s: slab_cols = %r must be an integer in [1, %d], or None for the widest slab' % (what, slab_cols, KNN_MAX_SLAB))
    return slab_cols


def _knn_ptr(what, name, ptr, cols, on=None):
    _operand(what, name + '_ptr', ptr, torch.int64, 1, at_least=2, on=on)
    _operand(what, name + ' entries', cols, torch.int32, 1, on=ptr.device)
    return int(ptr.numel()) - 1


def knn_build_workspace_bytes(n_items):
    return _size('tkr_knn_build_workspace_bytes', (C.c_int64,), (n_items,))


def knn_build(u_ptr, u_cols, i_ptr, i_rows, norm, N, *, shrink=0.0, heavy_from=None, slab_cols=None, workspace=None, out=None, check=True):
    """K28 -> (nbr_ids int32 [n_items, N], nbr_w fp32 [n_items, N]) on the device: for every item the N items with the largest
    sim(i, j) = fp32(c_ij / (fl64(norm[i] * norm[j]) + shrink)), c_ij the number of users who like both, in the canonical order (ties ->
    the higher column first), padded -1 / +0.0 (include/tkr.h tkr_knn_build).  u_ptr / u_cols: the likes as a CSR over users (int64 /
    int32, ascending and unique in a row); i_ptr / i_rows: its transpose over items; norm float64 [n_items].  heavy_from: None =
    KNN_HEAVY_FROM; slab_cols: None = KNN_MAX_SLAB; the result depends on neither.  out: a pair of tensors to write.  A refusal raises
    KnnRefused and leaves the outputs untouched; check=False returns ((nbr_ids, nbr_w), status tensor) instead and reads nothing back"""
    what = 'knn_build'
    n_users = _knn_ptr(what, 'u', u_ptr, u_cols)
    n_items = _knn_ptr(what, 'i', i_ptr, i_rows, on=u_ptr.device)
    dev = u_ptr.device
    _operand(what, 'norm', norm, torch.float64, 1, numel=n_items, on=dev)
    if not isinstance(N, int) or isinstance(N, bool) or not 1 <= N <= KNN_MAX_N:
        raise ValueError('%s: N = %r, 1 <= N <= %d neighbours are supported' % (what, N, KNN_MAX_N))
    if not (0.0 <= shrink < float('inf')):
        raise ValueError('%s: shrink = %r must be finite and not negative' % (what, shrink))
    heavy_from = KNN_HEAVY_FROM if heavy_from is None else heavy_from
    if not isinstance(heavy_from, int) or isinstance(heavy_from, bool) or heavy_from < 1:
        raise ValueError('%s: heavy_from = %r must be an integer, at least 1' % (what, heavy_from))
    slab_cols = _knn_slab(what, slab_cols)
    if out is None:
        out = (torch.empty((n_items, N), dtype=torch.int32, device=dev), torch.empty((n_items, N), dtype=torch.float32, device=dev))
    _operand(what, 'nbr_ids', out[0], torch.int32, 2, numel=n_items * N, on=dev)
    _operand(what, 'nbr_w', out[1], torch.float32, 2, numel=n_items * N, on=dev)
    workspace = workspace_room(workspace, knn_build_workspace_bytes(n_items), dev)
    status = torch.empty(1, dtype=torch.int64, device=dev)
    nil = C.c_void_p(0)
    _call('tkr_knn_build', u_ptr, _p(u_ptr), _p(u_cols) if u_cols.numel() else nil, C.c_int64(u_cols.numel()), _p(i_ptr),
          _p(i_rows) if i_rows.numel() else nil, C.c_int64(i_rows.numel()), C.c_int64(n_users), C.c_int64(n_items), _p(norm), C.c_double(shrink),
          C.c_int32(N), C.c_int64(heavy_from), C.c_int32(slab_cols), _p(out[0]), _p(out[1]), _p(workspace),
          C.c_int64(workspace.numel() * workspace.element_size()), _p(status))
    return _done(what, out, status, check, _KNN_BUILD_REFUSED, KnnRefused)


def _knn_score_once(args, n_rows, K, mask, mask_pitch, want_scores, likes, slab_cols, dev):
    hist_ptr, hist_cols, nbr_ids, nbr_w, n_items, N, col_of_item, n_cols = args
    nil = C.c_void_p(0)
    ids = torch.empty((n_rows, K), dtype=torch.int32, device=dev) if K else None
    scores = torch.empty((n_rows, K), dtype=torch.float32, device=dev) if K and want_scores else None
    ranks = torch.empty(int(likes[1].numel()), dtype=torch.int32, device=dev) if likes is not None else None
    status = torch.empty(1, dtype=torch.int64, device=dev)
    _call('tkr_knn_score', hist_ptr, _p(hist_ptr), _p(hist_cols) if hist_cols.numel() else nil, C.c_int64(hist_cols.numel()), C.c_int64(n_rows),
          _p(nbr_ids), _p(nbr_w), C.c_int32(n_items), C.c_int32(N), _p(col_of_item), C.c_int32(n_cols), _p(mask), C.c_int32(mask_pitch),
          C.c_int32(K), _p(ids), _p(scores), _p(likes[0]) if likes is not None else nil,
          _p(likes[1]) if likes is not None and likes[1].numel() else nil, C.c_int64(likes[1].numel() if likes is not None else 0), _p(ranks),
          C.c_int32(slab_cols), _p(status))
    status_check('knn_score', _KNN_SCORE_REFUSED, KnnRefused, int(status.item()))
    return ids, scores, ranks


def knn_score(hist_ptr, hist_cols, nbr_ids, nbr_w, K, *, col_of_item=None, n_cols=None, mask=None, mask_pitch=0, want_scores=False,
              like_ptr=None, like_cols=None, slab_cols=None):
    """K29 -> ids int32 [n_rows, K] (with want_scores: (ids, scores fp32 [n_rows, K]); with like_ptr / like_cols the ranks int32
    [n_likes] come last; K = 0 with likes: the ranks alone).  hist_ptr / hist_cols: the liked catalogue items of every line (int64 /
    int32, ascending and unique); nbr_ids / nbr_w: K28's table; col_of_item int32 [n_items] or None: the column of a catalogue item or
    -1, with n_cols columns (None: the identity).  The score of a column is the fp32 chain over the history, in stored order, of the
    weights with which its item is among the N nearest of a history item; lists and ranks are score_topk's and like_ranks's with that
    score (include/tkr.h tkr_knn_score).  K above KNN_MAX_K is served as score_topk serves it: the best KNN_MAX_K, then the best of what
    is left with the found columns added to a copy of the mask, and so on.  A refusal raises KnnRefused"""
    what = 'knn_score'
    n_rows = _knn_ptr(what, 'hist', hist_ptr, hist_cols)
    dev = hist_ptr.device
    _operand(what, 'nbr_ids', nbr_ids, torch.int32, 2, on=dev)
    _operand(what, 'nbr_w', nbr_w, torch.float32, 2, numel=nbr_ids.numel(), on=dev)
    n_items, N = int(nbr_ids.shape[0]), int(nbr_ids.shape[1])
    if tuple(nbr_w.shape) != (n_items, N) or n_items < 1 or not 1 <= N <= KNN_MAX_N:
        raise TkrError('%s: the table has shapes %s and %s; both must be (n_items, N), 1 <= N <= %d' % (what, tuple(nbr_ids.shape), tuple(nbr_w.shape),
                                                                                                     KNN_MAX_N))
    _operand(what, 'col_of_item', col_of_item, torch.int32, 1, numel=n_items, on=dev, optional=True)
    n_cols = n_items if col_of_item is None and n_cols is None else n_cols
    if not isinstance(n_cols, int) or isinstance(n_cols, bool) or n_cols < 1 or (col_of_item is None and n_cols != n_items):
        raise ValueError('%s: n_cols = %r must be a positive integer, and the number of items without col_of_item' % (what, n_cols))
    if (like_ptr is None) != (like_cols is None):
        raise ValueError('%s: like_ptr and like_cols go together' % what)
    if not isinstance(K, int) or isinstance(K, bool) or K < 0 or (K == 0 and like_ptr is None):
        raise ValueError('%s: K = %r must be a positive integer (0 with likes: the ranks alone)' % (what, K))
    likes = None
    if like_ptr is not None:
        if _knn_ptr(what, 'like', like_ptr, like_cols, on=dev) != n_rows:
            raise TkrError('%s: like_ptr holds %d rows, hist_ptr %d' % (what, like_ptr.numel() - 1, n_rows))
        likes = (like_ptr, like_cols)
    if mask is not None:
        _operand(what, 'mask', mask, torch.int32, at_least=((n_cols + 31) // 32) * mask_pitch, on=dev)
        if mask_pitch < n_rows:
            raise ValueError('%s: mask_pitch = %d is below the %d rows' % (what, mask_pitch, n_rows))
    slab_cols = _knn_slab(what, slab_cols)
    args = (hist_ptr, hist_cols, nbr_ids, nbr_w, n_items, N, col_of_item, n_cols)
    if K <= KNN_MAX_K:
        ids, scores, ranks = _knn_score_once(args, n_rows, K, mask, mask_pitch, want_scores, likes, slab_cols, dev)
    else:
        pitch = mask_pitch if mask is not None else (n_rows + 31) // 32 * 32
        work = mask.clone() if mask is not None else torch.zeros(((n_cols + 31) // 32) * pitch, dtype=torch.int32, device=dev)
        ptr = torch.arange(0, (n_rows + 1) * KNN_MAX_K, KNN_MAX_K, dtype=torch.int64, device=dev)
        parts_i, parts_s, left, ranks = [], [], K, None
        while left > 0:
            first = not parts_i                       # the ranks are counted under the caller's mask: by the first launch
            ids, scores, r = _knn_score_once(args, n_rows, KNN_MAX_K, work, pitch, want_scores, likes if first else None, slab_cols, dev)
            ranks = r if first else ranks
            take = min(left, KNN_MAX_K)
            parts_i.append(ids[:, :take])
            if want_scores:
                parts_s.append(scores[:, :take])
            left -= take
            if left > 0:                              # found columns join the mask (negative ids = padding are skipped by the kernel)
                _call('tkr_build_rated_mask', work, _p(ptr), _p(ids.reshape(-1)), C.c_int32(n_rows), C.c_int32(n_cols), _p(work), C.c_int32(pitch))
        ids = torch.cat(parts_i, dim=1).contiguous()
        scores = torch.cat(parts_s, dim=1).contiguous() if want_scores else None
    result = tuple(x for x in (ids, scores if want_scores else None, ranks) if x is not None)
    return result[0] if len(result) == 1 else result


# ---- K22: a dense MLP content encoder, applied and trained (csrc/mlp.hip)------------------------------------------------------------------
MLP_MAX_LAYERS = 5          # TKR_MLP_MAX_LAYERS of include/tkr.h
MLP_MAX_BATCH = 256          # TKR_MLP_MAX_BATCH
MLP_SLAB = 512               # TKR_MLP_SLAB: the inputs of a layer one workgroup sums
MLP_FORWARD_CHUNK = 256      # TKR_MLP_FORWARD_CHUNK


class MlpNet(C.Structure):
    """mirror of tkr_mlp_net (include/tkr.h)"""
    _fields_ = [('n_layers', C.c_int32), ('width', C.c_int32 * (MLP_MAX_LAYERS + 1))] + \
               [(n, C.c_void_p * MLP_MAX_LAYERS) for n in ('W', 'bias', 'msW', 'msb')]


class MlpRefused(TkrError):
    """a status word of K22 that is not -1: .position (= .row) is the entry of rows / order that lies outside [0, n)"""
    position = property(lambda self: self.row)


_MLP_REFUSED = (None, 'entry %d of the row list lies outside [0, n)')


def mlp_net(layers):
    """layers: per dense layer a dict of device tensors W fp32 [in, out], bias [out] and (for mlp_fit) msW, msb -> MlpNet; the tensors
    live as long as the struct"""
    what = 'mlp_net'
    if not 1 <= len(layers) <= MLP_MAX_LAYERS:
        raise ValueError('%s: %d layers, 1 <= layers <= %d is supported' % (what, len(layers), MLP_MAX_LAYERS))
    net = MlpNet()
    net.n_layers = len(layers)
    device = layers[0]['W'].device
    for l, layer in enumerate(layers):
        W = layer['W']
        _operand(what, 'W of layer %d' % l, W, torch.float32, 2, on=device)
        if W.shape[0] < 1 or W.shape[1] < 1:
            raise TkrError('%s: W of layer %d has shape %s' % (what, l, tuple(W.shape)))
        if l and W.shape[0] != layers[l - 1]['W'].shape[1]:
            raise ValueError('%s: layer %d takes %d inputs, layer %d gives %d' % (what, l, W.shape[0], l - 1, layers[l - 1]['W'].shape[1]))
        net.width[l], net.width[l + 1] = int(W.shape[0]), int(W.shape[1])
        net.W[l] = W.data_ptr()
        for name, shape in (('bias', W.shape[1:]), ('msW', W.shape), ('msb', W.shape[1:])):
            t = layer.get(name)
            if t is None and name in ('msW', 'msb'):
                continue
            _operand(what, '%s of layer %d' % (name, l), t, torch.float32, len(shape), on=device)
            if t.shape != shape:
                raise TkrError('%s: %s of layer %d must have shape %s, not %s' % (what, name, l, tuple(shape), tuple(t.shape)))
            getattr(net, name)[l] = t.data_ptr()
    net.keep = layers
    net.device = device
    return net


def mlp_workspace_bytes(net, m, batch=0):
    return _size('tkr_mlp_workspace_bytes', (C.byref, C.c_int64, C.c_int32), (net, m, batch), 'm = %d, batch = %d' % (m, batch))


def _mlp_table(what, name, t, n, width, device):
    """X or Y of the K22 entry points: fp32 [n, width] (n None: any, at least one row) on the GPU of the parameters"""
    _operand(what, name, t, torch.float32, 2, on=device)
    if t.shape[1] != width or t.shape[0] < 1 or (n is not None and t.shape[0] != n):
        raise TkrError('%s: %s must be [n, %d], not %s' % (what, name, width, tuple(t.shape)))


def mlp_forward(net, X, rows=None, workspace=None, out=None, check=True):
    """K22 -> fp32 [m, k] on the device: the network applied to X[rows] (int32 tensor; None: every row of X), include/tkr.h
    tkr_mlp_forward.  A row outside [0, n) raises MlpRefused and nothing is written; check=False returns (out, status tensor) and
    reads nothing back"""
    what = 'mlp_forward'
    _mlp_table(what, 'X', X, None, net.width[0], net.device)
    n = int(X.shape[0])
    _operand(what, 'rows', rows, torch.int32, 1, on=X.device, optional=True)
    m = n if rows is None else int(rows.numel())
    k = net.width[net.n_layers]
    workspace = workspace_room(workspace, mlp_workspace_bytes(net, m), X.device)
    if out is None:
        out = torch.empty((m, k), dtype=torch.float32, device=X.device)
    _operand(what, 'out', out, torch.float32, 2, on=X.device)
    if tuple(out.shape) != (m, k):
        raise TkrError('%s: out must be [%d, %d], not %s' % (what, m, k, tuple(out.shape)))
    status = torch.empty(1, dtype=torch.int64, device=X.device)
    _call('tkr_mlp_forward', X, C.byref(net), _p(X), C.c_int32(n), C.c_void_p(0) if rows is None else _p(rows if m else X), C.c_int64(m),
          _p(out if m else X), _p(workspace), C.c_int64(workspace.numel() * workspace.element_size()), _p(status))
    return _done(what, out, status, check, _MLP_REFUSED, MlpRefused)


def mlp_fit(net, X, Y, order, batch, lr, workspace=None, check=True):
    """K22: one epoch of mini-batch RMSProp over the rows `order` (int32 tensor) of X fp32 [n, d] and Y fp32 [n, k], in place on the
    parameters and slots of `net` (include/tkr.h tkr_mlp_fit) -> batch_loss float64 [ceil(m / batch)] on the device.  An entry of
    order outside [0, n) raises MlpRefused and nothing is written; check=False returns (batch_loss, status tensor) and reads nothing
    back"""
    what = 'mlp_fit'
    k = net.width[net.n_layers]
    _mlp_table(what, 'X', X, None, net.width[0], net.device)
    _mlp_table(what, 'Y', Y, int(X.shape[0]), k, net.device)
    _operand(what, 'order', order, torch.int32, 1, on=X.device)
    batch = int(batch)
    if not 1 <= batch <= MLP_MAX_BATCH:
        raise ValueError('%s: batch = %d, 1 <= batch <= %d is supported' % (what, batch, MLP_MAX_BATCH))
    m = int(order.numel())
    workspace = workspace_room(workspace, mlp_workspace_bytes(net, 0, batch), X.device)
    loss = torch.zeros((m + batch - 1) // batch, dtype=torch.float64, device=X.device)
    status = torch.empty(1, dtype=torch.int64, device=X.device)
    _call('tkr_mlp_fit', X, C.byref(net), _p(X), C.c_int32(int(X.shape[0])), _p(Y), _p(order if m else X), C.c_int64(m), C.c_int32(batch),
          C.c_float(lr), _p(loss if m else X), _p(workspace), C.c_int64(workspace.numel() * workspace.element_size()), _p(status))
    return _done(what, loss, status, check, _MLP_REFUSED, MlpRefused)


# ---- K18: the metric values of every test line, their sums over resampled lines (csrc/line_metrics.hip) -------------------------------
LINE_MAX_TOTAL = 1024        # TKR_LINE_MAX_TOTAL of include/tkr.h
LINE_MAX_COLS = GROUP_MAX_COLS   # TKR_LINE_MAX_COLS: the bitmap of one line must fit the LDS of one workgroup, as K15's of one row
BOOT_MAX_COLUMNS = 64        # TKR_BOOT_MAX_COLUMNS: a lane per column of a row
BOOT_CHUNK = 8192            # TKR_BOOT_CHUNK: the draws one wave sums
_LINE_REFUSED = ('line %d holds a rank below -1', 'line %d holds a rank that is not below its number of unrated columns',
                 'line %d names a rank twice', 'like_ptr / rated_ptr do not ascend from 0 inside their arrays at line %d')


def line_metrics(ranks, like_ptr, rated_ptr, n_cols, step, total, gain, ideal):
    """K18 -> X float64 [n_lines, 3 * (total // step) + 5] on the device: per test line the hit counts, the like count, AUC / reciprocal
    rank with their flags, NDCG and average precision at every cut-off (include/tkr.h tkr_line_metrics; the columns:
    significance.columns).  ranks int32 [n_likes] as tkr_hip.like_ranks returns them, like_ptr / rated_ptr int64 [n_lines + 1], gain
    float64 [total], ideal float64 [total + 1], all on one GPU.  Ranks or pointers that cannot come from K8 raise TkrError"""
    what = 'line_metrics'
    _operand(what, 'ranks', ranks, torch.int32, 1)
    for name, t, dtype in (('like_ptr', like_ptr, torch.int64), ('rated_ptr', rated_ptr, torch.int64), ('gain', gain, torch.float64),
                           ('ideal', ideal, torch.float64)):
        _operand(what, name, t, dtype, 1, on=ranks.device)
    n_cols, step, total = int(n_cols), int(step), int(total)
    n_lines = int(like_ptr.numel()) - 1
    if n_lines < 0 or rated_ptr.numel() != n_lines + 1:
        raise TkrError('%s: like_ptr and rated_ptr must both hold n_lines + 1 entries' % what)
    if n_cols < 1 or step < 1 or total < 1:
        raise TkrError('%s: n_cols, step and total must be at least 1' % what)
    if total > LINE_MAX_TOTAL or n_cols > LINE_MAX_COLS:
        raise TkrError('%s: total = %d, n_cols = %d; at most %d and %d are supported' % (what, total, n_cols, LINE_MAX_TOTAL, LINE_MAX_COLS))
    if gain.numel() != total or ideal.numel() != total + 1:
        raise TkrError('%s: gain must hold total and ideal total + 1 entries' % what)
    X = torch.empty((n_lines, 3 * (total // step) + 5), dtype=torch.float64, device=ranks.device)
    if n_lines == 0:
        return X
    status = torch.empty(1, dtype=torch.int64, device=ranks.device)
    _call('tkr_line_metrics', ranks, _p(ranks) if ranks.numel() else C.c_void_p(0), C.c_int64(ranks.numel()), _p(like_ptr), _p(rated_ptr),
          C.c_int64(n_lines), C.c_int32(n_cols), C.c_int32(step), C.c_int32(total), _p(gain), _p(ideal), _p(X), _p(status))
    status_check(what, _LINE_REFUSED, TkrError, int(status.item()))
    return X


def boot_pitch(width):
    """the row pitch (doubles) bootstrap_sums copies a table of `width` columns to: whole 64- / 128-byte lines, the same lanes per row"""
    return next(p for p in (8, 16, 32, 48, 64) if width <= p)


def bootstrap_sums(X, R, seed, pad=True):
    """K18 -> float64 [R, C] on the device: row r = the column sums of n = len(X) rows of X (float64 [n, C], C <= 64) drawn with
    replacement, the draw a function of (seed, r, n) alone (include/tkr.h tkr_bootstrap_sums).  Bitwise repeatable.  pad: gather from
    a copy of X at a row pitch of whole cache lines (boot_pitch: faster, the same bits; one more table in memory)"""
    what = 'bootstrap_sums'
    _operand(what, 'X', X, torch.float64, 2)
    n, width = int(X.shape[0]), int(X.shape[1])
    R, seed = int(R), int(seed)
    if not 1 <= width <= BOOT_MAX_COLUMNS:
        raise TkrError('%s: X has %d columns, 1 to %d are supported' % (what, width, BOOT_MAX_COLUMNS))
    if not 1 <= n < 2 ** 31:
        raise TkrError('%s: X needs 1 to 2^31 - 1 rows, got %d' % (what, n))
    if not 1 <= R < 2 ** 31:
        raise TkrError('%s: 1 <= R < 2^31 required, got %d' % (what, R))
    if not 0 <= seed < 2 ** 64:
        raise TkrError('%s: the seed must fit 64 bits' % what)
    out = torch.empty((R, width), dtype=torch.float64, device=X.device)
    workspace = torch.empty(R * ((n + BOOT_CHUNK - 1) // BOOT_CHUNK) * width, dtype=torch.float64, device=X.device)
    pitch = boot_pitch(width) if pad else width
    if pitch != width:
        table = torch.zeros((n, pitch), dtype=torch.float64, device=X.device)
        table[:, :width] = X
    else:
        table = X
    _call('tkr_bootstrap_sums', X, _p(table), C.c_int64(n), C.c_int32(width), C.c_int64(pitch), C.c_int32(R), C.c_uint64(seed), _p(out),
          _p(workspace), C.c_int64(workspace.numel() * 8))
    return out


# ---- per-epoch exchange of replicated tables (csrc/sync.hip) ----------------------------------------
def sync_snapshot(P, cnt, start, n, w):
    _call('tkr_sync_snapshot', P, _p(P), _p(cnt), _p(start), C.c_int64(n), C.c_int32(w))


def sync_pack(P, ms, cnt, start, flat_delta, flat_ms, n, w, inv_world):
    _call('tkr_sync_pack', P, _p(P), _p(ms), _p(cnt), _p(start), _p(flat_delta), _p(flat_ms), C.c_int64(n), C.c_int32(w),
                               C.c_float(inv_world))


def sync_flow_snapshot(V, tailV, icnt, start, n, k, item_bufs=2):
    _call('tkr_sync_flow_snapshot', V, _p(V), _p(tailV), _p(icnt), _p(start), C.c_int32(n), C.c_int32(k), C.c_int32(item_bufs))


def sync_flow_pack(V, msV, tailV, icnt, start, flat_delta, flat_ms, n, k, inv_world, item_bufs=2):
    _call('tkr_sync_flow_pack', V, _p(V), _p(msV), _p(tailV), _p(icnt), _p(start), _p(flat_delta), _p(flat_ms), C.c_int32(n),
          C.c_int32(k), C.c_float(inv_world), C.c_int32(item_bufs))


def sync_flow_unpack(V, msV, tailV, rdV, icnt, start, flat_delta, flat_ms, n, k, item_bufs=2):
    _call('tkr_sync_flow_unpack', V, _p(V), _p(msV), _p(tailV), _p(rdV), _p(icnt), _p(start), _p(flat_delta), _p(flat_ms),
          C.c_int32(n), C.c_int32(k), C.c_int32(item_bufs))


def sync_unpack(P, ms, start, flat_delta, flat_ms, n, w):
    _call('tkr_sync_unpack', P, _p(P), _p(ms), _p(start), _p(flat_delta), _p(flat_ms), C.c_int64(n), C.c_int32(w))
