"""ctypes binding of libsrgnn_hip.so (the C-ABI declared in include/srgnn_hip.h).

The library is built in-tree by scalable-roubust-gnn_amd/csrc/Makefile (or __graft_entry__.build()).
There is no fallback: if the library is missing or fails to load, every product entry point raises.
"""
from __future__ import annotations

import ctypes
import os
import threading

import torch

_PKG_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB_PATH = os.environ.get("SRGNN_HIP_LIB", os.path.join(_PKG_ROOT, "lib", "libsrgnn_hip.so"))

SRG_OK = 0
SRG_ERR_INVALID = -1
SRG_ERR_HIP = -2
SRG_ERR_ALLOC = -3

SRG_SPMM_ACCUMULATE = 0x1
SRG_SPMM_NT_STORE = 0x2
SRG_SPMM_WIDE_ROWS = 0x4
SRG_SPMM_HUB_W256 = 0x8
SRG_SPMM_HUB_NOJOIN = 0x10
SRG_SPMM_PACKED_U2 = 0x20
SRG_SPMM_FAST = 0x40
SRG_SPMM_HUB_CONTINUE = 0x80
SRG_SPMM_CAP_WAVES = 0x200

SRG_CHEBY_INIT = 0
SRG_CHEBY_STEP = 1
SRG_CHEBY_INIT_T = 2
SRG_CHEBY_STEP_FIRST = 3
SRG_CHEBY_NO_T = 0x10
SRG_CHEBY_HUB_NOJOIN = 0x20

SRG_ACC_INIT = 0
SRG_ACC_ADD = 1
SRG_ACC_DIV = 2
SRG_ACC_COPY = 3
SRG_ACC_MIN = 4
SRG_ACC_MAX = 5
SRG_SIM_INIT = 0x1
SRG_SIM_HOP0 = 0x2
SRG_TAIL_MAX = 32
SRG_HOP_MAX = 32
SRG_HOP_GATE = 0
SRG_HOP_ORI_REF = 1
SRG_HOP_JK = 2
SRG_HOP_PAIR_TRANSPOSE = 0
SRG_HOP_PAIR_FLAT = 1

SRG_SPGEMM_SERIAL_B = 0x1

SRG_KNN_MAX_CAND = 4096
SRG_KNN_MAX_D = 8192
SRG_KNN_LAUNCH_ROWS = 4194304

SRG_GAT_MAX_HEADS = 32
SRG_GAT_MAX_WIDTH = 65536
SRG_GAT_LAUNCH_ROWS = 4194304

SRG_PLAN_MIN_HOPS_TO_CUT = 4
SRG_PLAN_MIN_HOPS_TO_COMPACT = 6
SRG_PLAN_COMPACT = 0x1
SRG_PLAN_SPANS = 0x2
SRG_PLAN_SPLIT_BLOCK0 = 0x4
SRG_PLAN_WHOLE_BLOCK0 = 0x8
SRG_PLAN_WHOLE_HUBS = 0x10
SRG_PLAN_WHOLE_MAX_SHIFT = 16
SRG_PLAN_AUTO = -1
SRG_PLAN_NONE = -2

SRG_HALO_AUTO = -1
SRG_HALO_NONE = -2
SRG_HALO_X_HALO_FILLED = 0x1
(SRG_HALO_STARTS, SRG_HALO_LOCAL_INDPTR, SRG_HALO_LOCAL_INDICES, SRG_HALO_GHOST_POSITIONS, SRG_HALO_HALO_IDS,
 SRG_HALO_GROUP_OFFSETS, SRG_HALO_GHOST_SEND, SRG_HALO_GHOST_SEND_COUNTS, SRG_HALO_GHOST_RECV_COUNTS,
 SRG_HALO_CHUNK_RANGES, SRG_HALO_HUB_THRESHOLDS, SRG_HALO_VIEW_ORDER, SRG_HALO_VIEW_META, SRG_HALO_SEND_ROWS,
 SRG_HALO_SEND_COUNTS, SRG_HALO_RECV_COUNTS) = range(16)


class HaloInfo(ctypes.Structure):
    """srg_halo_info (include/srgnn_hip.h)."""
    _fields_ = [(k, ctypes.c_int64) for k in ("row0", "n_rows", "n_recv", "n_ghost", "halo", "nnz_local",
                                               "n_groups", "hub_rows", "send_rows")] + \
               [(k, ctypes.c_int32) for k in ("ghost_max_degree", "chunks", "nranks", "rank")]

# every symbol include/srgnn_hip.h declares (checked by tests/test_capi.py)
EXPORTED_SYMBOLS = (
    "FloatCSRMulDenseOMP",
    "FloatCSRMulDense",
    "srg_spmm_csr_f32",
    "srg_propagate_khop_f32",
    "srg_propagate_plan_f32",
    "srg_plan_build",
    "srg_plan_query",
    "srg_plan_build_in",
    "srg_plan_destroy",
    "srg_plan_describe",
    "srg_plan_launch",
    "srg_plan_propagate_f32",
    "srg_plan_hop_f32",
    "srg_plan_cheby_step_f64",
    "srg_cheby_step_f64",
    "srg_cheby_step_hub_f64",
    "srg_cheby_step_f32",
    "srg_cheby_epilogue_f32",
    "srg_hop_accumulate_f32",
    "srg_hop_simweight_f32",
    "srg_row_divide_f32",
    "srg_hop_scores_f32",
    "srg_hop_attend_f32",
    "srg_hop_attend_grad_f32",
    "srg_hop_scores_grad_scratch_bytes",
    "srg_hop_scores_grad_f32",
    "srg_hop_recur_scores_f32",
    "srg_hop_recur_attend_f32",
    "srg_hop_recur_attend_grad_f32",
    "srg_hop_recur_scores_grad_scratch_bytes",
    "srg_hop_recur_scores_grad_f32",
    "srg_hop_scores_rows_f32",
    "srg_hop_attend_rows_f32",
    "srg_hop_attend_grad_rows_f32",
    "srg_hop_scores_grad_rows_f32",
    "srg_hop_recur_scores_rows_f32",
    "srg_hop_recur_attend_rows_f32",
    "srg_hop_recur_attend_grad_rows_f32",
    "srg_hop_recur_scores_grad_rows_f32",
    "srg_spmm_agg_f32",
    "srg_spmm_span_f32",
    "srg_spmm_cheby_f32",
    "srg_tail_record_f32",
    "srg_tail_rowsum_f32",
    "srg_segment_sum_f64",
    "srg_segment_sum_f32",
    "srg_segment_sum_numpy_f64",
    "srg_spmm_csr_f64",
    "srg_gather_rows_f32",
    "srg_spgemm_scratch_bytes",
    "srg_spgemm_f32",
    "srg_spgemm_grad_f32",
    "srg_spmm_muladd_f32",
    "srg_sddmm_f32",
    "srg_spmm_scaled_f32",
    "srg_sddmm_rowsum_f32",
    "srg_knn_select_f32",
    "srg_sample_distinct_i64",
    "srg_gconv_rows_f32",
    "srg_gconv_rows_adjoint_f32",
    "srg_gat_attend_f32",
    "srg_gat_edge_grad_f32",
    "srg_gat_attend_adjoint_f32",
    "srg_gat_attend_rows_f32",
    "srg_gat_edge_grad_rows_f32",
    "srg_gat_attend_rows_adjoint_f32",
    "srg_hub_join",
    "srg_hub_side_streams",
    "srg_csr_col_splits",
    "srg_csr_copy_spans",
    "srg_csr_mirror",
    "srg_csr_validate",
    "srg_csr_induced_f32",
    "srg_csr_sample_f32",
    "srg_pair_gather_add_f32",
    "srg_pair_segment_sum_f32",
    "srg_dense_sparsify_f64",
    "srg_csr_append_rows_f32",
    "srg_csr_row_normalize_l1_f32",
    "srg_comm_unique_id",
    "srg_comm_init_rank",
    "srg_comm_init_all",
    "srg_comm_destroy",
    "srg_comm_size",
    "srg_dist_propagate_khop_f32",
    "srg_halo_plan_build",
    "srg_halo_plan_destroy",
    "srg_halo_plan_info",
    "srg_halo_plan_array",
    "srg_halo_share_create",
    "srg_halo_share_destroy",
    "srg_halo_share_col_blocks",
    "srg_halo_fill_x_halo",
    "srg_halo_propagate_f32",
    "srg_comm_init_loopback",
    "srg_last_error",
    "srg_last_error_code",
    "srg_clear_error",
    "srg_version",
    "srg_debug_launch_cap",
    "srg_debug_chunk_launches",
)


class SrgError(RuntimeError):
    """A libsrgnn_hip entry point returned an error status."""


_lock = threading.Lock()
_lib = None

_p = ctypes.c_void_p
_i32 = ctypes.c_int32
_i64 = ctypes.c_int64
_u32 = ctypes.c_uint32
_f32 = ctypes.c_float
_f64 = ctypes.c_double


def _declare(lib):
    lib.srg_spmm_csr_f32.argtypes = [_p, _p, _p, _i64, _p, _i64, _i64, _p, _i64, _p, _i64, _i32, _u32, _p]
    lib.srg_spmm_csr_f32.restype = ctypes.c_int
    lib.srg_propagate_khop_f32.argtypes = [_p, _p, _p, _i64, _p, _i64, _i64, _p, _i64, _i32, _i32, _u32, _p]
    lib.srg_propagate_khop_f32.restype = ctypes.c_int
    lib.srg_propagate_plan_f32.argtypes = [_p, _i32, _i32, _p, _i64, _i32, _i32, _p]
    lib.srg_propagate_plan_f32.restype = ctypes.c_int
    lib.srg_plan_build.argtypes = [_p, _p, _p, _i64, _i32, _i32, _i32, _i64, _i64, _u32, _p, ctypes.POINTER(_p)]
    lib.srg_plan_query.argtypes = [_p, _i64, _i32, _i32, _i32, _i64, _i64, _u32, _p, ctypes.POINTER(ctypes.c_size_t),
                                   ctypes.POINTER(ctypes.c_size_t), ctypes.POINTER(_u32), ctypes.POINTER(_i32)]
    lib.srg_plan_build_in.argtypes = [_p, _p, _p, _i64, _i32, _i32, _i32, _i64, _i64, _u32, _p, ctypes.c_size_t, _p,
                                      ctypes.c_size_t, _p, ctypes.POINTER(_p)]
    lib.srg_plan_destroy.argtypes = [_p, _p]
    lib.srg_plan_describe.argtypes = [_p, _p]
    lib.srg_plan_launch.argtypes = [_p, _i32, _i32, _p, _p, _p]
    lib.srg_plan_propagate_f32.argtypes = [_p, _p, _i64, _i32, _i32, _u32, _p]
    lib.srg_plan_hop_f32.argtypes = [_p, _p, _i64, _p, _i64, _i32, _u32, _p, _i64, _f32, _i32, _p]
    lib.srg_plan_cheby_step_f64.argtypes = [_p, _p, _p, _p, _p, _i64, _i32, ctypes.c_int, _f64, _f64, _p, _p, _i32, _p,
                                            _i64, _p]
    for name in ("srg_plan_build", "srg_plan_query", "srg_plan_build_in", "srg_plan_destroy", "srg_plan_describe", "srg_plan_launch", "srg_plan_propagate_f32",
                 "srg_plan_hop_f32", "srg_plan_cheby_step_f64"):
        getattr(lib, name).restype = ctypes.c_int
    lib.srg_cheby_step_f64.argtypes = [_p, _p, _p, _i64, _p, _p, _p, _p, _i64, _i32, ctypes.c_int,
                                       _f64, _f64, _p, _p, _i32, _p, _i64, _p]
    lib.srg_cheby_step_f64.restype = ctypes.c_int
    lib.srg_cheby_step_hub_f64.argtypes = [_p, _p, _p, _i64, _p, _i64, _p, _p, _p, _i64, _i32, ctypes.c_int,
                                           _f64, _f64, _p, _p, _i32, _p, _i64, _p]
    lib.srg_cheby_step_hub_f64.restype = ctypes.c_int
    lib.srg_cheby_step_f32.argtypes = [_p, _p, _p, _i64, _p, _p, _p, _p, _i64, _i32, ctypes.c_int,
                                       _f32, _f32, _p, _p, _i32, _p, _i64, _p]
    lib.srg_cheby_step_f32.restype = ctypes.c_int
    lib.srg_cheby_epilogue_f32.argtypes = [_p, _i64, _p, _i64, _p, _i64, _i64, _i32, ctypes.c_int, _f32, _f32,
                                           _p, _p, _i32, _p, _i64, _i64, _p]
    lib.srg_cheby_epilogue_f32.restype = ctypes.c_int
    lib.srg_spmm_agg_f32.argtypes = [_p, _p, _p, _i64, _p, _i64, _i64, _p, _i64, _p, _i64, _i32, ctypes.c_uint32,
                                     _p, _i64, _f32, ctypes.c_int, _p]
    lib.srg_spmm_agg_f32.restype = ctypes.c_int
    lib.srg_spmm_span_f32.argtypes = [_p, _p, _p, _p, _i64, _p, _i64, _i64, _p, _i64, _p, _i64, _i32,
                                      ctypes.c_uint32, _p, _i64, _f32, ctypes.c_int, _p]
    lib.srg_spmm_span_f32.restype = ctypes.c_int
    lib.srg_csr_col_splits.argtypes = [_p, _p, _i64, _i64, _i32, _p, _p]
    lib.srg_csr_col_splits.restype = ctypes.c_int
    lib.srg_csr_mirror.argtypes = [_p, _p, _p, _i64, _i64, _p, _p]
    lib.srg_csr_mirror.restype = ctypes.c_int
    lib.srg_spmm_cheby_f32.argtypes = [_p, _p, _p, _i64, _p, _i64, _i64, _p, _i64, _p, _i64, _i32, ctypes.c_uint32,
                                       ctypes.c_int, _f32, _f32, _p, _i64, _p, _p, _i32, _p, _i64, _i64, _p]
    lib.srg_spmm_cheby_f32.restype = ctypes.c_int
    lib.srg_hop_accumulate_f32.argtypes = [_p, _i64, _p, _i64, _i64, _i32, _f32, ctypes.c_int, _p]
    lib.srg_hop_accumulate_f32.restype = ctypes.c_int
    lib.srg_hop_simweight_f32.argtypes = [_p, _i64, _p, _i64, _p, _p, _i64, _p, _p, _i64, _i64, _i32, _u32, _p]
    lib.srg_hop_simweight_f32.restype = ctypes.c_int
    lib.srg_row_divide_f32.argtypes = [_p, _i64, _p, _i64, _i32, _p]
    lib.srg_row_divide_f32.restype = ctypes.c_int
    lib.srg_hop_scores_f32.argtypes = [_p, _p, _i32, _i32, _i32, ctypes.c_int, _p, _p, _p, _i64, _i32, _p]
    lib.srg_hop_attend_f32.argtypes = [_p, _p, _i32, _i32, _i32, _p, ctypes.c_int, _p, _p, _i64, _i64, _i32, _p]
    lib.srg_hop_attend_grad_f32.argtypes = [_p, _p, _i32, _i32, _i32, _p, _i64, _p, _p, ctypes.c_int, _p, _p, _i64,
                                            _i32, _p]
    lib.srg_hop_scores_grad_scratch_bytes.argtypes = [_i64, _i32, _i32, _i32, ctypes.c_int, ctypes.POINTER(_i64)]
    lib.srg_hop_scores_grad_f32.argtypes = [_p, _p, _i32, _i32, _i32, ctypes.c_int, _p, _p, _p, _p, _i64, _i32, _p]
    lib.srg_hop_recur_scores_f32.argtypes = [_p, _p, _i32, _i32, _p, _p, _p, _i64, _i32, _p]
    lib.srg_hop_recur_attend_f32.argtypes = [_p, _p, _i32, _i32, _p, _p, _p, _p, _p, _p, _i64, _i64, _i32, _p]
    lib.srg_hop_recur_attend_grad_f32.argtypes = [_p, _p, _i32, _i32, _p, _i64, _p, _p, _p, _p, _i64, _i32, _p]
    lib.srg_hop_recur_scores_grad_scratch_bytes.argtypes = [_i64, _i32, _i32, ctypes.POINTER(_i64)]
    lib.srg_hop_recur_scores_grad_f32.argtypes = [_p, _p, _i32, _i32, _p, _p, _p, _p, _p, _i64, _i32, _p]
    for name in ("srg_hop_scores_f32", "srg_hop_attend_f32", "srg_hop_attend_grad_f32",
                 "srg_hop_scores_grad_scratch_bytes", "srg_hop_scores_grad_f32",
                 "srg_hop_recur_scores_f32", "srg_hop_recur_attend_f32", "srg_hop_recur_attend_grad_f32",
                 "srg_hop_recur_scores_grad_scratch_bytes", "srg_hop_recur_scores_grad_f32"):
        getattr(lib, name).restype = ctypes.c_int
    # the row-indexed twins: the base entry's arguments with (rows, n_src) after ldp
    for name in ("srg_hop_scores_f32", "srg_hop_attend_f32", "srg_hop_attend_grad_f32", "srg_hop_scores_grad_f32",
                 "srg_hop_recur_scores_f32", "srg_hop_recur_attend_f32", "srg_hop_recur_attend_grad_f32",
                 "srg_hop_recur_scores_grad_f32"):
        twin = getattr(lib, name.replace("_f32", "_rows_f32"))
        base = getattr(lib, name).argtypes
        twin.argtypes = list(base[:2]) + [_p, _i64] + list(base[2:])
        twin.restype = ctypes.c_int
    lib.srg_tail_record_f32.argtypes = [_p, _p, _i64, _i32, _i64, _i32, _f32, _p]
    lib.srg_tail_record_f32.restype = ctypes.c_int
    lib.srg_tail_rowsum_f32.argtypes = [_p, _i64, _i32, _i64, _i32, _p, _i32, _p]
    lib.srg_tail_rowsum_f32.restype = ctypes.c_int
    lib.srg_segment_sum_f64.argtypes = [_p, _p, _i64, _p, _p]
    lib.srg_segment_sum_f64.restype = ctypes.c_int
    lib.srg_segment_sum_f32.argtypes = [_p, _p, _i64, _p, _p]
    lib.srg_segment_sum_f32.restype = ctypes.c_int
    lib.srg_segment_sum_numpy_f64.argtypes = [_p, _p, _i64, _p, _p]
    lib.srg_segment_sum_numpy_f64.restype = ctypes.c_int
    lib.srg_spmm_csr_f64.argtypes = [_p, _p, _p, _i64, _p, _i64, _p, _i64, _i32, _p]
    lib.srg_spmm_csr_f64.restype = ctypes.c_int
    lib.srg_gather_rows_f32.argtypes = [_p, _i64, _i64, _p, _i64, _p, _i64, _i32, _p]
    lib.srg_gather_rows_f32.restype = ctypes.c_int
    lib.srg_spgemm_scratch_bytes.argtypes = [_i64, _i64, ctypes.POINTER(_i64)]
    lib.srg_spgemm_scratch_bytes.restype = ctypes.c_int
    lib.srg_spgemm_f32.argtypes = [ctypes.c_int, _p, _p, _p, _i64, _p, _p, _p, _i64, _p, _p, _p, _p, _p, _i64,
                                   _u32, _p]
    lib.srg_spgemm_f32.restype = ctypes.c_int
    lib.srg_spgemm_grad_f32.argtypes = [_p, _p, _i64, _p, _p, _p, _p, _p, _p, _i64, _p, _p, _i64, _p]
    lib.srg_spgemm_grad_f32.restype = ctypes.c_int
    lib.srg_spmm_muladd_f32.argtypes = [_p, _p, _p, _i64, _p, _i64, _p, _i64, _i32, _p]
    lib.srg_spmm_muladd_f32.restype = ctypes.c_int
    lib.srg_sddmm_f32.argtypes = [_p, _p, _i64, _i64, _p, _i64, _p, _i64, _i32, _p, _p, _p]
    lib.srg_sddmm_f32.restype = ctypes.c_int
    lib.srg_spmm_scaled_f32.argtypes = [_p, _p, _p, _p, _i32, _i64, _p, _i64, _p, _i64, _i32, _p]
    lib.srg_spmm_scaled_f32.restype = ctypes.c_int
    lib.srg_sddmm_rowsum_f32.argtypes = [_p, _p, _p, _i64, _p, _i64, _p, _i64, _i32, _p, _p]
    lib.srg_sddmm_rowsum_f32.restype = ctypes.c_int
    lib.srg_knn_select_f32.argtypes = [_p, _i64, _i64, _i32, _p, _p, _p, _p, _i64, _p, _p, _p]
    lib.srg_knn_select_f32.restype = ctypes.c_int
    lib.srg_sample_distinct_i64.argtypes = [_p, _p, _i64, _i64, ctypes.c_uint64, _p, _p]
    lib.srg_sample_distinct_i64.restype = ctypes.c_int
    lib.srg_gconv_rows_f32.argtypes = [_p, _p, _p, _i64, _p, _i64, _p, _i64, _p, _i64, _i32, _p]
    lib.srg_gconv_rows_f32.restype = ctypes.c_int
    lib.srg_gconv_rows_adjoint_f32.argtypes = [_p, _p, _p, _i64, _p, _i64, _p, _i64, _p, _i64, _i32, _p]
    lib.srg_gconv_rows_adjoint_f32.restype = ctypes.c_int
    lib.srg_gat_attend_f32.argtypes = [_p, _p, _i64, _i64, _i64, _p, _p, _f32, _p, _i64, _i32, _i32, _p, _i64, _p, _p, _p]
    lib.srg_gat_attend_f32.restype = ctypes.c_int
    lib.srg_gat_edge_grad_f32.argtypes = [_p, _p, _i64, _i64, _i64, _p, _p, _f32, _p, _i64, _i32, _i32, _p, _i64, _p, _p,
                                          _p, _i64, _p, _p, _p, _p]
    lib.srg_gat_edge_grad_f32.restype = ctypes.c_int
    lib.srg_gat_attend_adjoint_f32.argtypes = [_p, _p, _p, _i64, _i64, _i64, _p, _p, _f32, _i32, _i32, _p, _p, _p, _i64,
                                               _p, _p, _i64, _p, _p]
    lib.srg_gat_attend_adjoint_f32.restype = ctypes.c_int
    lib.srg_gat_attend_rows_f32.argtypes = [_p, _p, _i64, _i64, _i64, _p, _i64, _p, _p, _f32, _p, _i64, _i32, _i32, _p,
                                            _i64, _p, _p, _p]
    lib.srg_gat_attend_rows_f32.restype = ctypes.c_int
    lib.srg_gat_edge_grad_rows_f32.argtypes = [_p, _p, _i64, _i64, _i64, _p, _i64, _p, _i64, _p, _p, _f32, _p, _i64, _i32,
                                               _i32, _p, _i64, _p, _p, _p, _i64, _p, _p, _p, _p]
    lib.srg_gat_edge_grad_rows_f32.restype = ctypes.c_int
    lib.srg_gat_attend_rows_adjoint_f32.argtypes = [_p, _p, _p, _i64, _i64, _i64, _p, _i64, _p, _p, _i64, _p, _p, _f32,
                                                    _i32, _i32, _p, _p, _p, _i64, _p, _p, _i64, _p, _p]
    lib.srg_gat_attend_rows_adjoint_f32.restype = ctypes.c_int
    lib.srg_hub_join.argtypes = [_p]
    lib.srg_hub_join.restype = ctypes.c_int
    lib.srg_hub_side_streams.argtypes = []
    lib.srg_hub_side_streams.restype = ctypes.c_int
    lib.srg_csr_validate.argtypes = [_p, _p, _i64, _i64, _i64, _p]
    lib.srg_csr_validate.restype = ctypes.c_int
    lib.srg_csr_induced_f32.argtypes = [ctypes.c_int, _p, _p, _p, _i64, _i64, _p, _i64, _p, _p, _p, _p, _p, _p, _p]
    lib.srg_csr_induced_f32.restype = ctypes.c_int
    lib.srg_csr_sample_f32.argtypes = [_p, _p, _p, _i64, _p, _i64, _i32, ctypes.c_uint64, _p, _p, _p, _p, _p]
    lib.srg_csr_sample_f32.restype = ctypes.c_int
    lib.srg_pair_gather_add_f32.argtypes = [_p, _i64, _i64, _p, _p, _i64, _i32, _p, _i64, _p]
    lib.srg_pair_gather_add_f32.restype = ctypes.c_int
    lib.srg_pair_segment_sum_f32.argtypes = [_p, _i64, _i64, _p, _p, _i64, _i32, _p, _i64, _p]
    lib.srg_pair_segment_sum_f32.restype = ctypes.c_int
    lib.srg_dense_sparsify_f64.argtypes = [ctypes.c_int, _p, _i64, _i64, _i32, _f64, _i32, _p, _p, _p, _p, _p]
    lib.srg_dense_sparsify_f64.restype = ctypes.c_int
    lib.srg_csr_append_rows_f32.argtypes = [_p, _p, _p, _i64, _p, _p, _p, _p]
    lib.srg_csr_append_rows_f32.restype = ctypes.c_int
    lib.srg_csr_row_normalize_l1_f32.argtypes = [_p, _p, _i64, _p]
    lib.srg_csr_row_normalize_l1_f32.restype = ctypes.c_int
    lib.srg_comm_unique_id.argtypes = [_p]
    lib.srg_comm_unique_id.restype = ctypes.c_int
    lib.srg_comm_init_rank.argtypes = [ctypes.c_int, _p, ctypes.c_int, ctypes.c_int, ctypes.POINTER(_p)]
    lib.srg_comm_init_rank.restype = ctypes.c_int
    lib.srg_comm_init_all.argtypes = [ctypes.c_int, _p, ctypes.POINTER(_p)]
    lib.srg_comm_init_all.restype = ctypes.c_int
    lib.srg_comm_destroy.argtypes = [_p]
    lib.srg_comm_destroy.restype = ctypes.c_int
    lib.srg_comm_size.argtypes = [_p]
    lib.srg_comm_size.restype = ctypes.c_int
    lib.srg_dist_propagate_khop_f32.argtypes = [_p, _p, ctypes.c_int, _p, _i64, _i32, _i32]
    lib.srg_dist_propagate_khop_f32.restype = ctypes.c_int
    lib.srg_csr_copy_spans.argtypes = [_p, _i64, _p, _p, _p, _p, _p, _p, _p, _p, _p, _p]
    lib.srg_csr_copy_spans.restype = ctypes.c_int
    lib.srg_halo_plan_build.argtypes = [_p, _p, _i64, _i32, _i32, _i32, _i64, _i64, _i32, _f64, ctypes.POINTER(_p)]
    lib.srg_halo_plan_destroy.argtypes = [_p]
    lib.srg_halo_plan_info.argtypes = [_p, ctypes.POINTER(HaloInfo)]
    lib.srg_halo_plan_array.argtypes = [_p, _i32, _i32, ctypes.POINTER(_p), ctypes.POINTER(_i64)]
    lib.srg_halo_share_create.argtypes = [_p, _p, ctypes.c_int, _i32, ctypes.POINTER(_p)]
    lib.srg_halo_share_destroy.argtypes = [_p]
    lib.srg_halo_share_col_blocks.argtypes = [_p, _i32]
    lib.srg_halo_fill_x_halo.argtypes = [_p, _p, _i64, _p, _i64, _i32, _p]
    lib.srg_halo_propagate_f32.argtypes = [_p, _p, ctypes.c_int, _p, _i64, _i32, _i32, _u32, _p]
    lib.srg_comm_init_loopback.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.POINTER(_p)]
    for name in ("srg_halo_plan_build", "srg_halo_plan_destroy", "srg_halo_plan_info", "srg_halo_plan_array",
                 "srg_halo_share_create", "srg_halo_share_destroy", "srg_halo_share_col_blocks", "srg_halo_fill_x_halo", "srg_halo_propagate_f32",
                 "srg_comm_init_loopback"):
        getattr(lib, name).restype = ctypes.c_int
    lib.srg_last_error.argtypes = []
    lib.srg_last_error.restype = ctypes.c_char_p
    lib.srg_last_error_code.argtypes = []
    lib.srg_last_error_code.restype = ctypes.c_int
    lib.srg_clear_error.argtypes = []
    lib.srg_clear_error.restype = None
    lib.srg_version.argtypes = []
    lib.srg_version.restype = ctypes.c_char_p
    lib.srg_debug_launch_cap.argtypes = [_i64]
    lib.srg_debug_launch_cap.restype = _i64
    lib.srg_debug_chunk_launches.argtypes = []
    lib.srg_debug_chunk_launches.restype = _i64
    lib.FloatCSRMulDense.restype = ctypes.c_int
    return lib


def lib():
    """The loaded library (loaded once).  Raises OSError with the build hint if it is missing."""
    global _lib
    if _lib is not None:
        return _lib
    with _lock:
        if _lib is None:
            if not os.path.exists(LIB_PATH):
                raise OSError(
                    f"libsrgnn_hip.so not found at {LIB_PATH}: build it with "
                    f"`make -C scalable-roubust-gnn_amd/csrc` or `python -c 'import __graft_entry__ as g; g.build()'`"
                )
            _lib = _declare(ctypes.CDLL(LIB_PATH))
    return _lib


def last_error() -> str:
    return lib().srg_last_error().decode(errors="replace")


def check(rc: int, what: str) -> None:
    if rc != SRG_OK:
        raise SrgError(f"{what} failed ({rc}): {last_error()}")


def stream(device) -> int:
    """torch's current HIP stream of `device` as the C-ABI's stream argument (0 = the null stream,
    i.e. that of the CURRENT device: run the call under on_device(device), as call() does)."""
    return torch.cuda.current_stream(device).cuda_stream


def call(device, name: str, *args) -> None:
    """Runs entry point `name` with `device` current (the library resolves its side streams and
    the null stream from the current device) and raises SrgError on a failed status."""
    fn = getattr(lib(), name)
    device = torch.device(device)
    if device.index is not None and device.index != torch.cuda.current_device():
        with torch.cuda.device(device):
            check(fn(*args), name)
    else:
        check(fn(*args), name)


class hub_forked:
    """A hub group forked onto the library's hub side stream of `device`'s current stream: the block
    launches the hub rows unjoined (HUB_NOJOIN) and whatever runs beside them; leaving it, normally or
    by an exception, joins the side stream into the current stream (srg_hub_join), so hub rows are
    never left running unjoined.  join() joins early; leaving the block is then a no-op.  on=False:
    the caller forked nothing, and nothing is joined."""

    def __init__(self, device, on: bool = True):
        self.device = device
        self._open = bool(on)

    def __enter__(self):
        return self

    def join(self) -> None:
        if self._open:
            self._open = False
            call(self.device, "srg_hub_join", stream(self.device))

    def __exit__(self, *exc):
        self.join()
        return False


class launch_cap:
    """Test hook (srg_debug_launch_cap): inside the block no launch of the library has more than `n` blocks,
    so chunked launches go out in several chunks and grid-stride kernels take several trips -- the same
    results, scheduled differently.  Leaving the block, normally or by an exception, restores the bound
    that held before; `launches` is then the number of chunk launches made inside it
    (srg_debug_chunk_launches; `launches` reads the running count while the block is open)."""

    def __init__(self, n: int):
        self.n = int(n)
        self._start = self._end = None
        self._prev = 0

    def __enter__(self):
        self._start = lib().srg_debug_chunk_launches()
        self._prev = lib().srg_debug_launch_cap(self.n)
        return self

    @property
    def launches(self) -> int:
        end = self._end if self._end is not None else lib().srg_debug_chunk_launches()
        return end - self._start

    def __exit__(self, *exc):
        try:
            self._end = lib().srg_debug_chunk_launches()
        finally:
            lib().srg_debug_launch_cap(self._prev)
        return False


def call_host(name: str, *args) -> None:
    """Entry points that choose their devices themselves (srg_comm_*, srg_dist_propagate_khop_f32:
    every shard names its device) -- no device guard; raises SrgError on a failed status."""
    check(getattr(lib(), name)(*args), name)


def query(name: str, *args) -> int:
    """An entry point that returns a value, not a status (srg_comm_size)."""
    return getattr(lib(), name)(*args)


def version() -> str:
    return lib().srg_version().decode()
