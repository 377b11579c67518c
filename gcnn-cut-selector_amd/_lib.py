"""ctypes binding of libgcnn_hip.so (C ABI declared in include/gcnn_hip.h).

The product path has NO fallback: if the shared library is missing or a call fails, an exception is raised."""

from __future__ import annotations

import ctypes as C
import os

# Kernel arguments in device memory: with them in host memory every launch of this library (argument blocks of 1-3 KB) pays
# PCIe round trips -- measured +0.1 ms per training step.  Must be set before the HIP runtime initialises; this image
# already defaults to 1, so this only guards against an environment that does not.
os.environ.setdefault("HIP_FORCE_DEV_KERNARG", "1")

import torch  # noqa: F401  -- MUST be imported before the CDLL below: torch ships its own libamdhip64; loading ours first
#                              would register the kernels with a second HIP runtime (hipErrorNoDevice at first launch)

LIB_PATH = os.environ.get("GCNN_LIB") or os.path.join(os.path.dirname(os.path.abspath(__file__)), "csrc", "libgcnn_hip.so")  # GCNN_LIB: A/B builds
ABI_VERSION = 13


class GcnnError(RuntimeError):
    pass


class Dims(C.Structure):
    _fields_ = [("n_cons", C.c_int32), ("n_vars", C.c_int32), ("n_cuts", C.c_int32),
                ("n_cons_edges", C.c_int32), ("n_cut_edges", C.c_int32)]


class Graph(C.Structure):
    _fields_ = [("l_ptr", C.c_void_p), ("l_oth", C.c_void_p), ("l_coef", C.c_void_p),
                ("v_ptr", C.c_void_p), ("v_oth", C.c_void_p), ("v_coef", C.c_void_p),
                ("l_max_deg", C.c_int32), ("v_max_deg", C.c_int32)]


class AdamArgs(C.Structure):
    _fields_ = [("params", C.c_void_p), ("m", C.c_void_p), ("v", C.c_void_p), ("lr_t", C.c_float), ("beta1", C.c_float),
                ("beta2", C.c_float), ("eps", C.c_float)]


class InferLayout(C.Structure):
    _fields_ = [("in_bytes", C.c_size_t), ("in_off", C.c_size_t * 8), ("out_bytes", C.c_size_t), ("out_off", C.c_size_t * 3),
                ("arena_bytes", C.c_size_t), ("dev_off", C.c_size_t * 8)]


class SelectLayout(C.Structure):
    _fields_ = [("infer", InferLayout), ("forced_off", C.c_size_t * 3), ("n_kept_off", C.c_size_t), ("ws_off", C.c_size_t)]


IBATCH_MAX, IBATCH_TABLE_COLS, IBATCH_TABLE_STRIDE = 64, 7, 72   # GCNN_IBATCH_*
IBATCH_SCORES, IBATCH_RANK, IBATCH_SELECT = 0, 1, 2


class IbatchLayout(C.Structure):
    _fields_ = [("total", Dims), ("n_forced", C.c_int32), ("n_forced_entries", C.c_int32), ("max_cuts", C.c_int32),
                ("n_states", C.c_int32), ("in_bytes", C.c_size_t), ("in_off", C.c_size_t * 12), ("out_bytes", C.c_size_t),
                ("out_off", C.c_size_t * 4), ("arena_bytes", C.c_size_t), ("dev_off", C.c_size_t * 16)]


class GroupMember(C.Structure):
    _fields_ = [("dims", Dims), ("params", C.c_void_p), ("cons_feats", C.c_void_p), ("var_feats", C.c_void_p),
                ("cut_feats", C.c_void_p), ("cons_graph", Graph), ("cut_graph", Graph), ("workspace", C.c_void_p),
                ("workspace_floats", C.c_size_t), ("scores", C.c_void_p), ("targets", C.c_void_p), ("loss_scale", C.c_float),
                ("grads", C.c_void_p), ("loss_out", C.c_void_p), ("adam", C.POINTER(AdamArgs))]


class LpDims(C.Structure):
    _fields_ = [("n_rows", C.c_int32), ("n_cols", C.c_int32), ("n_cuts", C.c_int32), ("row_nnz", C.c_int32), ("cut_nnz", C.c_int32),
                ("has_incumbent", C.c_int32), ("n_model_vars", C.c_int32), ("n_state_rows", C.c_int32),
                ("n_state_edges", C.c_int32), ("reserved", C.c_int32), ("infinity", C.c_double), ("sum_epsilon", C.c_double),
                ("obj_norm", C.c_double)]


LP_ARRAYS = 22   # GCNN_LP_ARRAYS


class LpLayout(C.Structure):
    _fields_ = [("snap_bytes", C.c_size_t), ("snap_off", C.c_size_t * LP_ARRAYS), ("scratch_bytes", C.c_size_t),
                ("call_supported", C.c_int32), ("reserved", C.c_int32), ("in_bytes", C.c_size_t), ("forced_off", C.c_size_t * 3),
                ("out_bytes", C.c_size_t), ("out_off", C.c_size_t * 6), ("arena_bytes", C.c_size_t), ("ws_off", C.c_size_t),
                ("lp_off", C.c_size_t), ("scratch_off", C.c_size_t), ("state", InferLayout)]


class LpBatchLayout(C.Structure):
    _fields_ = [("state", IbatchLayout), ("n_snapshots", C.c_int32), ("reserved", C.c_int32), ("table_bytes", C.c_size_t),
                ("in_bytes", C.c_size_t), ("snap_base", C.c_size_t * IBATCH_MAX), ("forced_off", C.c_size_t * 3),
                ("out_bytes", C.c_size_t), ("out_off", C.c_size_t * 6), ("arena_bytes", C.c_size_t), ("up_off", C.c_size_t),
                ("out_dev_off", C.c_size_t), ("scratch_off", C.c_size_t), ("scratch_base", C.c_size_t * IBATCH_MAX)]


HYBRID_ARRAYS = 8   # GCNN_HYBRID_ARRAYS
HYBRID_QUALITY, HYBRID_RANK, HYBRID_SELECT = 0, 1, 2


class HybridDims(C.Structure):
    _fields_ = [("n_cols", C.c_int32), ("n_cuts", C.c_int32), ("cut_nnz", C.c_int32), ("reserved", C.c_int32), ("infinity", C.c_double)]


class HybridLayout(C.Structure):
    _fields_ = [("n_snapshots", C.c_int32), ("total_cuts", C.c_int32), ("total_nnz", C.c_int32), ("max_cuts", C.c_int32),
                ("max_cols", C.c_int32), ("n_forced", C.c_int32), ("n_forced_entries", C.c_int32), ("reserved", C.c_int32),
                ("table_bytes", C.c_size_t), ("in_bytes", C.c_size_t), ("snap_off", (C.c_size_t * HYBRID_ARRAYS) * IBATCH_MAX),
                ("forced_off", C.c_size_t * 3), ("out_bytes", C.c_size_t), ("out_off", C.c_size_t * 5), ("arena_bytes", C.c_size_t),
                ("out_dev_off", C.c_size_t), ("rows_off", C.c_size_t * 3), ("ws_off", C.c_size_t), ("scratch_off", C.c_size_t),
                ("scratch_base", C.c_size_t * IBATCH_MAX)]


LP_COLLECT_OUTPUTS = 14   # GCNN_LP_COLLECT_OUTPUTS


class LpCollectLayout(C.Structure):
    _fields_ = [("in_bytes", C.c_size_t), ("snap_off", C.c_size_t * LP_ARRAYS), ("quality_off", C.c_size_t),
                ("forced_off", C.c_size_t * 3), ("table_off", C.c_size_t), ("table_bytes", C.c_size_t), ("out_bytes", C.c_size_t),
                ("out_off", C.c_size_t * LP_COLLECT_OUTPUTS), ("arena_bytes", C.c_size_t), ("out_dev_off", C.c_size_t),
                ("rows_off", C.c_size_t * 3), ("ws_off", C.c_size_t), ("lp_scratch_off", C.c_size_t),
                ("hyb_scratch_off", C.c_size_t), ("entry_snap", C.c_size_t * HYBRID_ARRAYS)]


GROUP_MAX = 8   # GCNN_GROUP_MAX
MBATCH_HEAD = 16                                                              # model words in front of the states' models
MBATCH_TABLE_WORDS = IBATCH_TABLE_COLS * IBATCH_TABLE_STRIDE + MBATCH_HEAD + IBATCH_MAX   # GCNN_MBATCH_TABLE_WORDS


class MbatchLayout(C.Structure):
    _fields_ = [("u", IbatchLayout), ("n_models", C.c_int32), ("first_state", C.c_int32 * (GROUP_MAX + 1)),
                ("model", Dims * GROUP_MAX), ("ws_off", C.c_size_t * GROUP_MAX), ("table_off", C.c_size_t),
                ("table_bytes", C.c_size_t)]


class LpModelsLayout(C.Structure):
    _fields_ = [("models", MbatchLayout), ("lp", LpBatchLayout)]   # lp.state == models.u


class EnsembleLayout(C.Structure):
    _fields_ = [("u", IbatchLayout), ("n_models", C.c_int32), ("reserved", C.c_int32), ("member_off", C.c_size_t),
                ("member_stride", C.c_size_t), ("ws_off", C.c_size_t * GROUP_MAX), ("table_off", C.c_size_t),
                ("table_bytes", C.c_size_t)]


class LpEnsembleLayout(C.Structure):
    _fields_ = [("ens", EnsembleLayout), ("lp", LpBatchLayout)]   # lp.state == ens.u


LPR_LB, LPR_UB, LPR_PRIMAL, LPR_PRIMAL_AVG = 1, 2, 4, 8      # GCNN_LPR_*: the optional column arrays a round carries
LPR_DERIVED, LPR_ARRAYS, LPR_BLOCKS = 7, 15, 11             # GCNN_LPR_DERIVED, GCNN_LPR_ARRAYS, GCNN_LPR_BLOCKS


class LpRowsLayout(C.Structure):
    _fields_ = [("bytes", C.c_size_t), ("off", C.c_size_t * LPR_DERIVED)]


class LpResident(C.Structure):
    _fields_ = [("row_place", C.c_void_p), ("row_scale", C.c_void_p), ("cons_feats", C.c_void_p), ("col_type", C.c_void_p),
                ("col_obj", C.c_void_p), ("col_lb", C.c_void_p), ("col_ub", C.c_void_p), ("col_primal", C.c_void_p),
                ("col_primal_avg", C.c_void_p), ("cons_graph", Graph)]


class LpRoundLayout(C.Structure):
    _fields_ = [("in_bytes", C.c_size_t), ("in_off", C.c_size_t * LPR_ARRAYS), ("forced_off", C.c_size_t * 3),
                ("out_bytes", C.c_size_t), ("out_off", C.c_size_t * 6), ("arena_bytes", C.c_size_t),
                ("dev_off", C.c_size_t * LPR_BLOCKS)]


class LpAppendDims(C.Structure):
    _fields_ = [("n_rows", C.c_int32), ("row_nnz", C.c_int32), ("n_state_rows", C.c_int32), ("n_state_edges", C.c_int32),
                ("n_lhs_rows", C.c_int32), ("n_lhs_edges", C.c_int32), ("res_lhs_rows", C.c_int32), ("res_lhs_edges", C.c_int32)]


LP_SET_FIELDS = ("cons_feats", "edge_row", "edge_col", "edge_coef", "l_ptr", "v_ptr", "v_oth", "v_coef", "row_place", "row_scale")


class LpRowsSet(C.Structure):
    _fields_ = [(name, C.c_void_p) for name in LP_SET_FIELDS]


class LpAppendLayout(C.Structure):
    _fields_ = [("block_bytes", C.c_size_t), ("block_off", C.c_size_t * 5), ("in_bytes", C.c_size_t), ("out_bytes", C.c_size_t),
                ("flags_off", C.c_size_t), ("scratch_bytes", C.c_size_t), ("arena_bytes", C.c_size_t), ("round_off", C.c_size_t),
                ("scratch_off", C.c_size_t), ("round", LpRoundLayout)]


class LpRemoveDims(C.Structure):
    _fields_ = list(LpAppendDims._fields_)     # the same eight counts, of the removed rows


class LpRemoveLayout(C.Structure):
    _fields_ = [("list_bytes", C.c_size_t), ("block_bytes", C.c_size_t), ("block_off", C.c_size_t * 5), ("in_bytes", C.c_size_t),
                ("out_bytes", C.c_size_t), ("flags_off", C.c_size_t), ("append_flags_off", C.c_size_t), ("scratch_bytes", C.c_size_t),
                ("arena_bytes", C.c_size_t), ("round_off", C.c_size_t), ("append_scratch_off", C.c_size_t), ("scratch_off", C.c_size_t),
                ("round", LpRoundLayout)]


LP_ROUNDS_MAX = GROUP_MAX   # GCNN_LP_ROUNDS_MAX


class LpRoundsMember(C.Structure):
    _fields_ = [("dims", LpDims), ("present", C.c_int32), ("n_forced", C.c_int32), ("n_forced_entries", C.c_int32),
                ("has_append", C.c_int32), ("block", LpAppendDims), ("row_ptr", C.c_void_p), ("row_col", C.c_void_p),
                ("row_val", C.c_void_p), ("row_lhs", C.c_void_p), ("row_rhs", C.c_void_p), ("src", C.POINTER(LpRowsSet)),
                ("dst", C.POINTER(LpRowsSet)), ("resident", C.POINTER(LpResident)), ("params", C.c_void_p)]


class LpRoundsLayout(C.Structure):
    _fields_ = [("n", C.c_int32), ("mode", C.c_int32), ("in_bytes", C.c_size_t), ("in_off", C.c_size_t * LP_ROUNDS_MAX),
                ("in_size", C.c_size_t * LP_ROUNDS_MAX), ("arena_off", C.c_size_t * LP_ROUNDS_MAX),
                ("member_round_off", C.c_size_t * LP_ROUNDS_MAX), ("scratch_off", C.c_size_t * LP_ROUNDS_MAX),
                ("counts_base", C.c_size_t), ("counts_bytes", C.c_size_t), ("counts_off", C.c_size_t * LP_ROUNDS_MAX),
                ("out_base", C.c_size_t), ("out_bytes", C.c_size_t), ("out_off", C.c_size_t * LP_ROUNDS_MAX),
                ("out_size", C.c_size_t * LP_ROUNDS_MAX), ("table_off", C.c_size_t), ("table_bytes", C.c_size_t),
                ("arena_bytes", C.c_size_t)]


class LpRoundsEditMember(C.Structure):      # gcnn_lp_rounds_edit_member: LpRoundsMember's fields, then the removal's
    _fields_ = list(LpRoundsMember._fields_) + [
        ("has_remove", C.c_int32), ("reserved", C.c_int32), ("removed", LpRemoveDims), ("out_ptr", C.c_void_p), ("out_col", C.c_void_p),
        ("out_val", C.c_void_p), ("out_lhs", C.c_void_p), ("out_rhs", C.c_void_p), ("transit", C.POINTER(LpRowsSet))]


class LpRoundsEditLayout(C.Structure):
    _fields_ = [("n", C.c_int32), ("mode", C.c_int32), ("in_bytes", C.c_size_t), ("in_off", C.c_size_t * LP_ROUNDS_MAX),
                ("in_size", C.c_size_t * LP_ROUNDS_MAX), ("arena_off", C.c_size_t * LP_ROUNDS_MAX),
                ("member_round_off", C.c_size_t * LP_ROUNDS_MAX), ("scratch_off", C.c_size_t * LP_ROUNDS_MAX),
                ("remove_scratch_off", C.c_size_t * LP_ROUNDS_MAX), ("counts_base", C.c_size_t), ("counts_bytes", C.c_size_t),
                ("counts_off", C.c_size_t * LP_ROUNDS_MAX), ("remove_counts_off", C.c_size_t * LP_ROUNDS_MAX),
                ("out_base", C.c_size_t), ("out_bytes", C.c_size_t), ("out_off", C.c_size_t * LP_ROUNDS_MAX),
                ("out_size", C.c_size_t * LP_ROUNDS_MAX), ("table_off", C.c_size_t), ("table_bytes", C.c_size_t),
                ("arena_bytes", C.c_size_t)]


class LpRoundEnsembleLayout(C.Structure):   # gcnn_lp_round_ensemble_layout: the solo round's layout, then where the ensemble's pieces lie
    _fields_ = [("round", LpRoundLayout), ("n_models", C.c_int32), ("reserved", C.c_int32), ("in_bytes", C.c_size_t),
                ("out_bytes", C.c_size_t), ("solo_out_bytes", C.c_size_t), ("flags_off", C.c_size_t), ("append_flags_off", C.c_size_t),
                ("member_off", C.c_size_t), ("member_stride", C.c_size_t), ("arena_bytes", C.c_size_t), ("solo_arena_bytes", C.c_size_t),
                ("round_off", C.c_size_t), ("out_base", C.c_size_t), ("ws_off", C.c_size_t * GROUP_MAX), ("table_off", C.c_size_t),
                ("table_bytes", C.c_size_t)]


# gcnn_prenorm_merge's state: fp32 count at byte 0, mean [units] and var [units] at these byte offsets
PRENORM_STATE_BYTES, PRENORM_STATE_MEAN, PRENORM_STATE_VAR = 272, 16, 80   # GCNN_PRENORM_STATE_*


class CollateJob(C.Structure):
    _fields_ = [("src", C.c_void_p), ("dst", C.c_void_p), ("unit_kind", C.c_int32), ("width", C.c_int32),
                ("add_kind", C.c_int32), ("is_ptr", C.c_int32)]


_P, _I, _F, _Z, _D = C.c_void_p, C.c_int32, C.c_float, C.c_size_t, C.c_double
_DP, _GP = C.POINTER(Dims), C.POINTER(Graph)

# name -> (restype, argtypes); every symbol include/gcnn_hip.h declares
SIGNATURES = {
    "gcnn_abi_version": (C.c_int, []),
    "gcnn_profile_begin": (C.c_int, []),
    "gcnn_profile_end": (C.c_int, [_I, C.POINTER(C.c_char_p), C.POINTER(C.c_float)]),
    "gcnn_param_count": (C.c_int, []),
    "gcnn_param_total_floats": (C.c_int, []),
    "gcnn_param_info": (C.c_int, [C.c_int] + [C.POINTER(C.c_int)] * 4),
    "gcnn_graph_temp_bytes": (_Z, [_I]),
    "gcnn_graph_check": (C.c_int, [_P, _I, _I, _I, _P, _P]),
    "gcnn_collate": (C.c_int, [_P, _I, _P, _P, _I, C.c_int64, _P]),
    "gcnn_graph_build": (C.c_int, [_P, _P, _I, _I, _I, _I, _P, _P, _P, _P, _P, _P, _P, _P, _Z, _P]),
    "gcnn_seg_sum_f32": (C.c_int, [_P, _P, _P, _I, _P, _P]),
    "gcnn_seg_bcast_f32": (C.c_int, [_P, _P, _P, _I, _P, _P]),
    "gcnn_linear_fwd": (C.c_int, [_P, _P, _P, _P, _P, _P, _P, _P, _I, _P, _I, _P]),
    "gcnn_linear_bwd": (C.c_int, [_P, _P, _P, _P, _P, _I, _P, _P, _I, _I, _P]),
    "gcnn_conv_edge_fwd": (C.c_int, [_P, _P, _P, _I, _I, _P, _P, _P, _P, _P, _P, _P, _P, _I, _P]),
    "gcnn_conv_edge_bwd_recv": (C.c_int, [_P, _P, _P, _I, _P, _P]),
    "gcnn_conv_edge_bwd_send": (C.c_int, [_P, _P, _P, _I, _I, _P, _P, _P, _P, _P, _P, _P, _P, _P, C.POINTER(C.c_int32), _I, _P]),
    "gcnn_workspace_floats": (_Z, [_DP]),
    "gcnn_forward": (C.c_int, [_DP, _P, _P, _P, _P, _GP, _GP, _P, _Z, _P, _I, _P]),
    "gcnn_infer_layout_for": (C.c_int, [_DP, C.POINTER(InferLayout)]),
    "gcnn_infer": (C.c_int, [_DP, _P, _P, _P, _P, _Z, _I, _P]),
    "gcnn_mse_loss": (C.c_int, [_P, _P, _I, _F, _P, _P, _P]),
    "gcnn_forward_loss": (C.c_int, [_DP, _P, _P, _P, _P, _GP, _GP, _P, _Z, _P, _P, _F, _P]),
    "gcnn_backward": (C.c_int, [_DP, _P, _P, _P, _P, _GP, _GP, _P, _Z, _P, _P, _P, _P, _P, _P]),
    "gcnn_prenorm_stats": (C.c_int, [_DP, _P, _P, _P, _P, _GP, _GP, _P, _Z, _I, _P, _P]),
    "gcnn_adam_step": (C.c_int, [_P, _P, _P, _P, _I, _F, _F, _F, _F, _P, _I, _P]),
    "gcnn_ranking_metric": (C.c_int, [_P, _P, _P, _I, _I, _P, _I, _P, _P, _P, _F, _P, _P]),
    "gcnn_adam_step_dev": (C.c_int, [_P, _P, _P, _P, _I, _P, _P, _I, _P]),
    "gcnn_host_sort_edges_by_row": (C.c_int, [_P, _P, _P, _I, _I, _P, _P, _P]),
    "gcnn_host_pack_edges": (C.c_int, [_P, _P, _P, _I, _I, _P, _P, _P]),
    "gcnn_select_workspace_bytes": (_Z, [_I, _I, _I]),
    "gcnn_select_cuts": (C.c_int, [_P, _P, _P, _P, _P, _I, _I, _I, _I, _P, _P, _P, _P, _I, _D, _D, _P, _P, _P, _Z, _P]),
    "gcnn_infer_select_layout_for": (C.c_int, [_DP, _I, _I, C.POINTER(SelectLayout)]),
    "gcnn_infer_select": (C.c_int, [_DP, _I, _I, _P, _P, _P, _P, _Z, _D, _D, _P]),
    "gcnn_group_table_bytes": (C.c_int, [_I, C.POINTER(C.c_size_t)]),
    "gcnn_group_train_step": (C.c_int, [_I, C.POINTER(GroupMember), _P, _P, _Z, _P]),
    "gcnn_group_forward": (C.c_int, [_I, C.POINTER(GroupMember), _P, _P, _Z, _P]),
    "gcnn_prenorm_merge": (C.c_int, [_DP, _P, _P, _P, _P, _GP, _GP, _P, _Z, _I, _P, _P]),
    "gcnn_group_prenorm_merge": (C.c_int, [_I, C.POINTER(GroupMember), C.POINTER(C.c_int32), C.POINTER(C.c_void_p), _P, _P, _Z, _P]),
    "gcnn_rank_deviations": (C.c_int, [_P, _I, _P, _P, _P, _I, _P, _P, _I, _P, _P]),
    "gcnn_infer_batch_layout_for": (C.c_int, [_I, _P, _P, _P, _I, C.POINTER(IbatchLayout)]),
    "gcnn_infer_batch_fill_table": (C.c_int, [_I, _P, _P, _P, _P]),
    "gcnn_infer_batch": (C.c_int, [_I, _P, _P, _P, _I, _P, _P, _P, _P, _Z, _D, _D, _P]),
    "gcnn_lp_layout_for": (C.c_int, [C.POINTER(LpDims), _I, _I, C.POINTER(LpLayout)]),
    "gcnn_lp_state": (C.c_int, [C.POINTER(LpDims), _P, _P, _Z, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P]),
    "gcnn_lp_infer": (C.c_int, [C.POINTER(LpDims), _P, _P, _P, _P, _Z, _I, _P]),
    "gcnn_lp_infer_select": (C.c_int, [C.POINTER(LpDims), _I, _I, _P, _P, _P, _P, _Z, _D, _D, _P]),
    "gcnn_lp_batch_layout_for": (C.c_int, [_I, _P, _P, _P, _I, C.POINTER(LpBatchLayout)]),
    "gcnn_lp_batch_fill_table": (C.c_int, [_I, _P, _P, _P, _I, _P]),
    "gcnn_lp_batch": (C.c_int, [_I, _P, _P, _P, _I, _P, _P, _P, _P, _Z, _D, _D, _P]),
    "gcnn_hybrid_layout_for": (C.c_int, [_I, _P, _P, _P, _I, C.POINTER(HybridLayout)]),
    "gcnn_hybrid_fill_table": (C.c_int, [_I, _P, _P, _P, _I, _P]),
    "gcnn_hybrid_select": (C.c_int, [_I, _P, _P, _P, _I, _P, _P, _P, _Z, _D, _D, _P]),
    "gcnn_lp_collect_layout_for": (C.c_int, [C.POINTER(LpDims), _I, _I, C.POINTER(LpCollectLayout)]),
    "gcnn_lp_collect": (C.c_int, [C.POINTER(LpDims), _I, _I, _P, _P, _P, _Z, _D, _D, _P]),
    "gcnn_infer_models_layout_for": (C.c_int, [_I, _P, _P, _P, _I, _I, _P, C.POINTER(MbatchLayout)]),
    "gcnn_infer_models_fill_table": (C.c_int, [_I, _P, _P, _P, _I, _P, _P]),
    "gcnn_infer_models": (C.c_int, [_I, _P, _P, _P, _I, _I, _P, _P, _P, _P, _P, _Z, _P, _D, _D, _P]),
    "gcnn_lp_models_layout_for": (C.c_int, [_I, _P, _P, _P, _I, _I, _P, C.POINTER(LpModelsLayout)]),
    "gcnn_lp_models_fill_table": (C.c_int, [_I, _P, _P, _P, _I, _I, _P, _P]),
    "gcnn_lp_models": (C.c_int, [_I, _P, _P, _P, _I, _I, _P, _P, _P, _P, _P, _Z, _P, _D, _D, _P]),
    "gcnn_lp_rows_layout_for": (C.c_int, [C.POINTER(LpDims), C.POINTER(LpRowsLayout)]),
    "gcnn_lp_rows_build": (C.c_int, [C.POINTER(LpDims), _P, _P, _P, _P, _P, _P, _P, _Z, _P]),
    "gcnn_lp_round_layout_for": (C.c_int, [C.POINTER(LpDims), _I, _I, _I, C.POINTER(LpRoundLayout)]),
    "gcnn_lp_round": (C.c_int, [C.POINTER(LpDims), _I, C.POINTER(LpResident), _P, _P, _P, _P, _Z, _I, _P]),
    "gcnn_lp_round_select": (C.c_int, [C.POINTER(LpDims), _I, _I, _I, C.POINTER(LpResident), _P, _P, _P, _P, _Z, _D, _D, _P]),
    "gcnn_lp_append_layout_for": (C.c_int, [C.POINTER(LpDims), C.POINTER(LpAppendDims), _I, _I, _I, C.POINTER(LpAppendLayout)]),
    "gcnn_lp_rows_append": (C.c_int, [C.POINTER(LpDims), C.POINTER(LpAppendDims), _P, _P, _P, _P, _P, _P, C.POINTER(LpRowsSet),
                                      C.POINTER(LpRowsSet), _P, _Z, _P, _P]),
    "gcnn_lp_round_append": (C.c_int, [C.POINTER(LpDims), C.POINTER(LpAppendDims), _I, _I, _I, _P, _P, _P, _P, _P, C.POINTER(LpRowsSet),
                                       C.POINTER(LpRowsSet), C.POINTER(LpResident), _P, _P, _P, _P, _Z, _I, _D, _D, _P]),
    "gcnn_lp_remove_layout_for": (C.c_int, [C.POINTER(LpDims), C.POINTER(LpRemoveDims), C.POINTER(LpAppendDims), _I, _I, _I,
                                            C.POINTER(LpRemoveLayout)]),
    "gcnn_lp_rows_remove": (C.c_int, [C.POINTER(LpDims), C.POINTER(LpRemoveDims), _P] + [_P] * 10 + [C.POINTER(LpRowsSet),
                                      C.POINTER(LpRowsSet), _P, _Z, _P, _P]),
    "gcnn_lp_round_remove": (C.c_int, [C.POINTER(LpDims), C.POINTER(LpRemoveDims), C.POINTER(LpAppendDims), _I, _I, _I] + [_P] * 10 + [
                                       C.POINTER(LpRowsSet), C.POINTER(LpRowsSet), C.POINTER(LpRowsSet), C.POINTER(LpResident), _P, _P, _P,
                                       _P, _Z, _I, _D, _D, _P]),
    "gcnn_lp_rounds_layout_for": (C.c_int, [_I, C.POINTER(LpRoundsMember), _I, C.POINTER(LpRoundsLayout)]),
    "gcnn_lp_rounds": (C.c_int, [_I, C.POINTER(LpRoundsMember), _I, _P, _P, _P, _Z, _P, _D, _D, _P]),
    "gcnn_lp_rounds_edit_layout_for": (C.c_int, [_I, C.POINTER(LpRoundsEditMember), _I, C.POINTER(LpRoundsEditLayout)]),
    "gcnn_lp_rounds_edit": (C.c_int, [_I, C.POINTER(LpRoundsEditMember), _I, _P, _P, _P, _Z, _P, _D, _D, _P]),
    "gcnn_ensemble_mean": (C.c_int, [_P, _I, _I, _P, _P]),
    "gcnn_infer_ensemble_layout_for": (C.c_int, [_DP, _I, _I, _I, _I, C.POINTER(EnsembleLayout)]),
    "gcnn_infer_ensemble": (C.c_int, [_DP, _I, _I, _I, _I, _P, _P, _P, _P, _Z, _P, _D, _D, _P]),
    "gcnn_lp_ensemble_layout_for": (C.c_int, [C.POINTER(LpDims), _I, _I, _I, _I, C.POINTER(LpEnsembleLayout)]),
    "gcnn_lp_ensemble": (C.c_int, [C.POINTER(LpDims), _I, _I, _I, _I, _P, _P, _P, _P, _Z, _P, _D, _D, _P]),
    "gcnn_infer_ensemble_batch_layout_for": (C.c_int, [_I, _P, _P, _P, _I, _I, C.POINTER(EnsembleLayout)]),
    "gcnn_infer_ensemble_batch": (C.c_int, [_I, _P, _P, _P, _I, _I, _P, _P, _P, _P, _Z, _P, _D, _D, _P]),
    "gcnn_lp_ensemble_batch_layout_for": (C.c_int, [_I, _P, _P, _P, _I, _I, C.POINTER(LpEnsembleLayout)]),
    "gcnn_lp_ensemble_batch": (C.c_int, [_I, _P, _P, _P, _I, _I, _P, _P, _P, _P, _Z, _P, _D, _D, _P]),
    "gcnn_lp_round_ensemble_layout_for": (C.c_int, [C.POINTER(LpRoundsEditMember), _I, _I, C.POINTER(LpRoundEnsembleLayout)]),
    "gcnn_lp_round_ensemble": (C.c_int, [C.POINTER(LpRoundsEditMember), _I, _I, _P, _P, _P, _P, _Z, _P, _D, _D, _P]),
}

_lib = None


def lib() -> C.CDLL:
    """Load (once) and return the shared library; raises GcnnError when it is absent -- there is no CPU fallback."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise GcnnError(f"{LIB_PATH} not found: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                            "(or gcnn-cut-selector_amd/csrc/build.sh); there is no CPU fallback")
        try:
            handle = C.CDLL(LIB_PATH)
        except OSError as exc:  # pragma: no cover
            raise GcnnError(f"cannot load {LIB_PATH}: {exc}") from exc
        for name, (res, args) in SIGNATURES.items():
            fn = getattr(handle, name)
            fn.restype, fn.argtypes = res, args
        if handle.gcnn_abi_version() != ABI_VERSION:
            raise GcnnError(f"ABI mismatch: library {handle.gcnn_abi_version()} vs binding {ABI_VERSION}; rebuild")
        _lib = handle
    return _lib


def check(rc: int, what: str):
    if rc != 0:
        kind = {-1: "bad argument", -2: "workspace too small", -3: "HIP call failed", -4: "unsupported size"}.get(rc, f"hipError_t {rc}" if rc > 0 else f"code {rc}")
        raise GcnnError(f"{what} failed: {kind}")


class launch_profile:
    """`with launch_profile() as prof: ...` -> prof.launches = [(kernel name, milliseconds)] of every library launch inside."""

    def __enter__(self):
        check(lib().gcnn_profile_begin(), "gcnn_profile_begin")
        self.launches = []
        return self

    def __exit__(self, *exc):
        cap = 512
        names, ms = (C.c_char_p * cap)(), (C.c_float * cap)()
        n = lib().gcnn_profile_end(cap, names, ms)
        if n < 0:
            check(n, "gcnn_profile_end")
        self.launches = [(names[i].decode(), float(ms[i])) for i in range(min(n, cap))]
        return False


def param_layout():
    """[(offset, rows, cols, trainable)] for the 62 checkpoint arrays, and the flat buffer size, from the library."""
    handle = lib()
    out = []
    for i in range(handle.gcnn_param_count()):
        off, rows, cols, tr = C.c_int(), C.c_int(), C.c_int(), C.c_int()
        check(handle.gcnn_param_info(i, C.byref(off), C.byref(rows), C.byref(cols), C.byref(tr)), "gcnn_param_info")
        out.append((off.value, rows.value, cols.value, bool(tr.value)))
    return out, handle.gcnn_param_total_floats()
