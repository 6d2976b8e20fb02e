"""ctypes binding of ``libsemidetr_hip.so`` (C ABI declared in ``include/semidetr_hip.h``).

There is NO fallback: if the shared library is missing or a call fails, an exception is raised.  The
library is built in-tree by ``__graft_entry__.build()`` / ``make -C semi-detr_amd/csrc``.
"""
import contextlib
import ctypes
import os

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
# SEMIDETR_EXPERIMENTS=1 (tests that force kernel variants, tools/, bench.py's HBM-peak probe) selects the experiments
# build: the same sources with every measured-and-rejected kernel variant + the tuning entry points
# (include/semidetr_hip_experiments.h).  The product library has neither.
EXPERIMENTS = os.environ.get("SEMIDETR_EXPERIMENTS", "0") not in ("", "0")
LIB_PATH = os.path.join(_HERE, "csrc", "libsemidetr_hip_exp.so" if EXPERIMENTS else "libsemidetr_hip.so")

c_void_p, c_int, c_int64, c_double = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64, ctypes.c_double
c_float, c_size_t, POINTER = ctypes.c_float, ctypes.c_size_t, ctypes.POINTER

# ---------------------------------------------------------------------------------------------
# the ctypes mirrors of include/semidetr_hip.h: constants, parameter blocks, signatures.  A new op declares all three HERE;
# tests/test_cabi_mirror.py compiles the header and checks every value, size, offset, field type and argument type below.
# ---------------------------------------------------------------------------------------------
# macro -> value: every macro a mirror depends on
CONSTANTS = {
    "SEMIDETR_ABI_VERSION": 7,
    "SEMIDETR_EMA_CHUNK": 8192,
    "SEMIDETR_GMM_COVARIANCE_DIAG": 1,
    "SEMIDETR_SET_LOSS_MATCHED": 0, "SEMIDETR_SET_LOSS_DN": 1, "SEMIDETR_SET_LOSS_WARMUP": 2,
    "SEMIDETR_SET_LOSS_MAX_LAYERS": 64, "SEMIDETR_SET_LOSS_NUM_STATS": 10, "SEMIDETR_SET_LOSS_NUM_TERMS": 5,
    "SEMIDETR_DN_MAX_IMAGES": 64, "SEMIDETR_DN_NOISE_COLS": 10,
    "SEMIDETR_QSEL_MAX_LEVELS": 8, "SEMIDETR_QSEL_MAX_K": 4096,
    "SEMIDETR_DET_MAX_K": 2048,
    "SEMIDETR_CONSIS_MAX_LAYERS": 16,
}
# the element type codes of semidetr_add_norm_mixed's rows (tests/test_add_norm_mixed_ref.py reads them back from the header)
ROW_TYPES = {"SEMIDETR_ROW_F32": 0, "SEMIDETR_ROW_FP16": 1, "SEMIDETR_ROW_BF16": 2}
_DN_IMAGES, _CONSIS_LAYERS = CONSTANTS["SEMIDETR_DN_MAX_IMAGES"], CONSTANTS["SEMIDETR_CONSIS_MAX_LAYERS"]
_STRIDE2 = c_int64 * 2                # the strides of a tensor's two leading dimensions, in elements


def _f(ctype, names):
    """The fields of one declaration of the header: ``int a, b;`` is ``_f(c_int, "a b")`` (every pointer is a ``c_void_p``)."""
    return [(n, ctype) for n in names.split()]


class CostParams(ctypes.Structure):
    _fields_ = (_f(c_float, "cls_weight alpha gamma eps reg_weight") + _f(c_int, "reg_xywh") + _f(c_float, "iou_weight")
                + _f(c_int, "iou_giou pred_xyxy"))


# the ground-truth table of semidetr_hungarian_assign_f32: SEMIDETR_MATCH_TABLE problems, by value in the kernel arguments
# (tests/test_native_chains_host.py reads the macro back from the header)
MATCH_TABLE = 64


class MatchTable(ctypes.Structure):
    _fields_ = (_f(c_int, "num_problems") + _f(ctypes.c_int32 * MATCH_TABLE, "count") + _f(ctypes.c_int32 * (MATCH_TABLE + 1), "offsets")
                + _f(c_float * 2 * MATCH_TABLE, "img_wh") + _f(c_void_p * MATCH_TABLE, "boxes labels"))


# the per-image tables of semidetr_teacher_pseudo_labels_f32 / semidetr_transform_bboxes_table_f32: SEMIDETR_IMAGE_TABLE images
IMAGE_TABLE = 64
_IMG_I32 = ctypes.c_int32 * IMAGE_TABLE


class ImageSizes(ctypes.Structure):
    _fields_ = _f(c_int, "num_images") + _f(c_float * 2 * IMAGE_TABLE, "hw")


class BoxTable(ctypes.Structure):
    _fields_ = (_f(c_int, "num_images") + _f(_IMG_I32, "count box_stride out_offset") + _f(c_float * 2 * IMAGE_TABLE, "out_hw")
                + _f(c_void_p * IMAGE_TABLE, "boxes matrix"))


class SetLossSegment(ctypes.Structure):
    _fields_ = (_f(c_int, "kind num_layers num_images num_query num_classes")
                + _f(c_void_p, "logits") + _f(c_int64 * 3, "logit_stride") + _f(c_void_p, "boxes") + _f(c_int64 * 3, "box_stride")
                + _f(c_void_p, "labels label_weights bbox_targets bbox_weights metrics gt_offsets gt_boxes gt_labels")
                + _f(c_int, "single_pad dn_groups") + _f(c_void_p, "img_wh")
                + _f(c_float, "alpha gamma cls_weight l1_weight iou_weight iou_eps bg_cls_weight") + _f(c_int, "sync_cls")
                + _f(c_void_p, "grad_logits grad_boxes"))


class DnLayout(ctypes.Structure):
    _fields_ = _f(c_int, "num_images single_pad groups") + _f(ctypes.c_int32 * (_DN_IMAGES + 1), "offsets")


class DnBuild(ctypes.Structure):
    _fields_ = (_f(DnLayout, "dn cons") + _f(ctypes.c_int32 * _DN_IMAGES, "src_counts") + _f(c_void_p * _DN_IMAGES, "labels boxes")
                + _f(c_int, "box_stride num_known") + _f(c_void_p, "label_weight")
                + _f(c_int, "num_embeddings hidden_dim num_classes num_queries") + _f(c_void_p, "noise image_noise")
                + _f(c_float, "label_noise_threshold box_noise_scale")
                + _f(c_void_p, "query_label query_bbox known_bid map_known_indice noised_labels pad_mask cons_rows cons_label "
                               "attn_mask"))


class DnConsistency(ctypes.Structure):
    _fields_ = (_f(DnLayout, "cons") + _f(ctypes.c_int32 * _DN_IMAGES, "src_counts")
                + _f(c_void_p * _DN_IMAGES, "pseudo_boxes det_boxes") + _f(c_int, "pseudo_stride det_stride num_known")
                + _f(c_float * 2 * _DN_IMAGES, "tgt_wh src_wh")
                + _f(c_void_p, "query_bbox known_bid map_known_indice loss_weights rois") + _f(c_float, "loss_weight"))


class ConsisLayer(ctypes.Structure):
    _fields_ = _f(c_void_p, "v1 v2") + _f(_STRIDE2, "v1_stride v2_stride") + _f(c_void_p, "grad_v1")


class ConsisLoss(ctypes.Structure):
    _fields_ = (_f(c_int, "num_layers batch num_query dim pad_size num_known bid_is_int64") + _f(c_float, "scale eps")
                + _f(c_void_p, "known_bid map_known_indice loss_weights") + _f(ConsisLayer * _CONSIS_LAYERS, "layer"))


class SelfAttn(ctypes.Structure):
    _fields_ = (_f(c_int, "batch heads head_dim len_q len_k") + _f(c_float, "scale") + _f(c_void_p, "q k v")
                + _f(_STRIDE2, "q_stride k_stride v_stride") + _f(c_void_p, "mask out lse grad_out grad_q grad_k grad_v")
                + _f(_STRIDE2, "gq_stride gk_stride gv_stride"))


class SelfAttnH16(ctypes.Structure):
    _fields_ = (_f(c_int, "batch heads head_dim len_q len_k") + _f(c_float, "scale") + _f(c_int, "type") + _f(c_void_p, "q k v")
                + _f(_STRIDE2, "q_stride k_stride v_stride") + _f(c_void_p, "mask out lse grad_out grad_q grad_k grad_v")
                + _f(_STRIDE2, "gq_stride gk_stride gv_stride"))


class AddNorm(ctypes.Structure):
    _fields_ = (_f(c_int, "rows0 rows1 dim") + _f(c_float, "eps") + _f(c_void_p, "x residual pos gy gq")
                + _f(_STRIDE2, "x_stride residual_stride pos_stride gy_stride gq_stride")
                + _f(c_void_p, "weight bias y q mean rstd grad_x grad_weight grad_bias"))


class AddNormMixed(ctypes.Structure):
    _fields_ = (_f(c_int, "rows0 rows1 dim") + _f(c_float, "eps") + _f(c_void_p, "x residual pos gy gq")
                + _f(_STRIDE2, "x_stride residual_stride pos_stride gy_stride gq_stride")
                + _f(c_void_p, "weight bias y q mean rstd grad_x grad_residual grad_pos grad_weight grad_bias")
                + _f(c_int, "x_type residual_type pos_type gy_type gq_type y_type q_type grad_x_type grad_residual_type "
                            "grad_pos_type"))


# the level table of semidetr_gn_tokens: SEMIDETR_GN_MAX_LEVELS entries per field (tests/test_input_proj_ref.py reads the macro
# back from the header)
GN_MAX_LEVELS = 8
_GN_I64, _GN_PTR = c_int64 * GN_MAX_LEVELS, c_void_p * GN_MAX_LEVELS


class GnTokens(ctypes.Structure):
    _fields_ = (_f(c_int, "batch levels channels groups") + _f(c_float, "eps") + _f(_GN_I64, "hw start")
                + _f(c_int64, "tokens_per_image") + _f(_GN_PTR, "x") + _f(_GN_I64, "x_batch_stride")
                + _f(_GN_PTR, "weight bias grad_x grad_weight grad_bias") + _f(c_void_p, "tokens q pos gy gq")
                + _f(_STRIDE2, "pos_stride gy_stride gq_stride") + _f(c_void_p, "mean rstd") + _f(c_int, "x_type out_type pos_type"))


# the segment table of semidetr_ref_points: SEMIDETR_REF_MAX_SEGMENTS entries, SEMIDETR_REF_MAX_LEVELS valid-ratio levels, and the
# SEMIDETR_REF_* modes (tests/test_ref_points_ref.py reads the macros back from the header)
REF_MAX_SEGMENTS, REF_MAX_LEVELS = 8, 8
REF_MODES = {"SEMIDETR_REF_NONE": 0, "SEMIDETR_REF_SIGMOID": 1, "SEMIDETR_REF_REFINE": 2}


class RefSegment(ctypes.Structure):
    _fields_ = (_f(c_int, "rows0 rows1") + _f(c_void_p, "delta ref") + _f(_STRIDE2, "delta_stride ref_stride")
                + _f(c_void_p, "new_ref") + _f(_STRIDE2, "new_ref_stride") + _f(c_void_p, "g_new") + _f(_STRIDE2, "g_new_stride")
                + _f(c_void_p, "g_delta g_ref"))


class RefPoints(ctypes.Structure):
    _fields_ = (_f(c_int, "width mode num_segments levels") + _f(c_float, "eps") + _f(c_int, "delta_type ref_type out_type")
                + _f(c_void_p, "valid_ratios dim_t ref_input embed g_ref_input g_embed")
                + _f(RefSegment * REF_MAX_SEGMENTS, "segment"))


# the level table and the by-value image sizes of semidetr_pyramid_inputs: SEMIDETR_PYR_MAX_LEVELS levels, SEMIDETR_PYR_MAX_BATCH
# images (tests/test_pyramid_inputs_ref.py reads the macros back from the header)
PYR_MAX_LEVELS, PYR_MAX_BATCH = 8, 64
_PYR_I32, _PYR_IMG = ctypes.c_int * PYR_MAX_LEVELS, ctypes.c_int * PYR_MAX_BATCH


class PyramidInputsBlock(ctypes.Structure):
    _fields_ = (_f(c_int, "batch levels") + _f(_PYR_I32, "h w") + _f(c_int64 * PYR_MAX_LEVELS, "start")
                + _f(c_int64, "tokens_per_image") + _f(c_int, "from_sizes input_h input_w") + _f(_PYR_IMG, "img_h img_w")
                + _f(c_void_p * PYR_MAX_LEVELS, "masks") + _f(c_int, "normalize") + _f(c_float, "offset eps scale")
                + _f(c_void_p, "dim_ty dim_tx level_embed") + _f(c_int, "level_embed_type pos_type g_type")
                + _f(c_void_p, "pos mask_flatten valid_ratios reference_points g") + _f(_STRIDE2, "g_stride")
                + _f(c_void_p, "grad_level_embed"))


# C struct -> mirror, in the header's order
STRUCTS = {"semidetr_cost_params": CostParams, "semidetr_match_table": MatchTable, "semidetr_image_sizes": ImageSizes,
           "semidetr_box_table": BoxTable, "semidetr_set_loss_segment": SetLossSegment, "semidetr_dn_layout": DnLayout,
           "semidetr_dn_build": DnBuild, "semidetr_dn_consistency": DnConsistency, "semidetr_consis_layer": ConsisLayer,
           "semidetr_consis_loss": ConsisLoss, "semidetr_self_attn": SelfAttn, "semidetr_self_attn_h16": SelfAttnH16,
           "semidetr_add_norm": AddNorm,
           "semidetr_add_norm_mixed": AddNormMixed, "semidetr_gn_tokens": GnTokens,
           "semidetr_ref_segment": RefSegment, "semidetr_ref_points": RefPoints, "semidetr_pyramid_inputs": PyramidInputsBlock}
_SEGS, _WORK = POINTER(SetLossSegment), [c_void_p, c_size_t]        # a segment table; the (workspace, workspace_bytes) pair

_MSDA_FWD = [c_void_p] * 6 + [c_int] * 7 + [c_void_p]
_MSDA_BWD = [c_void_p] * 7 + [c_int] * 7 + [c_void_p] * 3
_MSDA_FWD_F32 = [c_void_p] * 6 + [c_int] * 8 + [c_void_p]           # f32 entry points carry `flags`
_MSDA_BWD_F32 = [c_void_p] * 7 + [c_int] * 8 + [c_void_p] * 3

# name -> (restype, argtypes) of every function include/semidetr_hip.h declares
SIGNATURES = {
    "semidetr_abi_version": (c_int, []),
    "semidetr_last_error": (ctypes.c_char_p, []),
    "semidetr_msda_forward_f32": (c_int, _MSDA_FWD_F32),
    "semidetr_msda_forward_f64": (c_int, _MSDA_FWD),
    "semidetr_msda_backward_f32": (c_int, _MSDA_BWD_F32),
    "semidetr_msda_backward_f64": (c_int, _MSDA_BWD),
    "semidetr_msda_fused_forward_f32": (c_int, [c_void_p] * 5 + [c_int] + [c_void_p] * 4 + [c_int] * 8 + [c_void_p]),
    "semidetr_msda_fused_backward_f32": (c_int, [c_void_p] * 6 + [c_int] + [c_void_p] * 4 + [c_int] * 8 + [c_void_p] * 3),
    # ... with a host copy of spatial_shapes last (or None)
    "semidetr_msda_forward_f32_v2": (c_int, _MSDA_FWD_F32 + [c_void_p]),
    "semidetr_msda_backward_f32_v2": (c_int, _MSDA_BWD_F32 + [c_void_p]),
    "semidetr_msda_fused_forward_f32_v2": (c_int, [c_void_p] * 5 + [c_int] + [c_void_p] * 4 + [c_int] * 8 + [c_void_p] * 2),
    "semidetr_msda_fused_backward_f32_v2": (c_int, [c_void_p] * 6 + [c_int] + [c_void_p] * 4 + [c_int] * 8 + [c_void_p] * 4),
    "semidetr_msda_mask_extents": (c_int, [c_void_p] * 4 + [c_int] * 3 + [c_void_p]),
    # the exact backward: the arguments of semidetr_msda_backward_f32 with the (workspace, workspace_bytes) pair before the results
    "semidetr_msda_exact_workspace_bytes": (c_size_t, [c_int] * 6),
    "semidetr_msda_backward_exact_f32": (c_int, [c_void_p] * 7 + [c_int] * 8 + _WORK + [c_void_p] * 3),
    "semidetr_msda_last_kernels": (ctypes.c_char_p, []),
    "semidetr_msda_forward_h16": (c_int, [c_void_p, c_int] + [c_void_p] * 5 + [c_int] * 7 + [c_void_p]),
    "semidetr_msda_backward_h16_workspace_bytes": (c_size_t, [c_int] * 4),
    "semidetr_msda_backward_h16": (c_int, [c_void_p, c_int] + [c_void_p] * 6 + [c_int] * 7 + [c_void_p] * 4),
    "semidetr_msda_fused_forward_h16": (c_int, [c_void_p, c_int] + [c_void_p] * 4 + [c_int] + [c_void_p] * 2 + [c_int, c_void_p] +
                                        [c_int] * 7 + [c_void_p]),
    "semidetr_msda_fused_backward_h16": (c_int, [c_void_p, c_int] + [c_void_p] * 5 + [c_int] + [c_void_p] * 2 + [c_int, c_void_p] +
                                         [c_int] * 7 + [c_void_p] * 4),
    "semidetr_msda_h16_last_kernels": (ctypes.c_char_p, []),
    "semidetr_msda_set_forward_policy": (c_int, [c_int]),
    "semidetr_msda_forward_policy_state": (c_int, [c_void_p] * 4),
    "semidetr_msda_forward_policy_state_slot": (c_int, [c_int] + [c_void_p] * 4),
    "semidetr_msda_gather_choice": (c_int, [c_int]),
    "semidetr_msda_set_region_grid": (c_int, [c_int] * 3),
    "semidetr_msda_region_grid_query": (c_int, [c_int, c_void_p] + [c_int] * 4 + [c_void_p]),
    "semidetr_match_cost_f32": (c_int, [c_void_p] * 7 + [c_int] * 4 + [POINTER(CostParams), c_void_p]),
    "semidetr_lsap_workspace_bytes": (c_int64, [c_int, c_int, c_int]),
    "semidetr_lsap_solve": (c_int, [c_void_p] * 4 + [c_int] * 4 + [c_void_p] * 6),
    "semidetr_build_targets": (c_int, [c_void_p] * 6 + [c_int, c_int, c_int64] + [c_void_p] * 5),
    # ... the three as one call, the ground truths through a by-value table
    "semidetr_hungarian_assign_f32": (c_int, [c_void_p] * 3 + [POINTER(MatchTable), c_int, c_int, POINTER(CostParams)]
                                      + [c_void_p] * 7 + [c_int64] + [c_void_p] * 5),
    "semidetr_ema_multi_f32": (c_int, [c_void_p] * 5 + [c_int, c_int, c_double]),
    "semidetr_ema_flat_f32": (c_int, [c_void_p, c_void_p, c_void_p, c_int64, c_double]),
    "semidetr_pseudo_label_filter_f32": (c_int, [c_void_p] * 5 + [c_int] + [c_void_p] * 6),
    "semidetr_nms_workspace_bytes": (c_size_t, [c_int, c_int, c_int]),
    "semidetr_pseudo_nms_f32": (c_int, [c_void_p] * 4 + [c_int] * 3 + [c_float, c_float, c_int, c_void_p,
                                                                       c_size_t] + [c_void_p] * 3),
    "semidetr_o2m_assign_f32": (c_int, [c_void_p] * 7 + [c_int] * 7 + [c_float, c_float] + [c_void_p] * 7),
    "semidetr_tal_loss_workspace_bytes": (c_size_t, []),
    "semidetr_tal_loss_f32": (c_int, [c_void_p] * 4 + [c_int64, c_int, c_float, c_int] + [c_void_p] * 3),
    "semidetr_transform_bboxes_f32": (c_int, [c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_int, c_int] + [c_void_p] * 3),
    # ... the teacher's chain as one call and the warp through a pointer table, the small arguments by value
    "semidetr_teacher_pseudo_labels_f32": (c_int, [c_void_p] * 3 + [POINTER(ImageSizes), c_int, c_int, c_float, c_float, c_int,
                                                    c_void_p, c_size_t] + [c_void_p] * 7),
    "semidetr_transform_bboxes_table_f32": (c_int, [c_void_p, POINTER(BoxTable), c_void_p]),
    "semidetr_gmm_match_costs_f32": (c_int, [c_void_p] * 6 + [c_int] * 4 + [c_void_p] * 2),
    "semidetr_gmm_fit_f64": (c_int, [c_void_p, c_void_p, c_int64, c_void_p, c_int64] + [c_int] * 3 + [c_double, c_double, c_int]
                             + [c_void_p] * 4),
    "semidetr_gmm_double_filter_f32": (c_int, [c_void_p] * 12 + [c_int, c_int, c_float, c_int] + [c_void_p] * 10),
    # set_loss.py; the segment table is a host array
    "semidetr_set_loss_workspace_bytes": (c_int64, [_SEGS, c_int]),
    "semidetr_set_loss_forward_f32": (c_int, [c_void_p, _SEGS, c_int, c_void_p, c_int64] + [c_void_p] * 4),
    "semidetr_set_loss_finalize_f32": (c_int, [c_void_p, _SEGS, c_int] + [c_void_p] * 5),
    "semidetr_set_loss_backward_f32": (c_int, [c_void_p, _SEGS, c_int, c_void_p, c_void_p]),
    # dn_query.py; here and below a parameter block is a host pointer, typed: the block of another op is an ArgumentError
    "semidetr_dn_build_f32": (c_int, [c_void_p, POINTER(DnBuild)]),
    "semidetr_dn_consistency_f32": (c_int, [c_void_p, POINTER(DnConsistency)]),
    "semidetr_dn_label_backward_f32": (c_int, [c_void_p] * 5 + [c_int] * 5 + [c_void_p]),
    "semidetr_dn_gather_rows_f32": (c_int, [c_void_p, POINTER(DnLayout), c_void_p, c_int, c_void_p]),
    # two-stage query selection (query_select.py)
    "semidetr_qsel_proposals_f32": (c_int, [c_void_p] * 5 + [c_int] * 4 + [c_void_p] * 3),
    "semidetr_qsel_proposals_backward_f32": (c_int, [c_void_p] * 3 + [c_int] * 3 + [c_void_p]),
    "semidetr_qsel_topk_workspace_bytes": (c_size_t, [c_int, c_int]),
    "semidetr_qsel_topk_f32": (c_int, [c_void_p, c_void_p] + [c_int] * 4 + [c_void_p, c_size_t, c_void_p, c_void_p]),
    "semidetr_qsel_gather_f32": (c_int, [c_void_p] * 5 + [c_int] * 4 + [c_void_p] * 4),
    "semidetr_qsel_gather_backward_f32": (c_int, [c_void_p] * 6 + [c_int] * 4 + [c_void_p] * 2),
    # detection decode at evaluation / inference time (detect.py)
    "semidetr_det_workspace_bytes": (c_size_t, [c_int] * 4),
    "semidetr_det_decode_f32": (c_int, [c_void_p] * 5 + [c_int] * 4 + [c_void_p, c_size_t] + [c_void_p] * 4),
    # cross-view consistency loss (consis_loss.py)
    "semidetr_consis_loss_workspace_bytes": (c_size_t, [c_int] * 4),
    "semidetr_consis_loss_forward_f32": (c_int, [c_void_p, POINTER(ConsisLoss)] + _WORK + [c_void_p]),
    "semidetr_consis_loss_backward_f32": (c_int, [c_void_p, POINTER(ConsisLoss)] + _WORK + [c_void_p]),
    # decoder self-attention core (self_attn.py)
    "semidetr_self_attn_workspace_bytes": (c_size_t, [c_int] * 4),
    "semidetr_self_attn_forward_f32": (c_int, [c_void_p, POINTER(SelfAttn)] + _WORK),
    "semidetr_self_attn_backward_f32": (c_int, [c_void_p, POINTER(SelfAttn)] + _WORK),
    "semidetr_self_attn_forward_h16": (c_int, [c_void_p, POINTER(SelfAttnH16)] + _WORK),
    "semidetr_self_attn_backward_h16": (c_int, [c_void_p, POINTER(SelfAttnH16)] + _WORK),
    # residual add + LayerNorm + positional add (add_norm.py)
    "semidetr_add_norm_workspace_bytes": (c_size_t, [c_int64]),
    "semidetr_add_norm_forward_f32": (c_int, [c_void_p, POINTER(AddNorm)] + _WORK),
    "semidetr_add_norm_backward_f32": (c_int, [c_void_p, POINTER(AddNorm)] + _WORK),
    "semidetr_add_norm_forward_mixed": (c_int, [c_void_p, POINTER(AddNormMixed)] + _WORK),
    "semidetr_add_norm_backward_mixed": (c_int, [c_void_p, POINTER(AddNormMixed)] + _WORK),
    # GroupNorm of the input projection written into the token pyramid (input_proj.py)
    "semidetr_gn_tokens_workspace_bytes": (c_size_t, [POINTER(GnTokens), c_int]),
    "semidetr_gn_tokens_forward": (c_int, [c_void_p, POINTER(GnTokens)] + _WORK),
    "semidetr_gn_tokens_backward": (c_int, [c_void_p, POINTER(GnTokens)] + _WORK),
    # reference-point chain of the decoder: refine, valid-ratio scaling, sine embed (ref_points.py)
    "semidetr_ref_points_forward": (c_int, [c_void_p, POINTER(RefPoints)]),
    "semidetr_ref_points_backward": (c_int, [c_void_p, POINTER(RefPoints)]),
    # pyramid masks, sine position rows, valid ratios and encoder reference points (pyramid_inputs.py)
    "semidetr_pyramid_inputs_workspace_bytes": (c_size_t, [POINTER(PyramidInputsBlock), c_int]),
    "semidetr_pyramid_inputs_forward": (c_int, [c_void_p, POINTER(PyramidInputsBlock)] + _WORK),
    "semidetr_pyramid_inputs_backward": (c_int, [c_void_p, POINTER(PyramidInputsBlock)] + _WORK),
}

# include/semidetr_hip_experiments.h: only in libsemidetr_hip_exp.so
EXPERIMENT_SIGNATURES = {
    "semidetr_msda_set_variant": (None, [c_int, c_int]),
    "semidetr_debug_counters": (c_int, [c_void_p, c_int]),
    "semidetr_stream_copy_f32": (c_int, [c_void_p, c_void_p, c_void_p, c_int64, c_int]),
}

_lib = None


class NativeLibraryError(RuntimeError):
    pass


def lib():
    """Load the shared library (once).  Raises ``NativeLibraryError`` when it is not built."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise NativeLibraryError(
                f"{LIB_PATH} not found: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                "or `make -C semi-detr_amd/csrc` (hipcc --offload-arch=gfx950). There is no CPU fallback.")
        handle = ctypes.CDLL(LIB_PATH)
        table = dict(SIGNATURES, **EXPERIMENT_SIGNATURES) if EXPERIMENTS else SIGNATURES
        for name, (res, args) in table.items():
            fn = getattr(handle, name)       # AttributeError if the .so is stale / symbol missing
            fn.restype, fn.argtypes = res, args
        _lib = handle
    return _lib


def check(rc, what):
    """Turn a C-ABI status into a RuntimeError (what the reference's AT_ASSERTM / launch failures give)."""
    if rc != 0:
        msg = lib().semidetr_last_error().decode(errors="replace")
        raise RuntimeError(f"{what} failed (code {rc}): {msg}")


def current_stream_ptr():
    return c_void_p(torch.cuda.current_stream().cuda_stream)


# ---------------------------------------------------------------------------------------------
# the one call path of the host mirrors
# ---------------------------------------------------------------------------------------------
_NO_GUARD = contextlib.nullcontext()
_Tensor = torch.Tensor              # bound once: ptr_args tests every argument of every launch
_functions = {}                     # name -> (library handle, function): looked up and checked once per handle


def device_guard(dev):
    """Device guard only where ``dev`` is not the current device (entering ``torch.cuda.device`` costs more than a launch).
    A ``dev`` without an index is the current device."""
    if dev.index is None or dev.index == torch.cuda.current_device():
        return _NO_GUARD
    return torch.cuda.device(dev)


def ptr_args(args):
    """Arguments of a C-ABI call: a tensor becomes its data pointer, ``None`` stays ``None`` (NULL for a ``c_void_p``), anything
    else (Python numbers, ctypes instances, ``ctypes.byref(...)``, ctypes arrays) is left to the argtypes of ``SIGNATURES``."""
    return [c_void_p(a.data_ptr()) if isinstance(a, _Tensor) else a for a in args]


def _function(name):
    hit = _functions.get(name)
    if hit is not None and hit[0] is _lib:
        return hit[1]
    if name not in SIGNATURES and not (EXPERIMENTS and name in EXPERIMENT_SIGNATURES):
        raise AttributeError(f"{name} is not a function of the C ABI (_lib.SIGNATURES)")
    fn = getattr(lib(), name)
    _functions[name] = (_lib, fn)
    return fn


def calls(dev, *launches):
    """Launches back to back, each a ``(name, *args)``: ``name(stream, *args)`` on the current stream of ``dev`` with ``dev``
    current, under one guard decision and one stream lookup.  Every name is resolved before the first launch; a non-zero status
    raises (``check``) before the next one.  Every entry point that launches takes ``void *stream`` first; the size queries are
    plain ``lib().f(...)`` calls."""
    fns = [_function(launch[0]) for launch in launches]
    with device_guard(dev):
        stream = c_void_p(torch.cuda.current_stream(dev).cuda_stream)
        for fn, launch in zip(fns, launches):
            rc = fn(stream, *ptr_args(launch[1:]))
            if rc:
                check(rc, launch[0])


def call(name, dev, *args):
    """One launch: ``calls(dev, (name, *args))``."""
    calls(dev, (name,) + args)


def small_to_device(values, dtype, dev):
    """Small host list -> device tensor without a stream synchronisation (pinned staging + async copy); a plain
    ``torch.tensor(list, device=...)`` is a blocking copy that drains the stream on every call."""
    host = torch.tensor(values, dtype=dtype)
    if dev.type == "cuda":
        return host.pin_memory().to(dev, non_blocking=True)
    return host.to(dev)


def offsets(counts, dev):
    """Exclusive prefix sum of ``counts`` as (host list, int32 device tensor), one entry more than ``counts``."""
    offs = [0]
    for c in counts:
        offs.append(offs[-1] + int(c))
    return offs, small_to_device(offs, torch.int32, dev)


def rows_f32(t):
    """A 3-D tensor as the kernels read it through a base pointer and the strides of its two leading dimensions: detached, fp32,
    last stride 1, base and both leading strides 16-byte aligned; copied only where it is not."""
    t = t.detach()
    if t.dtype != torch.float32:
        t = t.float()
    if t.stride(2) != 1 or t.data_ptr() % 16 or t.stride(0) % 4 or t.stride(1) % 4:
        t = t.contiguous()
    return t


def row_type(dtype):
    """The ``SEMIDETR_ROW_*`` code of a torch dtype (``ROW_TYPES``); anything but fp32, fp16 and bf16 is a ``TypeError``."""
    code = _ROW_TYPE_OF.get(dtype)
    if code is None:
        raise TypeError(f"rows of {dtype} are not built (float32, float16, bfloat16)")
    return code


_ROW_TYPE_OF = {torch.float32: ROW_TYPES["SEMIDETR_ROW_F32"], torch.float16: ROW_TYPES["SEMIDETR_ROW_FP16"],
                torch.bfloat16: ROW_TYPES["SEMIDETR_ROW_BF16"]}


def rows_native(t):
    """``rows_f32`` that keeps the dtype (fp32, fp16 or bf16): a 3-D tensor as the mixed kernels read it, detached, last stride
    1, both leading strides non-negative multiples of 4 elements, base 16-byte (fp32) or 8-byte (16-bit) aligned; copied only
    where it is not.  A 16-bit slice whose rows start 8 bytes into a 16-byte line stays in place."""
    t = t.detach()
    row_type(t.dtype)
    if t.stride(2) != 1 or t.data_ptr() % (16 if t.dtype == torch.float32 else 8) or t.stride(0) % 4 or t.stride(1) % 4:
        t = t.contiguous()
    return t


def set_rows(block, name, t, stride=None):
    """``block.<name>`` = the data pointer of ``t`` and ``block.<stride>[0:2]`` = its two leading strides; the stride field is
    ``<name>_stride`` unless named.  ``None`` leaves the field NULL."""
    if t is None:
        return
    setattr(block, name, t.data_ptr())
    st, strides = getattr(block, stride or name + "_stride"), t.stride()
    st[0], st[1] = strides[0], strides[1]


def cast(t, dtype):
    """``t`` in ``dtype``, converted only where it is not; ``None`` stays ``None``."""
    return t if t is None or t.dtype == dtype else t.to(dtype)


FORWARD_POLICIES = {"adaptive": 0, "patch": 1, "window": 2}


def set_forward_policy(policy):
    """Which kernel runs the encoder self-attention forward: "adaptive" (default: chosen from how far the samples of the
    previous launches reached), "patch" or "window" (include/semidetr_hip.h, semidetr_msda_set_forward_policy)."""
    check(lib().semidetr_msda_set_forward_policy(FORWARD_POLICIES.get(policy, policy)), "semidetr_msda_set_forward_policy")


def forward_policy_state(slot=0):
    """{'policy', 'mode' (0 patch / 1 window), 'far_fraction' (-1: no count received yet), 'updates'} of the current device and
    call-site slot (0 = the slot of callers that name none; MSDeformAttn instances hold theirs in ``policy_slot``)."""
    pol, mode, upd, frac = c_int(), c_int(), ctypes.c_uint(), c_float()
    check(lib().semidetr_msda_forward_policy_state_slot(int(slot), ctypes.byref(pol), ctypes.byref(mode), ctypes.byref(frac),
                                                        ctypes.byref(upd)), "semidetr_msda_forward_policy_state_slot")
    return {"policy": pol.value, "mode": mode.value, "far_fraction": frac.value, "updates": upd.value}


REGION_GRID_KERNELS = {"forward": 0, "gather": 1, "scatter": 2}


def set_region_grid(kernel, nry=0, nrx=0):
    """Pin the region grid of an encoder window kernel ("forward", "gather" or "scatter"); 0, 0: chosen per launch
    (include/semidetr_hip.h, semidetr_msda_set_region_grid)."""
    check(lib().semidetr_msda_set_region_grid(REGION_GRID_KERNELS.get(kernel, kernel), int(nry), int(nrx)),
          "semidetr_msda_set_region_grid")


def region_grid(kernel, spatial_shapes, batch, num_heads, num_cus):
    """What a launch of ``kernel`` takes for the level table ``spatial_shapes`` (rows of (H, W), or None: no host table):
    {'nry', 'nrx' (0, 0: the kernel's own coarsest grid), 'regions' (0: unknown), 'workgroups', 'tail_split', 'max_queries'}.
    Needs no GPU (semidetr_msda_region_grid_query)."""
    flat = None if spatial_shapes is None else [int(v) for hw in spatial_shapes for v in hw]
    table = None if flat is None else (c_int64 * len(flat))(*flat)
    levels = 1 if flat is None else len(flat) // 2
    out = (c_int * 6)()
    check(lib().semidetr_msda_region_grid_query(REGION_GRID_KERNELS.get(kernel, kernel), table, levels, int(batch), int(num_heads),
                                                int(num_cus), out), "semidetr_msda_region_grid_query")
    return dict(zip(("nry", "nrx", "regions", "workgroups", "tail_split", "max_queries"), out))


def set_variant(fwd, bwd):
    """Force a kernel variant (experiments build only).  (0, 0) is always accepted: the product library has no variants."""
    if EXPERIMENTS:
        lib().semidetr_msda_set_variant(int(fwd), int(bwd))
    elif (fwd, bwd) != (0, 0):
        raise NativeLibraryError("kernel variants exist only in the experiments build: set SEMIDETR_EXPERIMENTS=1 "
                                 "(libsemidetr_hip_exp.so) before importing semi_detr_amd")
