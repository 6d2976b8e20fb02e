"""semi-detr_amd: MI355X (gfx950) native hot path of Semi-DETR / DINO-DETR.

Scope: multi-scale deformable attention forward/backward, the Hungarian matcher
(cost matrix + LSAP + scatter), the mean-teacher EMA update and the pseudo-label filter, plus the
image-sharded data-parallel wrapper.  Host side is Python mirroring the reference's operator/plugin
surface; all arithmetic runs in hand-written HIP kernels behind the C ABI of
``include/semidetr_hip.h`` (``csrc/libsemidetr_hip.so``).  There is no CPU fallback.
"""
import sys as _sys

from . import _lib  # noqa: F401
from . import MultiScaleDeformableAttention as _msda_native

# The reference does `import MultiScaleDeformableAttention as MSDA`
# (detr_od/models/utils/ops/functions/ms_deform_attn_func.py:18); make that import resolve to ours.
_sys.modules.setdefault("MultiScaleDeformableAttention", _msda_native)

from .ops.functions import (MSDeformAttnExactFunction, MSDeformAttnFunction, MSDeformAttnFusedFunction,  # noqa: E402,F401
                            MSDeformAttnMixedFunction, MSDeformAttnMixedFusedFunction)
from .ops.modules import MSDeformAttn, convert_exact_backward  # noqa: E402,F401
from .matcher import (AssignResult, BBoxL1Cost, FocalLossCost, HungarianAssigner, IoUCost,  # noqa: E402,F401
                      O2MAssigner, O2MAssignResult, linear_sum_assignment)
from .losses import TaskAlignedFocalLoss, task_aligned_focal_loss  # noqa: E402,F401
from .mean_teacher import MeanTeacher, ema_momentum, ema_update_, ema_update_flat_  # noqa: E402,F401
from .targets import TargetAssigner, get_targets, get_targets_layers  # noqa: E402,F401
from .gmm_filter import (GmmFilterResult, PendingGmmFilter, fit_gmm, fit_gmm_threshold,  # noqa: E402,F401
                         fit_gmm_threshold_segments, unsup_gmm_filter)
from .set_loss import FocalLoss, SetLossSegment, loss_set, set_losses  # noqa: E402,F401
from .dn_query import consistency_queries, prepare_for_cdn, prepare_for_cdn_plus, prepare_unsup_cdn  # noqa: E402,F401
from .query_select import gen_encoder_output_proposals, select_queries, two_stage_queries  # noqa: E402,F401
from .detect import PendingDetections, detection_results, get_bboxes  # noqa: E402,F401
from .consis_loss import ConsistencyLossFunction, consistency_loss  # noqa: E402,F401
from .self_attn import (MaskedAttentionFunction, MaskedAttentionH16Function, MultiheadAttention, convert_self_attention,  # noqa: E402,F401
                        masked_attention)
from .add_norm import (AddLayerNormFunction, LayerNorm, add_layer_norm, convert_layer_norms, decoder_layer_forward,  # noqa: E402,F401
                       decoder_layer_forward_ca, decoder_layer_forward_ffn, decoder_layer_forward_sa, encoder_forward,
                       encoder_layer_forward)
from .input_proj import (GroupNormTokensFunction, group_norm_to_tokens, group_norm_tokens_backward,  # noqa: E402,F401
                         group_norm_tokens_forward, project_pyramid)
from .ref_points import (RefPointsFunction, box_outputs, decoder_forward, gen_sineembed_for_position,  # noqa: E402,F401
                         reference_inputs, refine_boxes)
from .pyramid_inputs import (PyramidInputs, PyramidInputsFunction, SinePositionalEncodingHW, head_inputs,  # noqa: E402,F401
                             pyramid_inputs, pyramid_inputs_backward, pyramid_inputs_from_masks)
from .pseudo_label import (filter_pseudo_labels, get_bboxes_for_pseudo_label, teacher_pseudo_labels,  # noqa: E402,F401
                           transform_bboxes)

__all__ = ["MSDeformAttnExactFunction", "convert_exact_backward", "MSDeformAttnFunction", "MSDeformAttnFusedFunction", "MSDeformAttnMixedFunction", "MSDeformAttnMixedFusedFunction", "MSDeformAttn", "HungarianAssigner", "FocalLossCost", "BBoxL1Cost",
           "IoUCost", "AssignResult", "O2MAssigner", "O2MAssignResult", "TaskAlignedFocalLoss", "task_aligned_focal_loss", "linear_sum_assignment", "MeanTeacher", "ema_momentum", "ema_update_",
           "ema_update_flat_", "filter_pseudo_labels", "get_bboxes_for_pseudo_label", "teacher_pseudo_labels",
           "transform_bboxes", "TargetAssigner", "get_targets", "get_targets_layers", "fit_gmm", "fit_gmm_threshold",
           "fit_gmm_threshold_segments", "unsup_gmm_filter", "GmmFilterResult", "PendingGmmFilter",
           "FocalLoss", "SetLossSegment", "loss_set", "set_losses", "prepare_for_cdn", "prepare_for_cdn_plus",
           "prepare_unsup_cdn", "consistency_queries", "gen_encoder_output_proposals", "select_queries", "two_stage_queries",
           "get_bboxes", "detection_results", "PendingDetections", "consistency_loss", "ConsistencyLossFunction",
           "masked_attention", "MaskedAttentionFunction", "MaskedAttentionH16Function", "MultiheadAttention", "convert_self_attention",
           "add_layer_norm", "AddLayerNormFunction", "LayerNorm", "convert_layer_norms", "encoder_layer_forward", "encoder_forward",
           "decoder_layer_forward", "decoder_layer_forward_sa", "decoder_layer_forward_ca", "decoder_layer_forward_ffn",
           "group_norm_tokens_forward", "group_norm_tokens_backward", "GroupNormTokensFunction", "group_norm_to_tokens",
           "project_pyramid", "gen_sineembed_for_position", "refine_boxes", "reference_inputs", "decoder_forward", "box_outputs",
           "RefPointsFunction", "pyramid_inputs", "pyramid_inputs_from_masks", "pyramid_inputs_backward", "PyramidInputs",
           "PyramidInputsFunction", "SinePositionalEncodingHW", "head_inputs"]
