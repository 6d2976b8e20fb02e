"""``MultiScaleDeformableAttention`` -- the native module the reference imports
(``import MultiScaleDeformableAttention as MSDA``, detr_od/models/utils/ops/functions/ms_deform_attn_func.py:18).

The reference builds it with pybind from ``ops/src`` (vision.cpp:13-16).  Here it is the compiled extension
``_msda_ext`` (``csrc/msda_ext.cpp``: at::Tensor signatures of src/ms_deform_attn.h:20-61, same argument order, same
precondition errors, outputs freshly allocated on the inputs' device, current stream, no synchronisation) in front of
the C ABI of ``csrc/libsemidetr_hip.so`` where the hand-written gfx950 kernels live.  This file only loads it and
re-exports its functions; there is no Python or CPU implementation to fall back to.

    ms_deform_attn_forward(value, spatial_shapes, level_start_index, sampling_loc, attn_weight, im2col_step) -> Tensor
    ms_deform_attn_backward(value, spatial_shapes, level_start_index, sampling_loc, attn_weight, grad_output,
                            im2col_step) -> [grad_value, grad_sampling_loc, grad_attn_weight]
    ms_deform_attn_fused_forward / ms_deform_attn_fused_backward / fused_supported   
    ms_deform_attn_h16_forward(value16, spatial_shapes, level_start_index, sampling_loc_f32, attn_weight_f32[, im2col_step])
                                                                      -> Tensor of value's dtype (Half / BFloat16)
    ms_deform_attn_h16_backward(value16, spatial_shapes, level_start_index, sampling_loc_f32, attn_weight_f32, grad_output16
                                [, im2col_step]) -> [grad_value (value's dtype), grad_sampling_loc (fp32), grad_attn_weight (fp32)]
    h16_supported(value, sampling_loc, attn_weight) -> the mixed-precision op takes these tensors
    ms_deform_attn_h16_fused_forward(value16, spatial_shapes, level_start_index, reference_points, sampling_offsets, attn_logits
                                     [, padding_mask]) -> Tensor of value's dtype; offsets / logits both value's dtype or both fp32
    ms_deform_attn_h16_fused_backward(..., attn_logits, grad_output16[, padding_mask])
                                -> [grad_value (value's dtype), grad_sampling_offsets, grad_attn_logits (the offsets' dtype)]
    fused_h16_supported(value, reference_points, sampling_offsets, attn_logits) -> the fused 16-bit kernels take these tensors
    ms_deform_attn_exact_forward(value, spatial_shapes, level_start_index, sampling_loc, attn_weight, im2col_step) -> Tensor
                                the fp32 forward whose kernel is a function of the arguments alone (SEMIDETR_MSDA_FIXED_FORWARD)
    ms_deform_attn_exact_backward(value, spatial_shapes, level_start_index, sampling_loc, attn_weight, grad_output, im2col_step)
                                -> [grad_value, grad_sampling_loc, grad_attn_weight]: grad_value is the exact sum of its fp32
                                contributions rounded once -- bitwise independent of order (fp32, 32 channels)
    exact_supported(value, num_levels, num_point) -> the exact backward takes this value map (after an up-cast if it is 16-bit)
    pyramid_check(spatial_shapes, level_start_index, S) -> bit 0: sum(H*W) == S, bit 1: exact tiling (cached)
    mask_extents(padding_mask, spatial_shapes, level_start_index) -> (N, L) int32 summary of a padding mask (cached; the
                                                                      fused calls fetch it themselves)
"""
import torch  # noqa: F401  (libtorch must be loaded before the extension)

from . import _lib

try:
    if _lib.EXPERIMENTS:      # the front end linked against libsemidetr_hip_exp.so
        from . import _msda_ext_exp as _msda_ext
    else:
        from . import _msda_ext
except ImportError as e:      # not built (or built against another torch): fail loudly, never degrade
    raise _lib.NativeLibraryError(
        "semi-detr_amd/_msda_ext*.so is missing or does not load (%s): build it with "
        "`python -c 'import __graft_entry__ as g; g.build()'` or `make -C semi-detr_amd/csrc`. "
        "There is no CPU fallback." % (e,)) from e

ms_deform_attn_forward = _msda_ext.ms_deform_attn_forward
ms_deform_attn_backward = _msda_ext.ms_deform_attn_backward
ms_deform_attn_fused_forward = _msda_ext.ms_deform_attn_fused_forward
ms_deform_attn_fused_backward = _msda_ext.ms_deform_attn_fused_backward
fused_supported = _msda_ext.fused_supported
ms_deform_attn_h16_forward = _msda_ext.ms_deform_attn_h16_forward
ms_deform_attn_h16_backward = _msda_ext.ms_deform_attn_h16_backward
h16_supported = _msda_ext.h16_supported
ms_deform_attn_h16_fused_forward = _msda_ext.ms_deform_attn_h16_fused_forward
ms_deform_attn_h16_fused_backward = _msda_ext.ms_deform_attn_h16_fused_backward
fused_h16_supported = _msda_ext.fused_h16_supported
ms_deform_attn_exact_forward = _msda_ext.ms_deform_attn_exact_forward
ms_deform_attn_exact_backward = _msda_ext.ms_deform_attn_exact_backward
exact_supported = _msda_ext.exact_supported
pyramid_check = _msda_ext.pyramid_check
mask_extents = _msda_ext.mask_extents
gather_choice = _msda_ext.gather_choice

if _msda_ext.abi_version() != _lib.lib().semidetr_abi_version():      # a stale front end against a newer library
    raise _lib.NativeLibraryError("semi-detr_amd/_msda_ext*.so was built against ABI %d, libsemidetr_hip.so is ABI %d: rebuild "
                                  "(make -C semi-detr_amd/csrc)" % (_msda_ext.abi_version(), _lib.lib().semidetr_abi_version()))
