"""``MSDeformAttn`` -- the nn.Module around the operator.

Drop-in for detr_od/models/utils/ops/modules/ms_deform_attn.py:30-126: same constructor signature,
same sub-module names (``sampling_offsets``, ``attention_weights``, ``value_proj``, ``output_proj`` ->
identical ``state_dict`` keys, so published DINO / Semi-DETR checkpoints load unchanged), same
initialisation (:62-76), same ``forward`` arguments, errors and arithmetic (:78-126).  The four Linear
layers are dense GEMMs and stay on hipBLASLt/MFMA through torch; the sampling + aggregation and its
gradient go through ``MSDeformAttnFunction`` to the hand-written gfx950 kernels.
"""
import itertools
import math
import warnings

import torch
import torch.nn.functional as F
from torch import nn

from ... import MultiScaleDeformableAttention as MSDA
from ..functions import (MSDeformAttnExactFunction, MSDeformAttnFunction, MSDeformAttnFusedFunction, MSDeformAttnMixedFunction,
                         MSDeformAttnMixedFusedFunction)


def _is_power_of_2(n):
    if not isinstance(n, int) or n < 0:
        raise ValueError("invalid input for _is_power_of_2: {} (type: {})".format(n, type(n)))
    return n != 0 and (n & (n - 1)) == 0


_policy_slots = itertools.count(1)


def _next_policy_slot():
    return (next(_policy_slots) - 1) % 255 + 1


# Which 16-bit calls stay on the up-cast route (value.float() -> fp32 op -> .to(dtype)): the shape classes on which the
# mixed-precision kernels measured SLOWER than it by more than the spread between rounds (tools/msda_h16_probe.py,
# profiles/msda_h16_probe.txt; fp16 and bf16 alike).
#   * no backward will follow (no_grad / nothing requires grad: the teacher, evaluation): the 16-bit forward is no slower on any
#     shape measured (encoder 1.00-1.05x, decoder 2.3x, micro-benchmark 2.8x) -> every call takes it;
#   * a backward follows, the queries are the pixels (encoder self-attention): the fp32 op scatters grad_value with its
#     region-owned kernels, the 16-bit backward with row atomics -- 4.5 against 0.77 ms at bs 4 -> up-cast route;
#   * a backward follows, any other query set: level at 600 (n, q) rows, behind from _H16_TRAIN_MAX_ROWS rows on (the fp32 op's
#     merged level scatter) -> up-cast route above that.
_H16_TRAIN_MAX_ROWS = 600


def _h16_takes_upcast_route(queries_are_pixels, rows, backward_follows):
    if not backward_follows:
        return False
    return bool(queries_are_pixels) or rows > _H16_TRAIN_MAX_ROWS


class MSDeformAttn(nn.Module):
    def __init__(self, d_model=256, n_levels=4, n_heads=8, n_points=4):
        super().__init__()
        if d_model % n_heads != 0:
            raise ValueError("d_model must be divisible by n_heads, but got {} and {}".format(d_model, n_heads))
        if not _is_power_of_2(d_model // n_heads):
            warnings.warn("MSDeformAttn: a per-head dimension that is not a power of 2 (here {}) takes the "
                          "generic kernel; 32 channels per head is the tuned gfx950 path."
                          .format(d_model // n_heads))
        self.im2col_step = 64        # kept for config/state compatibility; one launch covers the batch
        # Fuse softmax + location arithmetic (and their backward) into the sampling kernels whenever the
        # configuration allows it (fp32, 32 channels per head): same results, none of the (N,Lq,M,L,P[,2])
        # intermediates in HBM.  Not a parameter / buffer -> state_dict is unchanged.  Set False for the
        # reference's op-by-op sequence.
        self.fuse_prologue = True
        # A 16-bit value map (torch.autocast, or the module after .half() / .bfloat16()) goes to the mixed-precision kernels as it
        # is: 16-bit value / output / grad_value, fp32 locations and weights, fp32 arithmetic.  False restores the
        # up-cast route (value.float() -> the fp32 op -> .to(dtype)).  Plain attribute like fuse_prologue, not in state_dict.
        self.native_16bit = True
        # Opt-in: a 16-bit call that would take the mixed-precision kernels hands them the Linear layers' RAW 16-bit offsets and
        # logits, the reference points and the padding mask instead -- softmax, location arithmetic and mask inside the kernels, in
        # fp32, none of the fp32 (N,Lq,M,L,P[,2]) intermediates in HBM.  Off by default: the results differ from
        # torch's autocast sequence, which forms offsets / normalizer in 16 bits (here that product is fp32).  Plain attribute.
        self.fuse_prologue_16bit = False
        # Opt-in: grad_value of this module's backward as the exact, order-independent sum of its fp32 contributions (DESIGN.md
        # 2.12c) -- with it a training step is reproducible bit for bit through MSDA.  False: nothing changes.  True: every call a
        # backward follows takes the op-by-op prologue and MSDeformAttnExactFunction (a 16-bit value through the up-cast route);
        # "auto": that while torch.are_deterministic_algorithms_enabled().  A no-grad call, and a call the exact entry does not
        # take (channels per head != 32, fp64), do exactly what they do with False.  Plain attribute, not in state_dict.
        self.exact_backward = False
        # Which of the two encoder forward kernels runs follows how far THIS instance's learned offsets reach (semidetr_hip.h:
        # SEMIDETR_MSDA_POLICY_SLOT): instances take consecutive slots 1..255 (the reference builds 12 per model,
        # transformer.py:609,760; beyond 255 instances slots are shared, which only mixes their counts).  Plain attribute.
        self.policy_slot = _next_policy_slot()
        self.d_model, self.n_levels, self.n_heads, self.n_points = d_model, n_levels, n_heads, n_points

        self.sampling_offsets = nn.Linear(d_model, n_heads * n_levels * n_points * 2)
        self.attention_weights = nn.Linear(d_model, n_heads * n_levels * n_points)
        self.value_proj = nn.Linear(d_model, d_model)
        self.output_proj = nn.Linear(d_model, d_model)
        self._reset_parameters()

    def __setstate__(self, state):
        # copy.deepcopy (an EMA teacher cloned from the student) and unpickling (torch.save(model), checkpoints that pickle modules)
        # both come through here: the copy is its own call site with its own learned offsets, so it takes a FRESH slot -- sharing
        # the original's would mix the two instances' sample-spread counts; a module pickled before the attribute existed gets one too
        super().__setstate__(state)
        self.__dict__["policy_slot"] = _next_policy_slot()
        self.__dict__.setdefault("fuse_prologue", True)
        self.__dict__.setdefault("native_16bit", True)
        self.__dict__.setdefault("fuse_prologue_16bit", False)
        self.__dict__.setdefault("exact_backward", False)

    def _reset_parameters(self):
        # ms_deform_attn.py:62-76 -- head m looks along direction 2*pi*m/M, point i at distance i+1
        nn.init.constant_(self.sampling_offsets.weight.data, 0.0)
        thetas = torch.arange(self.n_heads, dtype=torch.float32) * (2.0 * math.pi / self.n_heads)
        grid = torch.stack([thetas.cos(), thetas.sin()], -1)
        grid = grid / grid.abs().max(-1, keepdim=True)[0]
        grid = grid.view(self.n_heads, 1, 1, 2).repeat(1, self.n_levels, self.n_points, 1)
        grid = grid * torch.arange(1, self.n_points + 1, dtype=torch.float32).view(1, 1, -1, 1)
        with torch.no_grad():
            self.sampling_offsets.bias = nn.Parameter(grid.reshape(-1))
        nn.init.constant_(self.attention_weights.weight.data, 0.0)
        nn.init.constant_(self.attention_weights.bias.data, 0.0)
        nn.init.xavier_uniform_(self.value_proj.weight.data)
        nn.init.constant_(self.value_proj.bias.data, 0.0)
        nn.init.xavier_uniform_(self.output_proj.weight.data)
        nn.init.constant_(self.output_proj.bias.data, 0.0)

    def _takes_fused_16bit_route(self, value, reference_points, offsets, logits, shapes, starts):
        """fuse_prologue_16bit, on exactly the calls the mixed-precision kernels take today (native_16bit and the routing rule
        above) whose operands the fused 16-bit kernels accept and whose reference points need no gradient (the op returns none)."""
        if not (getattr(self, "fuse_prologue_16bit", False) and getattr(self, "native_16bit", True)):
            return False
        if value.dtype not in (torch.float16, torch.bfloat16) or not MSDA.fused_h16_supported(value, reference_points, offsets, logits):
            return False
        if torch.is_grad_enabled() and reference_points.requires_grad:
            return False
        N, Len_in, Len_q = value.shape[0], value.shape[1], offsets.shape[1]
        follows = torch.is_grad_enabled() and (value.requires_grad or offsets.requires_grad or logits.requires_grad)
        pixels = Len_q == Len_in and bool(MSDA.pyramid_check(shapes, starts, Len_in) & 2)
        return not _h16_takes_upcast_route(pixels, N * Len_q, follows)

    def _takes_exact_route(self, value, reference_points, offsets, logits):
        """exact_backward resolved for this call: the mode says so, a backward follows and the exact entry takes the shapes."""
        mode = getattr(self, "exact_backward", False)
        if mode == "auto":
            mode = torch.are_deterministic_algorithms_enabled()
        elif mode not in (True, False):
            raise ValueError("MSDeformAttn.exact_backward must be False, True or 'auto', got {!r}".format(mode))
        if not mode or not torch.is_grad_enabled():
            return False
        if not (value.requires_grad or offsets.requires_grad or logits.requires_grad or reference_points.requires_grad):
            return False
        return MSDA.exact_supported(value, self.n_levels, self.n_points)

    def forward(self, query, reference_points, input_flatten, input_spatial_shapes, input_level_start_index,
                input_padding_mask=None):
        """query (N, Lq, C); reference_points (N, Lq, L, 2|4) in [0,1]; input_flatten (N, sum HW, C);
        input_spatial_shapes (L, 2) [(H, W)]; input_level_start_index (L,); input_padding_mask (N, sum HW)
        True = padding.  Returns (N, Lq, C)."""
        N, Len_q, _ = query.shape
        N, Len_in, _ = input_flatten.shape
        # The reference asserts `(shapes[:, 0] * shapes[:, 1]).sum() == Len_in` on a device tensor (ms_deform_attn.py:90):
        # one blocking device-to-host copy per layer call, ~60 per SSOD step.  Same check, but answered from a cache keyed
        # on the (spatial_shapes, level_start_index) tensors -- all layers of a forward pass share them, so at most one
        # synchronisation per step, none when the caller keeps the two tensors alive between steps.
        assert MSDA.pyramid_check(input_spatial_shapes, input_level_start_index, Len_in) & 1
        M, L, P = self.n_heads, self.n_levels, self.n_points

        value = self.value_proj(input_flatten).view(N, Len_in, M, self.d_model // M)
        offsets = self.sampling_offsets(query).view(N, Len_q, M, L, P, 2)
        logits = self.attention_weights(query).view(N, Len_q, M, L * P)
        if reference_points.shape[-1] not in (2, 4):
            raise ValueError("Last dim of reference_points must be 2 or 4, but get {} instead."
                             .format(reference_points.shape[-1]))
        exact = self._takes_exact_route(value, reference_points, offsets, logits)
        if exact:
            pass      # the op-by-op prologue below (torch's softmax and elementwise backward are reproducible), then the exact op
        elif self.fuse_prologue and MSDA.fused_supported(value, reference_points, offsets, logits):
            # the padding mask (ms_deform_attn.py:95-96) goes INTO the kernels: no masked copy of `value`, no masking of its
            # gradient
            output = MSDeformAttnFusedFunction.apply(value.contiguous(), input_spatial_shapes,
                                                     input_level_start_index, reference_points.contiguous(),
                                                     offsets.contiguous(), logits.contiguous(), input_padding_mask,
                                                     getattr(self, "policy_slot", 0))
            return self.output_proj(output)
        elif self._takes_fused_16bit_route(value, reference_points, offsets, logits, input_spatial_shapes, input_level_start_index):
            output = MSDeformAttnMixedFusedFunction.apply(value.contiguous(), input_spatial_shapes, input_level_start_index,
                                                          reference_points.contiguous(), offsets.contiguous(), logits.contiguous(),
                                                          input_padding_mask)
            return self.output_proj(output)
        if input_padding_mask is not None:
            value = value.masked_fill(input_padding_mask[..., None, None], float(0))
        weights = F.softmax(logits, -1).view(N, Len_q, M, L, P)
        if reference_points.shape[-1] == 2:
            normalizer = torch.stack([input_spatial_shapes[..., 1], input_spatial_shapes[..., 0]], -1)
            locations = reference_points[:, :, None, :, None, :] + offsets / normalizer[None, None, None, :, None, :]
        elif reference_points.shape[-1] == 4:
            locations = reference_points[:, :, None, :, None, :2] \
                + offsets / P * reference_points[:, :, None, :, None, 2:] * 0.5
        else:
            raise ValueError("Last dim of reference_points must be 2 or 4, but get {} instead."
                             .format(reference_points.shape[-1]))

        if exact:      # fp32, or a 16-bit value up-cast as on the up-cast route below
            output = MSDeformAttnExactFunction.apply(value.float().contiguous(), input_spatial_shapes, input_level_start_index,
                                                     locations.float().contiguous(), weights.float().contiguous(), self.im2col_step,
                                                     getattr(self, "policy_slot", 0))
            return self.output_proj(output.to(value.dtype))
        if value.dtype in (torch.float16, torch.bfloat16):      # amp (ms_deform_attn.py:114-120)
            # Locations and weights are formed exactly as before and go in as fp32 (they already are under autocast; an all-fp16
            # module up-casts them as before); value goes in as it is and the op's output goes to output_proj in value's dtype.
            # The only difference from the up-cast route's results is the fp32 summation order before the ONE rounding of the
            # output and of grad_value; bf16 never ran on the up-cast route's fp32 entry points at all.
            loc32, w32 = locations.float().contiguous(), weights.float().contiguous()
            follows = torch.is_grad_enabled() and (value.requires_grad or loc32.requires_grad or w32.requires_grad)
            pixels = Len_q == Len_in and bool(MSDA.pyramid_check(input_spatial_shapes, input_level_start_index, Len_in) & 2)
            if getattr(self, "native_16bit", True) and MSDA.h16_supported(value, loc32, w32) \
                    and not _h16_takes_upcast_route(pixels, N * Len_q, follows):
                output = MSDeformAttnMixedFunction.apply(value.contiguous(), input_spatial_shapes, input_level_start_index,
                                                         loc32, w32, self.im2col_step)
                return self.output_proj(output)
            # the up-cast route: the op itself runs in fp32 on a copy of the value map
            output = MSDeformAttnFunction.apply(value.float(), input_spatial_shapes, input_level_start_index,
                                                loc32, w32, self.im2col_step, getattr(self, "policy_slot", 0))
            return self.output_proj(output.to(value.dtype))
        output = MSDeformAttnFunction.apply(value.contiguous(), input_spatial_shapes, input_level_start_index,
                                            locations.contiguous(), weights.contiguous(), self.im2col_step, getattr(self, "policy_slot", 0))
        return self.output_proj(output)


def convert_exact_backward(model, mode=True):
    """Set ``exact_backward = mode`` (False, True or "auto") on every ``MSDeformAttn`` below ``model`` (``model`` included);
    returns how many were set.  See the attribute's comment in ``MSDeformAttn.__init__`` and DESIGN.md 2.12c."""
    if not (mode is True or mode is False or mode == "auto"):
        raise ValueError("convert_exact_backward: mode must be False, True or 'auto', got {!r}".format(mode))
    done = 0
    for m in model.modules():
        if isinstance(m, MSDeformAttn):
            m.exact_backward = mode
            done += 1
    return done
