"""Multi-scale deformable attention re-stated in stock torch ops, from the formula (tests/msda_ref64.py states the same operation
in numpy): the module of detr_od/models/utils/ops/modules/ms_deform_attn.py:30-126 with its constructor arguments, sub-module
names and ``state_dict`` keys, so that a model built on it loads into ``semi_detr_amd.MSDeformAttn`` with ``strict=True``.

    value = masked_fill(value_proj(input), padding, 0)                              (N, S, M, D)
    a     = softmax over the L * P logits of a (query, head)                        (N, Lq, M, L, P)
    loc   = ref[..., :2] + off / (W_l, H_l)                  for 2-d points         (N, Lq, M, L, P, 2)
          = ref[..., :2] + off / P * ref[..., 2:] * 0.5      for 4-d boxes
    out   = output_proj(sum over (l, p) of a * bilinear(value of level l at x = loc_x W_l - 0.5, y = loc_y H_l - 0.5))

with zero padding outside the map (``align_corners=False``).  A level's rows are ``[level_start_index[l], + H_l W_l)``: the index
table is read, not recomputed from the shapes.

amp (ms_deform_attn.py:114-120): a 16-bit ``value`` (what ``value_proj`` returns under autocast) is up-cast, the sampling runs in
fp32 on fp32 locations and weights, and the result goes back to the 16-bit type in front of ``output_proj``.  The reference tests
for fp16 only and hands a bf16 map to an op that has no bf16 kernels; here bf16 takes the fp16 branch, as in the product.

Test helper like the other ``*_torch_restated.py`` files: the baseline of tests/detector_chain_cases.py, never the code under
test.  Runs in fp32, under autocast and in float64, on the CPU and the GPU, with autograd.
"""
import math

import torch
import torch.nn.functional as F
from torch import nn


def sample_level(value_l, H, W, loc_l):
    """Bilinear samples of one level.  value_l (N, H * W, M, D), loc_l (N, Lq, M, P, 2) normalised (x, y) -> (N, Lq, M, P, D).
    ``grid_sample`` with ``align_corners=False`` reads pixel ``(g + 1) * W / 2 - 0.5`` for a grid coordinate g: g = 2 loc - 1."""
    N, _, M, D = value_l.shape
    Lq, P = loc_l.shape[1], loc_l.shape[3]
    maps = value_l.permute(0, 2, 3, 1).reshape(N * M, D, H, W)
    grid = (2.0 * loc_l - 1.0).permute(0, 2, 1, 3, 4).reshape(N * M, Lq, P, 2)
    got = F.grid_sample(maps, grid, mode="bilinear", padding_mode="zeros", align_corners=False)      # (N * M, D, Lq, P)
    return got.reshape(N, M, D, Lq, P).permute(0, 3, 1, 4, 2)


def core(value, spatial_shapes, level_start_index, locations, weights):
    """value (N, S, M, D), locations (N, Lq, M, L, P, 2), weights (N, Lq, M, L, P) -> (N, Lq, M * D)"""
    N, Lq, M = locations.shape[:3]
    out = 0
    for l, ((H, W), start) in enumerate(zip(spatial_shapes.tolist(), level_start_index.tolist())):
        sampled = sample_level(value[:, start:start + H * W], H, W, locations[:, :, :, l])
        out = out + (sampled * weights[:, :, :, l, :, None]).sum(3)
    return out.reshape(N, Lq, -1)


def locations_of(reference_points, offsets, spatial_shapes, n_points):
    if reference_points.shape[-1] == 2:
        extent = torch.stack([spatial_shapes[:, 1], spatial_shapes[:, 0]], -1)                       # (W, H) per level
        return reference_points[:, :, None, :, None, :] + offsets / extent[None, None, None, :, None, :]
    if reference_points.shape[-1] == 4:
        centre, size = reference_points[:, :, None, :, None, :2], reference_points[:, :, None, :, None, 2:]
        return centre + offsets / n_points * size * 0.5
    raise ValueError(f"reference points of width {reference_points.shape[-1]}: 2 (points) or 4 (boxes)")


class MSDeformAttn(nn.Module):
    def __init__(self, d_model=256, n_levels=4, n_heads=8, n_points=4):
        super().__init__()
        if d_model % n_heads != 0:
            raise ValueError(f"{n_heads} heads do not divide d_model = {d_model}")
        self.im2col_step = 64
        self.d_model, self.n_levels, self.n_heads, self.n_points = d_model, n_levels, n_heads, n_points
        self.sampling_offsets = nn.Linear(d_model, n_heads * n_levels * n_points * 2)
        self.attention_weights = nn.Linear(d_model, n_heads * n_levels * n_points)
        self.value_proj = nn.Linear(d_model, d_model)
        self.output_proj = nn.Linear(d_model, d_model)
        self._reset_parameters()

    def _reset_parameters(self):
        """head m looks along 2 pi m / M (the longer coordinate 1), point i at i + 1 steps; the weights that form offsets and
        logits start at 0, the two projections xavier-uniform"""
        M, L, P = self.n_heads, self.n_levels, self.n_points
        angle = torch.arange(M, dtype=torch.float32) * (2.0 * math.pi / M)
        step = torch.stack([angle.cos(), angle.sin()], -1)
        step = step / step.abs().max(-1, keepdim=True)[0]
        bias = step[:, None, None, :] * torch.arange(1, P + 1, dtype=torch.float32)[None, None, :, None]
        with torch.no_grad():
            self.sampling_offsets.weight.zero_()
            self.sampling_offsets.bias.copy_(bias.expand(M, L, P, 2).reshape(-1))
            self.attention_weights.weight.zero_()
            self.attention_weights.bias.zero_()
            nn.init.xavier_uniform_(self.value_proj.weight)
            self.value_proj.bias.zero_()
            nn.init.xavier_uniform_(self.output_proj.weight)
            self.output_proj.bias.zero_()

    def forward(self, query, reference_points, input_flatten, input_spatial_shapes, input_level_start_index,
                input_padding_mask=None):
        N, Lq, _ = query.shape
        S = input_flatten.shape[1]
        assert int((input_spatial_shapes[:, 0] * input_spatial_shapes[:, 1]).sum()) == S
        M, L, P = self.n_heads, self.n_levels, self.n_points
        value = self.value_proj(input_flatten)
        if input_padding_mask is not None:
            value = value.masked_fill(input_padding_mask.unsqueeze(-1), 0.0)
        value = value.view(N, S, M, self.d_model // M)
        offsets = self.sampling_offsets(query).view(N, Lq, M, L, P, 2)
        weights = F.softmax(self.attention_weights(query).view(N, Lq, M, L * P), -1).view(N, Lq, M, L, P)
        locations = locations_of(reference_points, offsets, input_spatial_shapes, P)
        if value.dtype in (torch.float16, torch.bfloat16):                                           # amp
            out = core(value.float(), input_spatial_shapes, input_level_start_index, locations.float(), weights.float())
            return self.output_proj(out.to(value.dtype))
        return self.output_proj(core(value, input_spatial_shapes, input_level_start_index, locations, weights))
