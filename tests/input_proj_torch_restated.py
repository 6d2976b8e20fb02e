"""The reference's input projection re-stated with stock torch modules and ops: the ``input_proj`` ModuleList of
``nn.Sequential(Conv2d, GroupNorm(32, 256))`` (dino_detr_ssod_head.py:251-259, dino_detr_head.py:223-231), the loop that builds
``srcs`` (dino_detr_ssod_head.py:359-377), and the transformer's ``src.flatten(2).transpose(1, 2)``, ``torch.cat(src_flatten, 1)``,
``spatial_shapes`` / ``level_start_index`` and the ``src + pos`` in front of encoder layer 0
(detr_od/models/utils/transformer.py:1276-1291, 635).

Test helper like add_norm_torch_restated.py: the baseline of tools/input_proj_probe.py and of tests/test_gpu_input_proj.py,
never the code under test.  The modules are shared with the fused side (``semi_detr_amd.project_pyramid`` runs on them).
"""
import copy

import torch
from torch import nn

D = 256


def build_input_proj(backbone_channels, num_feature_levels, embed_dims=D):
    """dino_detr_ssod_head.py:246-262"""
    input_proj_list = []
    for in_channels in backbone_channels:
        input_proj_list.append(nn.Sequential(nn.Conv2d(in_channels, embed_dims, kernel_size=1), nn.GroupNorm(32, embed_dims)))
    for _ in range(num_feature_levels - len(backbone_channels)):
        input_proj_list.append(nn.Sequential(nn.Conv2d(in_channels, embed_dims, kernel_size=3, stride=2, padding=1),
                                             nn.GroupNorm(32, embed_dims)))
        in_channels = embed_dims
    return nn.ModuleList(input_proj_list)


def randomize_norms(module, generator):
    """GroupNorm weights and biases away from 1 and 0, distinct per level"""
    with torch.no_grad():
        for m in module.modules():
            if isinstance(m, nn.GroupNorm):
                m.weight.copy_(1.0 + 0.3 * torch.randn(m.weight.shape, generator=generator))
                m.bias.copy_(0.2 * torch.randn(m.bias.shape, generator=generator))


def srcs_of(input_proj, mlvl_feats, num_feature_levels):
    """dino_detr_ssod_head.py:359-377, ``srcs`` only"""
    srcs = []
    for l, feat in enumerate(mlvl_feats):
        srcs.append(input_proj[l](feat))
    if num_feature_levels > len(srcs):
        _len_srcs = len(srcs)
        for l in range(_len_srcs, num_feature_levels):
            if l == _len_srcs:
                src = input_proj[l](mlvl_feats[-1])
            else:
                src = input_proj[l](srcs[-1])
            srcs.append(src)
    return srcs


def flatten_srcs(srcs):
    """transformer.py:1270-1291: ``(src_flatten, spatial_shapes, level_start_index)``"""
    src_flatten, spatial_shapes = [], []
    for src in srcs:
        bs, c, h, w = src.shape
        spatial_shapes.append((h, w))
        src_flatten.append(src.flatten(2).transpose(1, 2))
    src_flatten = torch.cat(src_flatten, 1)
    spatial_shapes = torch.as_tensor(spatial_shapes, dtype=torch.long, device=src_flatten.device)
    level_start_index = torch.cat((spatial_shapes.new_zeros((1, )), spatial_shapes.prod(1).cumsum(0)[:-1]))
    return src_flatten, spatial_shapes, level_start_index


def norm_tokens(xs, norms, pos=None):
    """the norm stage alone: ``norms[l](xs[l])``, flatten, transpose, cat and, with ``pos``, the layer-0 ``src + pos``
    (transformer.py:635) -> ``(tokens, q or None)``"""
    tokens = flatten_srcs([norm(x) for x, norm in zip(xs, norms)])[0]
    return tokens, None if pos is None else tokens + pos


def project(input_proj, mlvl_feats, num_feature_levels, pos=None):
    """``srcs_of`` + ``flatten_srcs`` + ``src + pos`` -> ``(tokens, q or None, spatial_shapes, level_start_index)``"""
    tokens, spatial_shapes, level_start_index = flatten_srcs(srcs_of(input_proj, mlvl_feats, num_feature_levels))
    return tokens, None if pos is None else tokens + pos, spatial_shapes, level_start_index


def in_float64(module):
    return copy.deepcopy(module).double()
