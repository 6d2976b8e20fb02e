"""The stock op-by-op chain that ``semi_detr_amd.pyramid_inputs`` replaces, restated in plain torch: the image masks and their
nearest-neighbour resize per level, the HW sine encoding, the flatten / level row / concatenation loop, the valid ratios and the
encoder's reference points.  It is the "stock" side of the CPU and GPU tests and of tools/pyramid_inputs_probe.py: the same ops
in the same order as the model code, so torch's fp32 results of it are what a model without the fused op computes.

Test helper (not a conftest; imported by name).  Works on any device.
"""
import math

import torch
import torch.nn.functional as F
from torch import nn


class SineEncodingHW(nn.Module):
    """Sine / cosine position encoding with one temperature per axis; ``forward(mask)``: ``(bs, h, w)`` -> ``(bs, 2 * num_feats,
    h, w)`` fp32."""

    def __init__(self, num_feats, temperatureH=10000, temperatureW=10000, normalize=False, scale=2 * math.pi, eps=1e-6, offset=0.):
        super().__init__()
        self.num_feats, self.temperatureH, self.temperatureW = num_feats, temperatureH, temperatureW
        self.normalize, self.scale, self.eps, self.offset = normalize, scale, eps, offset

    def divisors(self, temperature, device):
        k = torch.arange(self.num_feats, dtype=torch.float32, device=device)
        return temperature ** (2 * (k // 2) / self.num_feats)

    def forward(self, mask):
        valid = 1 - mask.to(torch.int)
        down = valid.cumsum(1, dtype=torch.float32)
        along = valid.cumsum(2, dtype=torch.float32)
        if self.normalize:
            down = (down + self.offset) / (down[:, -1:, :] + self.eps) * self.scale
            along = (along + self.offset) / (along[:, :, -1:] + self.eps) * self.scale
        ax = along[:, :, :, None] / self.divisors(self.temperatureW, mask.device)
        ay = down[:, :, :, None] / self.divisors(self.temperatureH, mask.device)
        bs, h, w = mask.shape
        px = torch.stack((ax[..., 0::2].sin(), ax[..., 1::2].cos()), dim=4).view(bs, h, w, -1)
        py = torch.stack((ay[..., 0::2].sin(), ay[..., 1::2].cos()), dim=4).view(bs, h, w, -1)
        return torch.cat((py, px), dim=3).permute(0, 3, 1, 2)


def image_masks(img_shapes, batch_input_shape, device):
    """(N, H, W) fp32: 1 on the padding, 0 on the top-left ``(img_h, img_w)`` corner of each image"""
    masks = torch.ones((len(img_shapes), int(batch_input_shape[0]), int(batch_input_shape[1])), dtype=torch.float32, device=device)
    for n, (img_h, img_w) in enumerate(img_shapes):
        masks[n, :img_h, :img_w] = 0
    return masks


def level_masks(img_shapes, batch_input_shape, shapes, device):
    masks = image_masks(img_shapes, batch_input_shape, device)
    return [F.interpolate(masks[None], size=tuple(s)).to(torch.bool).squeeze(0) for s in shapes]


def valid_ratio(mask):
    _, h, w = mask.shape
    rows = torch.sum(~mask[:, :, 0], 1)
    cols = torch.sum(~mask[:, 0, :], 1)
    return torch.stack([cols.float() / w, rows.float() / h], -1)


def reference_points(spatial_shapes, valid_ratios, device):
    """the encoder's reference points; ``spatial_shapes``: the (L, 2) long tensor"""
    per_level = []
    for lvl, (h, w) in enumerate(spatial_shapes):
        ys, xs = torch.meshgrid(torch.linspace(0.5, h - 0.5, h, dtype=torch.float32, device=device),
                                torch.linspace(0.5, w - 0.5, w, dtype=torch.float32, device=device), indexing="ij")
        ys = ys.reshape(-1)[None] / (valid_ratios[:, None, lvl, 1] * h)
        xs = xs.reshape(-1)[None] / (valid_ratios[:, None, lvl, 0] * w)
        per_level.append(torch.stack((xs, ys), -1))
    points = torch.cat(per_level, 1)
    return points[:, :, None] * valid_ratios[:, None]


def chain(mlvl_masks, encoding, level_embed=None, want_reference_points=True):
    """The transformer's preparation loop on given level masks -> the dict of ``pos`` (N, S, C), ``mask_flatten``,
    ``valid_ratios``, ``reference_points``, ``spatial_shapes``, ``level_start_index``.  ``level_embed``: (L, C) or ``None``; it is
    added only where there is more than one level, as the transformer does."""
    device = mlvl_masks[0].device
    rows, flat, shapes = [], [], []
    for lvl, mask in enumerate(mlvl_masks):
        pos = encoding(mask)
        shapes.append(tuple(mask.shape[1:]))
        pos = pos.flatten(2).transpose(1, 2)
        if len(mlvl_masks) > 1 and level_embed is not None:
            pos = pos + level_embed[lvl].view(1, 1, -1)
        rows.append(pos)
        flat.append(mask.flatten(1))
    spatial_shapes = torch.as_tensor(shapes, dtype=torch.long, device=device)
    out = {"pos": torch.cat(rows, 1), "mask_flatten": torch.cat(flat, 1),
           "spatial_shapes": spatial_shapes,
           "level_start_index": torch.cat((spatial_shapes.new_zeros((1,)), spatial_shapes.prod(1).cumsum(0)[:-1])),
           "valid_ratios": torch.stack([valid_ratio(m) for m in mlvl_masks], 1)}
    if want_reference_points:
        out["reference_points"] = reference_points(spatial_shapes, out["valid_ratios"], device)
    return out


def chain_from_sizes(img_shapes, batch_input_shape, shapes, encoding, level_embed=None, device="cpu", want_reference_points=True):
    return chain(level_masks(img_shapes, batch_input_shape, shapes, device), encoding, level_embed, want_reference_points)
