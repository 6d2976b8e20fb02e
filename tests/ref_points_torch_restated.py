"""The decoder's reference-point chain re-stated line by line in stock torch (detr_od/models/utils/transformer.py:
``inverse_sigmoid`` 435-451, ``gen_sineembed_for_position`` 467-493, ``MLP`` 453-465, ``DINOTransformerDecoder.forward``
947-1045) and the head's coordinate loop (dino_detr_ssod_head.py:393-398), with the attribute names the reference uses, so that
``semi_detr_amd.ref_points.decoder_forward`` runs on ``Decoder`` as it runs on the reference's module.  The decoder layers are
those of add_norm_torch_restated.py with a cross-attention stand-in that also reads the reference points.

Test helper like add_norm_torch_restated.py: the baseline of tools/ref_points_probe.py and of tests/test_gpu_ref_points.py, never
the code under test.  ``MUTANTS`` name deliberate mistakes of the restatement; tests/test_ref_points_ref.py shows that the float64
statement rejects each.
"""
import math

import numpy as np
import torch
import torch.nn.functional as F
from torch import nn

import add_norm_torch_restated as A

D = A.D
MUTANTS = ("sin_cos_swapped", "xy_block_order", "dim_t_j", "ratio_after_embed", "no_eps", "eps_on_x2_only", "clamp_grad_exclusive",
           "w_by_vr1")


def inverse_sigmoid(x, eps=1e-5, mutant=None):
    x = x.clamp(min=0, max=1)
    if mutant == "clamp_grad_exclusive":              # the same values; the gradient stops AT the bound as well
        x1 = torch.where(x > eps, x, torch.full_like(x, eps))
        x2 = torch.where(1 - x > eps, 1 - x, torch.full_like(x, eps))
        return torch.log(x1 / x2)
    x1 = x if mutant in ("no_eps", "eps_on_x2_only") else x.clamp(min=eps)
    x2 = (1 - x) if mutant == "no_eps" else (1 - x).clamp(min=eps)
    return torch.log(x1 / x2)


def gen_sineembed_for_position(pos_tensor, mutant=None):
    scale = 2 * math.pi
    dim_t = torch.arange(128, dtype=torch.float32, device=pos_tensor.device)
    dim_t = 10000 ** (2 * (dim_t if mutant == "dim_t_j" else dim_t // 2) / 128)
    if pos_tensor.dtype == torch.float64:
        dim_t = dim_t.double()                        # the fp32 table, exactly, in a float64 evaluation
    first, second = (torch.cos, torch.sin) if mutant == "sin_cos_swapped" else (torch.sin, torch.cos)

    def block(k):
        embed = pos_tensor[:, :, k] * scale
        pos = embed[:, :, None] / dim_t
        return torch.stack((first(pos[:, :, 0::2]), second(pos[:, :, 1::2])), dim=3).flatten(2)

    pos_x, pos_y = block(0), block(1)
    if mutant == "xy_block_order":
        pos_x, pos_y = pos_y, pos_x
    if pos_tensor.size(-1) == 2:
        pos = torch.cat((pos_y, pos_x), dim=2)
    elif pos_tensor.size(-1) == 4:
        pos = torch.cat((pos_y, pos_x, block(2), block(3)), dim=2)
    else:
        raise ValueError("Unknown pos_tensor shape(-1):{}".format(pos_tensor.size(-1)))
    return pos


def reference_inputs(reference_points, valid_ratios, mutant=None):
    """transformer.py:979-985 -> (reference_points_input, query_sine_embed)"""
    if reference_points.shape[-1] == 4:
        second = valid_ratios.flip(-1) if mutant == "w_by_vr1" else valid_ratios
        reference_points_input = reference_points[:, :, None] * torch.cat([valid_ratios, second], -1)[None, :]
    else:
        assert reference_points.shape[-1] == 2
        reference_points_input = reference_points[:, :, None] * valid_ratios[None, :]
    if mutant == "ratio_after_embed":
        query_sine_embed = gen_sineembed_for_position(reference_points) * valid_ratios[None, :, 0, 0:1]
    else:
        query_sine_embed = gen_sineembed_for_position(reference_points_input[:, :, 0, :], mutant)
    return reference_points_input, query_sine_embed


def refine(delta, reference, eps=1e-5, mutant=None):
    """transformer.py:1029-1032"""
    reference_before_sigmoid = inverse_sigmoid(reference, eps, mutant)
    outputs_unsig = delta + reference_before_sigmoid
    return outputs_unsig.sigmoid()


def box_outputs(fc_reg, hs, reference):
    """dino_detr_ssod_head.py:393-398"""
    outputs_coord_list = []
    for dec_lid, (layer_ref_sig, layer_fc_reg, layer_hs) in enumerate(zip(reference[:-1], fc_reg, hs)):
        layer_delta_unsig = layer_fc_reg(layer_hs)
        layer_outputs_unsig = layer_delta_unsig + inverse_sigmoid(layer_ref_sig)
        layer_outputs_unsig = layer_outputs_unsig.sigmoid()
        outputs_coord_list.append(layer_outputs_unsig)
    return torch.stack(outputs_coord_list)


def evaluate(case, dtype=torch.float32, device="cpu", mutant=None, grads=True):
    """A case of tests/ref_points_cases.py through the restated ops and torch.autograd, every operand in ``dtype`` (the case's
    own 16-bit dtypes are not reproduced: the arrays hold the rounded numbers): ``{"new_ref": [...], "ref_input", "embed",
    "g_delta": [...], "g_ref": [...]}`` as numpy arrays in the logical shapes."""
    mode, eps = case["mode"], float(np.float32(case["eps"]))

    def leaf(a):
        return torch.from_numpy(np.asarray(a)).to(device=device, dtype=dtype).requires_grad_(True)

    got = {"new_ref": [], "g_delta": [], "g_ref": []}
    for s, seg in enumerate(case["segments"]):
        ref = leaf(seg["ref"])
        delta = leaf(seg["delta"]) if mode == 2 else None
        y = ref if mode == 0 else ref.sigmoid() if mode == 1 else refine(delta, ref, eps, mutant)
        outs, seeds = [y], [torch.from_numpy(seg["g_new"]).to(device=device, dtype=dtype)]
        got["new_ref"].append(y.detach().cpu().numpy())
        if s == 0 and case["vr"] is not None:
            vr = torch.from_numpy(case["vr"]).to(device=device, dtype=dtype)
            ref_input, embed = reference_inputs(y, vr, mutant)
            got["ref_input"], got["embed"] = ref_input.detach().cpu().numpy(), embed.detach().cpu().numpy()
            outs += [ref_input, embed]
            seeds += [torch.from_numpy(case[k]).to(device=device, dtype=dtype) for k in ("g_ref_input", "g_embed")]
        if grads:
            torch.autograd.backward(outs, seeds)
            got["g_ref"].append(ref.grad.cpu().numpy())
            got["g_delta"].append(None if delta is None else delta.grad.cpu().numpy())
    if mode == 0:
        del got["new_ref"]
    if not grads:
        del got["g_delta"], got["g_ref"]
    return got


class MLP(nn.Module):
    def __init__(self, input_dim, hidden_dim, output_dim, num_layers):
        super().__init__()
        self.num_layers = num_layers
        h = [hidden_dim] * (num_layers - 1)
        self.layers = nn.ModuleList(nn.Linear(n, k) for n, k in zip([input_dim] + h, h + [output_dim]))

    def forward(self, x):
        for i, layer in enumerate(self.layers):
            x = F.relu(layer(x)) if i < self.num_layers - 1 else layer(x)
        return x


class CrossAttnStandIn(nn.Module):
    """``A.AttnStandIn`` called as MSDeformAttn is, plus a fixed linear map of the query's reference points ``(bs, nq, L,
    width)``, so that ``reference_points_input`` reaches the output."""

    def __init__(self, levels, width):
        super().__init__()
        self.base, self.lin_r = A.AttnStandIn(), nn.Linear(levels * width, D)

    def forward(self, query, reference_points, value, *rest, **kw):
        return self.base(query, reference_points, value) + self.lin_r(reference_points.flatten(2))


class Decoder(nn.Module):
    """The minimal ``DINOTransformerDecoder``: the reference's attribute names and its forward, deformable branch."""

    def __init__(self, num_layers=2, levels=4, query_dim=4, d_ffn=512):
        super().__init__()
        self.layers = nn.ModuleList([A.DecoderLayer(d_ffn) for _ in range(num_layers)])
        for layer in self.layers:
            layer.cross_attn = CrossAttnStandIn(levels, query_dim)
        self.num_layers, self.norm, self.return_intermediate, self.query_dim = num_layers, nn.LayerNorm(D), True, query_dim
        self.num_feature_levels, self.d_model = levels, D
        self.ref_point_head = MLP(query_dim // 2 * D, D, D, 2)
        self.query_pos_sine_scale, self.query_scale, self.ref_anchor_head = None, None, None
        self.modulate_hw_attn, self.deformable_decoder = True, True
        self.decoder_query_perturber, self.box_pred_damping, self.dec_layer_number = None, None, None
        self.dec_layer_dropout_prob, self.rm_detach = None, None

    def forward(self, tgt, memory, tgt_mask=None, memory_mask=None, tgt_key_padding_mask=None, memory_key_padding_mask=None,
                pos=None, refpoints_unsigmoid=None, level_start_index=None, spatial_shapes=None, valid_ratios=None, fc_reg=None,
                fc_cls=None):
        output = tgt
        intermediate = []
        reference_points = refpoints_unsigmoid.sigmoid()
        ref_points = [reference_points]
        for layer_id, layer in enumerate(self.layers):
            reference_points_input, query_sine_embed = reference_inputs(reference_points, valid_ratios)
            raw_query_pos = self.ref_point_head(query_sine_embed)
            pos_scale = self.query_scale(output) if self.query_scale is not None else 1
            query_pos = pos_scale * raw_query_pos
            output = layer(tgt=output, tgt_query_pos=query_pos, tgt_query_sine_embed=query_sine_embed,
                           tgt_key_padding_mask=tgt_key_padding_mask, tgt_reference_points=reference_points_input, memory=memory,
                           memory_key_padding_mask=memory_key_padding_mask, memory_level_start_index=level_start_index,
                           memory_spatial_shapes=spatial_shapes, memory_pos=pos, self_attn_mask=tgt_mask,
                           cross_attn_mask=memory_mask)
            if fc_reg is not None:
                reference_before_sigmoid = inverse_sigmoid(reference_points)
                delta_unsig = fc_reg[layer_id](output)
                outputs_unsig = delta_unsig + reference_before_sigmoid
                new_reference_points = outputs_unsig.sigmoid()
                reference_points = new_reference_points.detach()
                ref_points.append(new_reference_points)
            intermediate.append(self.norm(output))
        return [[itm_out.transpose(0, 1) for itm_out in intermediate], [itm_refpoint.transpose(0, 1) for itm_refpoint in ref_points]]


def box_heads(num_layers, width=4):
    """``fc_reg``: one ``MLP(256, 256, width, 3)`` per layer, as the head builds them"""
    return nn.ModuleList([MLP(D, D, width, 3) for _ in range(num_layers)])
