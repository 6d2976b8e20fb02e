"""The glue of the reference's transformer layers re-stated with stock torch modules (detr_od/models/utils/transformer.py:
``DINOTransformerEncoderLayer`` 601-642, ``DINOTransformerEncoder.forward`` 723-744, ``DINOTransformerDecoderLayer`` 748-873 and
the decoder's ``norm`` applied to every intermediate output): the residual adds, dropouts, LayerNorms, positional adds and the
FFN, with the attribute names the reference uses, so that ``semi_detr_amd.add_norm``'s layer-level forwards run on these modules
as they run on the reference's.  The attention branches are fixed linear maps of the same operands (``AttnStandIn``): only the
glue differs between the two sides of a comparison.

Test helper like consis_torch_restated.py: the baseline of tools/add_norm_probe.py and of tests/test_gpu_add_norm.py, never the
code under test.
"""
import copy

import torch
from torch import nn

D = 256


class AttnStandIn(nn.Module):
    """A fixed linear map in place of an attention: ``lin_q(query) + lin_v(value)`` (the value averaged over its tokens where
    the two have different lengths).  Called as MSDeformAttn is, or, with ``mha=True``, as ``nn.MultiheadAttention`` is."""

    def __init__(self, mha=False):
        super().__init__()
        self.mha = mha
        self.lin_q, self.lin_v = nn.Linear(D, D), nn.Linear(D, D)

    def forward(self, query, second, third, *rest, **kw):
        value = third
        dim = 0 if self.mha else 1
        v = self.lin_v(value)
        if value.shape[dim] != query.shape[dim]:
            v = v.mean(dim, keepdim=True)
        out = self.lin_q(query) + v
        return (out, None) if self.mha else out


def with_pos_embed(tensor, pos):
    return tensor if pos is None else tensor + pos


class EncoderLayer(nn.Module):
    def __init__(self, d_ffn=512, dropout=0.0):
        super().__init__()
        self.self_attn = AttnStandIn()
        self.dropout1, self.norm1 = nn.Dropout(dropout), nn.LayerNorm(D)
        self.linear1, self.activation, self.dropout2 = nn.Linear(D, d_ffn), nn.ReLU(), nn.Dropout(dropout)
        self.linear2, self.dropout3, self.norm2 = nn.Linear(d_ffn, D), nn.Dropout(dropout), nn.LayerNorm(D)

    def forward_ffn(self, src):
        src2 = self.linear2(self.dropout2(self.activation(self.linear1(src))))
        src = src + self.dropout3(src2)
        return self.norm2(src)

    def forward(self, src, pos, reference_points, spatial_shapes, level_start_index, key_padding_mask=None):
        src2 = self.self_attn(with_pos_embed(src, pos), reference_points, src, spatial_shapes, level_start_index, key_padding_mask)
        src = src + self.dropout1(src2)
        src = self.norm1(src)
        return self.forward_ffn(src)


class Encoder(nn.Module):
    def __init__(self, num_layers=2, d_ffn=512, dropout=0.0):
        super().__init__()
        self.layers = nn.ModuleList([EncoderLayer(d_ffn, dropout) for _ in range(num_layers)])
        self.num_layers, self.norm, self.two_stage_type, self.deformable_encoder = num_layers, None, 'standard', True

    @staticmethod
    def get_reference_points(spatial_shapes, valid_ratios, device):
        return None                                   # the stand-in attention reads none

    def forward(self, src, pos, spatial_shapes, level_start_index, valid_ratios, key_padding_mask,
                ref_token_index=None, ref_token_coord=None):
        output = src
        reference_points = self.get_reference_points(spatial_shapes, valid_ratios, device=src.device)
        for layer in self.layers:
            output = layer(src=output, pos=pos, reference_points=reference_points, spatial_shapes=spatial_shapes,
                           level_start_index=level_start_index, key_padding_mask=key_padding_mask)
        if self.norm is not None:
            output = self.norm(output)
        return output, None, None


class DecoderLayer(nn.Module):
    def __init__(self, d_ffn=512, dropout=0.0):
        super().__init__()
        self.module_seq = ['sa', 'ca', 'ffn']
        self.cross_attn = AttnStandIn()
        self.dropout1, self.norm1 = nn.Dropout(dropout), nn.LayerNorm(D)
        self.self_attn = AttnStandIn(mha=True)
        self.dropout2, self.norm2 = nn.Dropout(dropout), nn.LayerNorm(D)
        self.linear1, self.activation, self.dropout3 = nn.Linear(D, d_ffn), nn.ReLU(), nn.Dropout(dropout)
        self.linear2, self.dropout4, self.norm3 = nn.Linear(d_ffn, D), nn.Dropout(dropout), nn.LayerNorm(D)
        self.key_aware_type, self.decoder_sa_type = None, 'sa'

    def forward_ffn(self, tgt):
        tgt2 = self.linear2(self.dropout3(self.activation(self.linear1(tgt))))
        tgt = tgt + self.dropout4(tgt2)
        return self.norm3(tgt)

    def forward_sa(self, tgt, tgt_query_pos=None, self_attn_mask=None):
        q = k = with_pos_embed(tgt, tgt_query_pos)
        tgt2 = self.self_attn(q, k, tgt, attn_mask=self_attn_mask)[0]
        tgt = tgt + self.dropout2(tgt2)
        return self.norm2(tgt)

    def forward_ca(self, tgt, tgt_query_pos=None, tgt_reference_points=None, memory=None, memory_key_padding_mask=None,
                   memory_level_start_index=None, memory_spatial_shapes=None):
        tgt2 = self.cross_attn(with_pos_embed(tgt, tgt_query_pos).transpose(0, 1), tgt_reference_points.transpose(0, 1).contiguous(),
                               memory.transpose(0, 1), memory_spatial_shapes, memory_level_start_index,
                               memory_key_padding_mask).transpose(0, 1)
        tgt = tgt + self.dropout1(tgt2)
        return self.norm1(tgt)

    def forward(self, tgt, tgt_query_pos=None, tgt_query_sine_embed=None, tgt_key_padding_mask=None, tgt_reference_points=None,
                memory=None, memory_key_padding_mask=None, memory_level_start_index=None, memory_spatial_shapes=None,
                memory_pos=None, self_attn_mask=None, cross_attn_mask=None):
        for funcname in self.module_seq:
            if funcname == 'ffn':
                tgt = self.forward_ffn(tgt)
            elif funcname == 'ca':
                tgt = self.forward_ca(tgt, tgt_query_pos, tgt_reference_points, memory, memory_key_padding_mask,
                                      memory_level_start_index, memory_spatial_shapes)
            elif funcname == 'sa':
                tgt = self.forward_sa(tgt, tgt_query_pos, self_attn_mask)
            else:
                raise ValueError(f"module_seq holds {funcname!r}")
        return tgt


class DecoderStack(nn.Module):
    """The loop of ``DINOTransformerDecoder.forward`` without its box refinement: every layer's output goes through the one
    final ``norm`` into the list of intermediates.  ``layer_forward(layer, tgt, **kw)`` replaces the layers' own forward."""

    def __init__(self, num_layers=2, d_ffn=512, dropout=0.0):
        super().__init__()
        self.layers = nn.ModuleList([DecoderLayer(d_ffn, dropout) for _ in range(num_layers)])
        self.norm = nn.LayerNorm(D)

    def forward(self, tgt, query_pos, reference_points, memory, layer_forward=None):
        intermediate = []
        for layer in self.layers:
            kw = dict(tgt_query_pos=query_pos, tgt_reference_points=reference_points, memory=memory)
            tgt = layer(tgt, **kw) if layer_forward is None else layer_forward(layer, tgt, **kw)
            intermediate.append(self.norm(tgt))
        return intermediate


def randomize_norms(module, generator):
    """LayerNorm weights and biases away from 1 and 0, so that their gradients and the affine step are exercised"""
    with torch.no_grad():
        for m in module.modules():
            if isinstance(m, nn.LayerNorm) or type(m).__name__ == "LayerNorm":
                m.weight.copy_(1.0 + 0.3 * torch.randn(m.weight.shape, generator=generator))
                m.bias.copy_(0.2 * torch.randn(m.bias.shape, generator=generator))


def in_float64(module):
    return copy.deepcopy(module).double()
