#!/usr/bin/env python
"""Generate tests/golden/self_attn.npz from the REFERENCE's own ``DINOTransformerDecoderLayer.forward_sa``
(detr_od/models/utils/transformer.py:793-816; the source is taken from the file with ``ast`` at run time and executed -- the
module itself imports mmcv, timm and cv2).  Runs on the CPU where the reference tree exists; what it writes is data.

    python tools/gen_self_attn_golden.py

``forward_sa`` runs unbound in float64 on a stand-in ``self`` that holds a seeded ``nn.MultiheadAttention`` (dropout 0.0, as
DINO builds it), ``nn.Dropout(0.0)`` and a seeded ``nn.LayerNorm``.  Inputs and weights are drawn in float32 and up-cast, so the
stored values are fp32-representable.

Per case ``<case>.``: ``heads``, ``tgt``, ``pos`` (L, B, E), ``mask`` (L, L) uint8 (absent: no mask), the weights
``in_proj_weight``, ``in_proj_bias``, ``out_w``, ``out_b``, ``ln_w``, ``ln_b``; recorded: ``tgt2`` (what ``self.self_attn``
returned, by a forward hook), ``out`` (what ``forward_sa`` returned) and, for the loss ``sum(out * G)`` with
``G = self_attn_ref64.grad_pattern(shape, 1)`` (not stored): ``g_tgt2`` (the gradient that reached the attention's output),
``g_tgt``, ``g_pos``, ``g_in_proj_bias``, ``g_out_b`` (the weights' gradients are left out to keep the file small).
"""
import ast
import os
import sys
import textwrap
import types

import numpy as np
import torch
from torch import nn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle.gen_golden import REF  # noqa: E402
sys.path.insert(0, os.path.join(ROOT, "tests"))
from self_attn_cases import dn_mask  # noqa: E402
from self_attn_ref64 import grad_pattern  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "self_attn.npz")
SRC = REF + "/detr_od/models/utils/transformer.py"


def _source(name, cls):
    src = open(SRC).read()
    tree = ast.parse(src)
    scope = next(n for n in ast.walk(tree) if isinstance(n, ast.ClassDef) and n.name == cls)
    for node in scope.body:
        if isinstance(node, ast.FunctionDef) and node.name == name:
            return textwrap.dedent(ast.get_source_segment(src, node, padded=True))
    raise KeyError(name)


def load_reference():
    from typing import Optional
    ns = {"torch": torch, "Tensor": torch.Tensor, "nn": nn, "Optional": Optional}
    exec(_source("forward_sa", "DINOTransformerDecoderLayer"), ns)
    return ns["forward_sa"]


def cases():
    rng = np.random.default_rng(20240611)
    out = {}

    def add(name, L, B, H, mask=None):
        E = 32 * H
        c = dict(heads=np.int64(H), tgt=rng.standard_normal((L, B, E)).astype(np.float32),
                 pos=rng.standard_normal((L, B, E)).astype(np.float32),
                 in_proj_weight=(rng.standard_normal((3 * E, E)) / np.sqrt(E)).astype(np.float32),
                 in_proj_bias=(rng.standard_normal(3 * E) * 0.1).astype(np.float32),
                 out_w=(rng.standard_normal((E, E)) / np.sqrt(E)).astype(np.float32),
                 out_b=(rng.standard_normal(E) * 0.1).astype(np.float32),
                 ln_w=(1 + 0.1 * rng.standard_normal(E)).astype(np.float32), ln_b=(0.1 * rng.standard_normal(E)).astype(np.float32))
        if mask is not None:
            c["mask"] = mask.astype(np.uint8)
        out[name] = c

    add("plain", 19, 1, 2)
    add("dn_mask", 46, 1, 2, dn_mask(3, 4, 22))
    add("two_images", 37, 2, 2, dn_mask(2, 3, 25))
    return out


def run(c, forward_sa):
    dt = torch.float64
    H, E = int(c["heads"]), c["tgt"].shape[2]
    T = lambda a: torch.from_numpy(a).to(dt)      # noqa: E731
    mha = nn.MultiheadAttention(E, H, dropout=0.0).to(dt)
    mha.in_proj_weight.data, mha.in_proj_bias.data = T(c["in_proj_weight"]), T(c["in_proj_bias"])
    mha.out_proj.weight.data, mha.out_proj.bias.data = T(c["out_w"]), T(c["out_b"])
    norm = nn.LayerNorm(E).to(dt)
    norm.weight.data, norm.bias.data = T(c["ln_w"]), T(c["ln_b"])
    rec = {}

    def hook(_m, _inp, outp):
        outp[0].retain_grad()
        rec["tgt2"] = outp[0]
    mha.register_forward_hook(hook)
    self = types.SimpleNamespace(self_attn=mha, decoder_sa_type="sa", dropout2=nn.Dropout(0.0), norm2=norm,
                                 with_pos_embed=lambda t, p: t if p is None else t + p)
    tgt, pos = T(c["tgt"]).requires_grad_(True), T(c["pos"]).requires_grad_(True)
    mask = torch.from_numpy(c["mask"].astype(bool)) if "mask" in c else None
    out = forward_sa(self, tgt, pos, self_attn_mask=mask)
    (out * torch.from_numpy(grad_pattern(out.shape, 1)).to(dt)).sum().backward()
    res = dict(tgt2=rec["tgt2"].detach(), out=out.detach(), g_tgt2=rec["tgt2"].grad, g_tgt=tgt.grad, g_pos=pos.grad,
               g_in_proj_bias=mha.in_proj_bias.grad, g_out_b=mha.out_proj.bias.grad)
    return {k: v.numpy() for k, v in res.items()}


def main():
    forward_sa = load_reference()
    out = {}
    for name, c in cases().items():
        for k, v in c.items():
            out[f"{name}.{k}"] = v
        for k, v in run(c, forward_sa).items():
            assert v.dtype == np.float64
            out[f"{name}.{k}"] = v
    np.savez_compressed(OUT, **out)
    print(f"wrote {OUT}: {len(out)} arrays, {os.path.getsize(OUT)} bytes")


if __name__ == "__main__":
    main()
