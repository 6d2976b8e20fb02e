#!/usr/bin/env python
"""Generate tests/golden/query_select.npz from the REFERENCE's own ``gen_encoder_output_proposals`` and
``DINOTransformer.forward`` (detr_od/models/utils/transformer.py:525-575, 1255-1406; the sources are taken from the file with
``ast`` at run time and executed -- the module itself imports mmcv, timm and cv2).  Runs on the CPU where the reference tree
exists; what it writes is data.

    python tools/gen_query_select_golden.py

``forward`` runs unbound on a stand-in ``self`` whose encoder returns the case's memory and whose decoder records its
arguments; ``gen_encoder_output_proposals`` and ``torch.topk`` are wrapped so that their results are recorded too.  In all
cases but ``forward`` the heads are stand-ins that return the case's logits / box deltas and ``enc_output`` /
``enc_output_norm`` are identities, so the keys are exactly the given numbers (ties, NaN); in ``forward`` they are seeded
``Linear`` / ``LayerNorm`` modules whose weights are stored.  Every case runs twice: in float32 (``*32``: decisions -- valid
flags, top-k values and indices) and in float64 (``*64``: values and gradients; ``torch.float32`` reads as float64 there, so
the anchors are float64 too).  Inputs are drawn in float32 and up-cast.

Per case ``<case>.``: ``shapes``, ``mask`` (N, S) uint8, ``memory``, ``logits``, ``reg`` (the head outputs; absent in
``forward``), ``dn_ref`` / ``dn_tgt`` (the dn part, may be absent), ``tgt_embed``, ``k``; recorded: ``prop32/64``, ``outmem32``,
``topv32``, ``topi32``, ``topi64``, ``dec_tgt32/64``, ``dec_ref32/64`` (the decoder's tgt / refpoints_unsigmoid, batch first),
``hs_enc32/64``, ``ref_enc32/64``, ``init32/64``; gradients of ``sum(hs_enc * G1) + sum(ref_enc * G2)`` with
``G = query_select_ref64.grad_pattern(shape, 1 / 2)`` (not stored) in float64: ``g_memory``, ``g_reg``.
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
from query_select_ref64 import grad_pattern  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "query_select.npz")
SRC = REF + "/detr_od/models/utils/transformer.py"


def _source(name, cls=None):
    src = open(SRC).read()
    tree = ast.parse(src)
    scope = tree
    if cls is not None:
        scope = next(n for n in ast.walk(tree) if isinstance(n, ast.ClassDef) and n.name == cls)
    for node in scope.body:
        if isinstance(node, ast.FunctionDef) and node.name == name:
            return textwrap.dedent(ast.get_source_segment(src, node, padded=True))
    raise KeyError(name)


class TorchProxy:
    """``torch`` as the reference's functions see it: ``topk`` recorded, ``float32`` -> float64 in the float64 run."""

    def __init__(self, rec, f64):
        self._rec, self._f64 = rec, f64

    def __getattr__(self, k):
        if k == "float32" and self._f64:
            return torch.float64
        if k == "topk":
            def topk(*a, **kw):
                v, i = torch.topk(*a, **kw)
                self._rec["topv"], self._rec["topi"] = v.detach(), i.detach()
                return v, i
            return topk
        return getattr(torch, k)


def load_reference(rec, f64):
    proxy = TorchProxy(rec, f64)
    ns = {"torch": proxy, "Tensor": torch.Tensor, "nn": nn}
    exec(_source("gen_encoder_output_proposals"), ns)
    gen = ns["gen_encoder_output_proposals"]

    def recording_gen(*a, **kw):
        om, op = gen(*a, **kw)
        rec["outmem"], rec["prop"] = om.detach(), op.detach()
        return om, op
    ns["gen_encoder_output_proposals"] = recording_gen
    exec(_source("forward", "DINOTransformer"), ns)
    return ns["forward"]


def band_mask(shapes, fracs):
    """(N, S) bool: image n occupies the top-left (fh, fw) fraction of every level (ceil), the rest is padding."""
    rows = []
    for fh, fw in fracs:
        parts = []
        for H, W in shapes:
            m = np.ones((H, W), bool)
            m[:int(np.ceil(H * fh)), :int(np.ceil(W * fw))] = False
            parts.append(m.reshape(-1))
        rows.append(np.concatenate(parts))
    return np.stack(rows)


def cases():
    rng = np.random.default_rng(20240607)
    out = {}

    def add(name, shapes, mask, C, k, D=8, dn=0, real_heads=False, logits=None):
        N, S = mask.shape
        c = dict(shapes=np.asarray(shapes, np.int64), mask=mask.astype(np.uint8), k=np.int64(k),
                 memory=rng.standard_normal((N, S, D)).astype(np.float32),
                 tgt_embed=rng.standard_normal((k, D)).astype(np.float32))
        if not real_heads:
            c["logits"] = rng.standard_normal((N, S, C)).astype(np.float32) if logits is None else logits(N, S, C)
            c["reg"] = (rng.standard_normal((N, S, 4)) * 0.5).astype(np.float32)
        else:
            c.update(w_out=(rng.standard_normal((D, D)) / np.sqrt(D)).astype(np.float32),
                     b_out=(rng.standard_normal(D) * 0.1).astype(np.float32), ln_w=(1 + 0.1 * rng.standard_normal(D)).astype(np.float32),
                     ln_b=(0.1 * rng.standard_normal(D)).astype(np.float32), w_cls=rng.standard_normal((C, D)).astype(np.float32),
                     b_cls=rng.standard_normal(C).astype(np.float32), w_reg=(rng.standard_normal((4, D)) * 0.3).astype(np.float32),
                     b_reg=(rng.standard_normal(4) * 0.1).astype(np.float32))
        if dn:
            c["dn_ref"] = rng.standard_normal((N, dn, 4)).astype(np.float32)
            c["dn_tgt"] = rng.standard_normal((N, dn, D)).astype(np.float32)
        out[name] = c

    sh = [(6, 7)]
    add("one_level", sh, band_mask(sh, [(1, 1), (0.7, 0.6)]), 1, 10)
    sh = [(12, 16), (6, 8), (3, 4), (2, 2)]
    add("four_levels", sh, band_mask(sh, [(1, 0.8), (0.6, 1)]), 20, 30, dn=6)
    sh = [(16, 12), (8, 6), (4, 3), (2, 2), (1, 1)]
    add("five_levels", sh, band_mask(sh, [(0.9, 0.5), (1, 1)]), 80, 20)
    sh = [(50, 84)]                                         # valid_H = 50: 0.5 / 50 against 0.01; and no mask bit at all
    add("h50_no_mask", sh, np.zeros((1, 4200), bool), 1, 64, D=4)
    sh = [(9, 1), (3, 2)]
    add("w1_level", sh, band_mask(sh, [(0.8, 1)]), 20, 6)
    sh = [(8, 9), (4, 5)]                                   # holes in row 0 / column 0: the counts differ from the extents
    m = band_mask(sh, [(1, 1), (0.8, 0.9)])
    m[0, [2, 5]] = True                                     # row 0 of level 0, image 0
    m[0, [9 * 3, 9 * 4]] = True                             # column 0
    m[1, 72 + 1] = True                                     # row 0 of level 1, image 1
    add("nonband", sh, m, 20, 12)
    sh = [(6, 6), (3, 3)]
    m = band_mask(sh, [(1, 1), (0.7, 0.7)])
    m[1, 36:] = True                                        # image 1: level 1 fully masked (0 / 0 counts)
    add("masked_level", sh, m, 20, 8)
    sh = [(4, 5)]
    add("k_eq_S", sh, band_mask(sh, [(1, 1)]), 20, 20)
    sh = [(6, 8), (3, 4)]                                   # fewer valid tokens than k: the zeroed rows tie

    def bias_rows(N, S, C):
        lg = rng.standard_normal((N, S, C)).astype(np.float32)
        lg[band_mask(sh, [(0.5, 0.5), (0.4, 0.7)])] = np.linspace(-1, 0.25, C, dtype=np.float32)
        return lg
    add("k_gt_valid", sh, band_mask(sh, [(0.5, 0.5), (0.4, 0.7)]), 20, 40, logits=bias_rows)
    sh = [(5, 6)]
    add("ties", sh, band_mask(sh, [(1, 1), (1, 0.9)]), 20, 12,
        logits=lambda N, S, C: rng.integers(-3, 3, (N, S, C)).astype(np.float32) - (rng.random((N, S, 1)) < 0.5) * 2.0)

    def with_nan(N, S, C):
        lg = rng.standard_normal((N, S, C)).astype(np.float32)
        lg[0, 17, 3] = np.nan
        lg[1, 4, 0] = -0.0
        return lg
    add("nan_key", sh, band_mask(sh, [(1, 1), (1, 1)]), 80, 5, logits=with_nan)
    sh = [(8, 10), (4, 5)]
    add("forward", sh, band_mask(sh, [(1, 1), (0.75, 0.6)]), 20, 12, D=16, dn=5, real_heads=True)
    return out


def run(c, f64):
    dt = torch.float64 if f64 else torch.float32
    rec = {}
    forward = load_reference(rec, f64)
    shapes = [tuple(int(v) for v in r) for r in c["shapes"]]
    mask = torch.from_numpy(c["mask"].astype(bool))
    N, S = mask.shape
    D, k = c["memory"].shape[2], int(c["k"])
    memory = torch.from_numpy(c["memory"]).to(dt).requires_grad_(True)
    T = lambda a: torch.from_numpy(a).to(dt)      # noqa: E731
    srcs, masks, pos, at = [], [], [], 0
    for H, W in shapes:
        srcs.append(torch.zeros(N, D, H, W, dtype=dt))
        pos.append(torch.zeros(N, D, H, W, dtype=dt))
        masks.append(mask[:, at:at + H * W].reshape(N, H, W))
        at += H * W
    leaves = {}
    if "logits" in c:
        logits, reg = T(c["logits"]), T(c["reg"]).requires_grad_(True)
        leaves["reg"] = reg
        fc_cls, fc_reg = (lambda x: logits), (lambda x: reg)
        enc_output = enc_norm = (lambda x: x)
    else:
        def lin(w, b):
            m = nn.Linear(w.shape[1], w.shape[0]).to(dt)
            m.weight.data, m.bias.data = T(w), T(b)
            return m
        enc_output, fc_cls, fc_reg = lin(c["w_out"], c["b_out"]), lin(c["w_cls"], c["b_cls"]), lin(c["w_reg"], c["b_reg"])
        enc_norm = nn.LayerNorm(D).to(dt)
        enc_norm.weight.data, enc_norm.bias.data = T(c["ln_w"]), T(c["ln_b"])
    emb = nn.Embedding(k, D).to(dt)
    emb.weight.data = T(c["tgt_embed"])

    def decoder(**kw):
        rec["dec_tgt"], rec["dec_ref"] = kw["tgt"].transpose(0, 1).detach(), kw["refpoints_unsigmoid"].transpose(0, 1).detach()
        return None, None
    self = types.SimpleNamespace(num_feature_levels=len(shapes), level_embed=None, two_stage_type="standard",
                                 get_valid_ratio=lambda m: torch.ones(N, 2, dtype=dt), encoder=lambda *a, **kw: (memory, None, None),
                                 enc_output=enc_output, enc_output_norm=enc_norm, num_queries=k, d_model=D, embed_init_tgt=True,
                                 tgt_embed=emb, decoder=decoder)
    dn_ref = T(c["dn_ref"]) if "dn_ref" in c else None
    dn_tgt = T(c["dn_tgt"]) if "dn_tgt" in c else None
    _, _, hs_enc, ref_enc, init = forward(self, srcs, masks, dn_ref, pos, dn_tgt, fc_enc_reg=fc_reg, fc_enc_cls=fc_cls)
    rec.update(hs_enc=hs_enc[0].detach(), ref_enc=ref_enc[0].detach(), init=init.detach())
    if f64 and "logits" in c:
        loss = (hs_enc[0] * torch.from_numpy(grad_pattern(hs_enc[0].shape, 1)).to(dt)).sum() + \
               (ref_enc[0] * torch.from_numpy(grad_pattern(ref_enc[0].shape, 2)).to(dt)).sum()
        loss.backward()
        rec["g_memory"], rec["g_reg"] = memory.grad, leaves["reg"].grad
    return {k_: v.numpy() for k_, v in rec.items()}


def main():
    out = {}
    for name, c in cases().items():
        r32, r64 = run(c, False), run(c, True)
        for k, v in c.items():
            out[f"{name}.{k}"] = v
        for k in ("prop", "topi", "dec_tgt", "dec_ref", "hs_enc", "ref_enc", "init"):
            out[f"{name}.{k}32"], out[f"{name}.{k}64"] = r32[k], r64[k]
        out[f"{name}.outmem32"], out[f"{name}.topv32"] = r32["outmem"], r32["topv"]
        assert r32["prop"].dtype == np.float32 and r64["prop"].dtype == np.float64
        for k in ("g_memory", "g_reg"):
            if k in r64:
                out[f"{name}.{k}"] = r64[k]
    np.savez_compressed(OUT, **out)
    print(f"wrote {OUT}: {len(out)} arrays, {os.path.getsize(OUT)} bytes")


if __name__ == "__main__":
    main()
