#!/usr/bin/env python
"""Generate tests/golden/pyramid_inputs.npz from the REFERENCE's own ``SinePositionalEncodingHW.forward``
(detr_od/models/utils/positional_encoding.py:57-99), ``DINOTransformer.get_valid_ratio`` (transformer.py:1237-1244),
``DINOTransformerEncoder.get_reference_points`` (:676-691) and the flatten loop at the top of ``DINOTransformer.forward``
(:1267-1292), and the head's mask construction (dino_detr_ssod_head.py:351-363, restated: it is three lines of torch).  The
sources are taken from the files with ``ast`` at run time and executed -- the modules themselves import mmcv.  Runs on the CPU
where the reference tree exists; what it writes is data.

    python tools/gen_pyramid_inputs_golden.py

Cases: ``FIXTURE_CASES`` of tests/pyramid_inputs_cases.py's cases (fp32 ``pos``).  To keep the file small ``pos`` and the
reference points are stored at ``ROWS`` token rows per case (the first and last row of every level and evenly spaced rows in
between); masks, valid ratios, index tensors and the ``level_embed`` gradient (from ``(pos * g).sum().backward()``) are whole.

Per case ``<case>.``: ``rows`` (the stored row indices), ``pos`` (N, rows, 256), ``reference_points`` (N, rows, L, 2),
``mask_flatten`` (N, S) uint8, ``valid_ratios``, ``spatial_shapes``, ``level_start_index``, ``grad`` (L, 256; absent without a
level row), ``dim_ty`` / ``dim_tx`` (the fp32 tables the reference's expression gives on the CPU).
"""
import ast
import os
import sys
import textwrap
import types

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle.gen_golden import REF  # noqa: E402
sys.path.insert(0, os.path.join(ROOT, "tests"))
import pyramid_inputs_cases as C  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "pyramid_inputs.npz")
ENC_SRC = REF + "/detr_od/models/utils/positional_encoding.py"
TR_SRC = REF + "/detr_od/models/utils/transformer.py"
FIXTURE_CASES = ("padded_batch", "exact_product", "real_divisor", "masks_row_col", "masks_one_full", "offset_temps", "no_normalize",
                 "one_level")
ROWS = 16


def _function(path, name, cls):
    src = open(path).read()
    scope = next(n for n in ast.walk(ast.parse(src)) if isinstance(n, ast.ClassDef) and n.name == cls)
    node = next(n for n in scope.body if isinstance(n, ast.FunctionDef) and n.name == name)
    return src, node


def _source(path, name, cls):
    src, node = _function(path, name, cls)
    return textwrap.dedent(ast.get_source_segment(src, node, padded=True))


def _flatten_loop():
    """The statements of ``DINOTransformer.forward`` from ``src_flatten = []`` to ``valid_ratios = ...`` as a function."""
    src, node = _function(TR_SRC, "forward", "DINOTransformer")

    def assigns(stmt, name):
        return isinstance(stmt, ast.Assign) and any(isinstance(t, ast.Name) and t.id == name for t in stmt.targets)
    first = next(i for i, s in enumerate(node.body) if assigns(s, "src_flatten"))
    last = next(i for i, s in enumerate(node.body) if assigns(s, "valid_ratios"))
    body = "\n".join(textwrap.dedent(ast.get_source_segment(src, s, padded=True)) for s in node.body[first:last + 1])
    return ("def prepare(self, srcs, masks, pos_embeds):\n" + textwrap.indent(body, "    ") +
            "\n    return lvl_pos_embed_flatten, mask_flatten, spatial_shapes, level_start_index, valid_ratios\n")


def load_reference():
    ns = {"torch": torch}
    exec(_source(ENC_SRC, "forward", "SinePositionalEncodingHW"), ns)
    encode = ns["forward"]
    exec(_source(TR_SRC, "get_valid_ratio", "DINOTransformer"), ns)
    exec(_source(TR_SRC, "get_reference_points", "DINOTransformerEncoder"), ns)
    exec(_flatten_loop(), ns)
    return encode, ns["get_valid_ratio"], ns["get_reference_points"], ns["prepare"]


def stored_rows(shapes):
    rows, at = set(), 0
    for h, w in shapes:
        rows |= {at, at + h * w - 1}
        at += h * w
    rows |= set(int(r) for r in np.linspace(0, at - 1, ROWS))
    return np.array(sorted(rows), np.int64)


def run(case, encode, get_valid_ratio, get_reference_points, prepare):
    enc = types.SimpleNamespace(**dict(dict(scale=2 * np.pi, eps=1e-6, offset=0.), **case["enc"]))
    if case["masks"] is not None:
        masks = [torch.from_numpy(np.asarray(m)) for m in case["masks"]]
    else:                                                       # the head's lines, on the CPU
        n = len(case["img_shapes"])
        img_masks = torch.ones((n,) + tuple(case["input"]))
        for img_id, (img_h, img_w) in enumerate(case["img_shapes"]):
            img_masks[img_id, :img_h, :img_w] = 0
        masks = [F.interpolate(img_masks[None], size=s).to(torch.bool).squeeze(0) for s in case["shapes"]]
    level_embed = None if case["level_embed"] is None else torch.from_numpy(case["level_embed"]).requires_grad_(True)
    pos_embeds = [encode(enc, m) for m in masks]
    srcs = [torch.zeros(p.shape) for p in pos_embeds]
    self = types.SimpleNamespace(num_feature_levels=len(masks), level_embed=level_embed,
                                 get_valid_ratio=lambda m: get_valid_ratio(None, m))
    pos, mask_flatten, spatial_shapes, level_start_index, valid_ratios = prepare(self, srcs, masks, pos_embeds)
    ref = get_reference_points(spatial_shapes, valid_ratios, device="cpu")
    rows = stored_rows(case["shapes"])
    k = torch.arange(C.NUM_FEATS, dtype=torch.float32)
    out = dict(rows=rows, pos=pos.detach().numpy()[:, rows], reference_points=ref.numpy()[:, rows],
               mask_flatten=mask_flatten.numpy().astype(np.uint8), valid_ratios=valid_ratios.numpy(),
               spatial_shapes=spatial_shapes.numpy(), level_start_index=level_start_index.numpy(),
               dim_ty=(enc.temperatureH ** (2 * (k // 2) / C.NUM_FEATS)).numpy(),
               dim_tx=(enc.temperatureW ** (2 * (k // 2) / C.NUM_FEATS)).numpy())
    if level_embed is not None:
        (pos * torch.from_numpy(case["g"])).sum().backward()
        out["grad"] = level_embed.grad.numpy()
    assert out["pos"].dtype == np.float32 and out["reference_points"].dtype == np.float32
    return out


def main():
    fns = load_reference()
    out = {}
    for name in FIXTURE_CASES:
        for k, v in run(C.cases()[name], *fns).items():
            out[f"{name}.{k}"] = v
    np.savez_compressed(OUT, **out)
    print(f"wrote {OUT}: {len(out)} arrays, {os.path.getsize(OUT)} bytes")


if __name__ == "__main__":
    main()
