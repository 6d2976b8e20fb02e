#!/usr/bin/env python
"""Generate tests/golden/detect.npz from the REFERENCE's own ``get_bboxes`` / ``_get_bboxes_single`` of both heads
(detr_od/models/dense_heads/dino_detr_ssod_head.py:1281-1413, dino_detr_head.py:1048-1152), ``bbox_cxcywh_to_xyxy`` and
``bbox2result`` (thirdparty/mmdetection/mmdet/core/bbox/transforms.py:100-117, 222-233).  The sources are taken from the files
with ``ast`` at run time and executed (the ``def`` without its ``force_fp32`` decorator: the inputs are fp32 / fp64 already) --
the modules themselves import mmcv.  Runs on the CPU where the reference tree exists;
what it writes is data.

    python tools/gen_detect_golden.py

The functions run unbound on a stand-in ``self`` (``test_cfg``, ``num_query``, ``num_classes``, a sigmoid ``loss_cls`` /
``loss_cls2``, ``in_warm_up = False``); ``Tensor.topk`` is wrapped for the duration so that the indices are recorded.  Both
heads must agree bit for bit.  Every case runs in float32 (``*32``: decisions and the fp32 values) and in float64 (``*64``:
values).  Inputs come from ``det_ref64.seeded_inputs(seed, kind, L, B, Q, C, k)``; the small cases store them as well, the
large ones store the seed and a checksum only.

Per case ``<case>.``: ``seed``, ``kind``, ``dims`` (L, B, Q, C, k), ``rescale``, ``img_shape`` (B, 3), ``scale_factor`` (B, 4)
float32, ``checksum``, ``tie`` (1: the reference's order is open, see below), ``cls`` / ``box`` (small cases); recorded:
``idx32`` (B, k) the reference's flat top-k indices, ``dets32`` (B, k, 5), ``labels32`` (B, k), and, where ``tie`` is 0,
``dets64`` and bbox2result of the float32 run as ``grouped32`` (B, k, 5) rows in class order + ``offsets32`` (B, C + 1).

In every case with ``tie`` 0 this script asserts that the reference's k + 1 best fp32 scores of every image are pairwise
distinct (k best when k = Q * C) -- so its selection and order are decided, and comparing against it exactly leaves out no
element -- and that the float64 run selected the same indices.
"""
import ast
import os
import sys
import textwrap
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle.gen_golden import REF  # noqa: E402
sys.path.insert(0, os.path.join(ROOT, "tests"))
import det_ref64 as R  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "detect.npz")
HEADS = {"DINODETRSSODHead": REF + "/detr_od/models/dense_heads/dino_detr_ssod_head.py",
         "DINODETRHead": REF + "/detr_od/models/dense_heads/dino_detr_head.py"}
TRANSFORMS = REF + "/thirdparty/mmdetection/mmdet/core/bbox/transforms.py"


def _source(path, name, cls=None):
    src = open(path).read()
    tree = ast.parse(src)
    scope = tree
    if cls is not None:
        scope = next(n for n in ast.walk(tree) if isinstance(n, ast.ClassDef) and n.name == cls)
    for node in scope.body:
        if isinstance(node, ast.FunctionDef) and node.name == name:
            return textwrap.dedent(ast.get_source_segment(src, node, padded=True))
    raise KeyError(name)


def load_reference():
    """{head name: (get_bboxes, _get_bboxes_single)}, bbox2result"""
    ns = {"torch": torch, "np": np}
    exec(_source(TRANSFORMS, "bbox_cxcywh_to_xyxy"), ns)
    exec(_source(TRANSFORMS, "bbox2result"), ns)
    heads = {}
    for cls, path in HEADS.items():
        hns = dict(ns, F=torch.nn.functional, multiclass_nms=None)
        for fn in ("get_bboxes", "_get_bboxes_single"):
            exec(_source(path, fn, cls), hns)
        heads[cls] = (hns["get_bboxes"], hns["_get_bboxes_single"])
    return heads, ns["bbox2result"]


def run_head(head, fns, cls, box, metas, rescale, k):
    get_bboxes, single = fns
    use = types.SimpleNamespace(use_sigmoid=True)
    self = types.SimpleNamespace(test_cfg=dict(max_per_img=k), num_query=cls.shape[2], num_classes=cls.shape[3], loss_cls=use,
                                 loss_cls2=use, in_warm_up=False)
    self._get_bboxes_single = types.MethodType(single, self)
    recorded = []
    topk = torch.Tensor.topk

    def recording(t, *a, **kw):
        v, i = topk(t, *a, **kw)
        recorded.append(i.clone())
        return v, i
    torch.Tensor.topk = recording
    try:
        result = get_bboxes(self, cls, box, None, None, None, None, metas, rescale=rescale)
    finally:
        torch.Tensor.topk = topk
    return torch.stack([r[0] for r in result]), torch.stack([r[1] for r in result]), torch.stack(recorded)


CASES = [
    # name, kind, L, B, Q, C, k, rescale, img shapes, scale factors
    ("q5_all", "plain", 2, 1, 5, 3, 15, True, [(48, 64, 3)], [(1.25, 0.75, 1.25, 0.75)]),
    ("q5_one", "plain", 2, 1, 5, 3, 1, False, [(48, 64, 3)], [(1.25, 0.75, 1.25, 0.75)]),
    ("q37", "plain", 2, 2, 37, 20, 100, True, [(480, 640, 3), (333, 500, 3)], [(0.8, 0.8125, 0.8, 0.8125), (1.6, 1.5, 1.6, 1.5)]),
    ("q37_noscale", "plain", 2, 2, 37, 20, 100, False, [(480, 640, 3), (333, 500, 3)], [(0.8, 0.8125, 0.8, 0.8125), (1.6, 1.5, 1.6, 1.5)]),
    ("full_k300", "plain", 2, 2, 900, 80, 300, True, [(800, 1199, 3), (1333, 750, 3)],
     [(1.873438, 1.873536, 1.873438, 1.873536), (1.5625, 1.5621094, 1.5625, 1.5621094)]),
    ("full_k900", "plain", 2, 1, 900, 80, 900, False, [(800, 1333, 3)], [(2.0828125, 2.0833333, 2.0828125, 2.0833333)]),
    ("tie_dup_chunks", "dup_chunks", 1, 1, 900, 80, 300, False, [(800, 1333, 3)], [(1, 1, 1, 1)]),
    ("tie_quantized", "quantized", 1, 2, 900, 80, 300, True, [(800, 1199, 3), (1333, 750, 3)],
     [(1.873438, 1.873536, 1.873438, 1.873536), (1.5625, 1.5621094, 1.5625, 1.5621094)]),
    ("tie_all_equal", "all_equal", 1, 1, 37, 20, 100, False, [(480, 640, 3)], [(1, 1, 1, 1)]),
    ("tie_saturated", "saturated", 1, 1, 37, 20, 100, False, [(480, 640, 3)], [(1, 1, 1, 1)]),
    ("tie_inf_nan", "inf_nan", 1, 2, 37, 20, 100, False, [(480, 640, 3), (333, 500, 3)], [(1, 1, 1, 1), (1, 1, 1, 1)]),
    ("tie_zeros", "zeros", 1, 1, 37, 20, 20, False, [(480, 640, 3)], [(1, 1, 1, 1)]),
]
SMALL = 37 * 20 * 2 * 2          # cases up to this many logits store their inputs


def main():
    heads, bbox2result = load_reference()
    out = {}
    for i, (name, kind, L, B, Q, C, k, rescale, shapes, scales) in enumerate(CASES):
        seed = 20250100 + i
        cls, box = R.seeded_inputs(seed, kind, L, B, Q, C, k)
        sf = np.asarray(scales, np.float32)
        metas = [dict(img_shape=shapes[b], scale_factor=sf[b]) for b in range(B)]
        tie = kind in R.TIE_KINDS
        runs = {}
        for dt in (torch.float32, torch.float64):
            per_head = [run_head(h, fns, torch.from_numpy(cls).to(dt), torch.from_numpy(box).to(dt), metas, rescale, k)
                        for h, fns in heads.items()]
            for other in per_head[1:]:
                assert all(np.array_equal(a.numpy(), b.numpy(), equal_nan=a.dtype.is_floating_point)
                           for a, b in zip(per_head[0], other)), name
            runs[dt] = [t.numpy() for t in per_head[0]]
        dets32, labels32, idx32 = runs[torch.float32]
        dets64, _, idx64 = runs[torch.float64]
        assert dets32.dtype == np.float32 and dets64.dtype == np.float64 and dets32.shape == (B, k, 5)
        assert np.array_equal(labels32, idx32 % C)
        if not tie:
            scores = torch.from_numpy(cls[-1]).sigmoid().reshape(B, -1)
            best = scores.topk(min(k + 1, Q * C), dim=1)[0].numpy()
            assert (np.diff(best, axis=1) < 0).all(), f"{name}: the reference's k + 1 best fp32 scores are not distinct"
            assert np.array_equal(best[:, :k], dets32[..., 4]) and np.array_equal(idx32, idx64), name
        c = dict(seed=np.int64(seed), kind=np.asarray(kind), dims=np.asarray([L, B, Q, C, k], np.int64), rescale=np.int64(rescale),
                 img_shape=np.asarray(shapes, np.int64), scale_factor=sf, checksum=R.checksum(cls, box), tie=np.int64(tie),
                 idx32=idx32.astype(np.int32), dets32=dets32, labels32=labels32.astype(np.int32))
        if cls.size <= SMALL:
            c.update(cls=cls, box=box)
        if not tie:
            c["dets64"] = dets64
            grouped, offsets = [], []
            for b in range(B):
                per_class = bbox2result(torch.from_numpy(dets32[b]), torch.from_numpy(labels32[b]), C)
                assert len(per_class) == C and all(a.dtype == np.float32 for a in per_class)
                grouped.append(np.concatenate(per_class))
                offsets.append(np.concatenate([[0], np.cumsum([len(a) for a in per_class])]))
            c.update(grouped32=np.stack(grouped), offsets32=np.asarray(offsets, np.int32))
        for key, v in c.items():
            out[f"{name}.{key}"] = v
    np.savez_compressed(OUT, **out)
    print(f"wrote {OUT}: {len(out)} arrays, {os.path.getsize(OUT)} bytes")


if __name__ == "__main__":
    main()
