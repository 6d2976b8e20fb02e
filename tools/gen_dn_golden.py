#!/usr/bin/env python
"""Generate tests/golden/dn_query.npz from the REFERENCE's own ``prepare_for_cdn`` / ``prepare_for_cdn_plus``
(detr_od/models/dense_heads/dn_components.py, executed as a module) and ``DinoDetrSSOD.prepare_unsup_cdn``
(detr_ssod/models/dino_detr_ssod.py:484-760, the method's source executed unbound on a stand-in ``self``), with mmdet's
``inverse_sigmoid`` and ``bbox_xyxy_to_cxcywh`` taken from their files.  Runs on the CPU where the reference tree exists;
what it writes is data.

    python tools/gen_dn_golden.py

Everything runs in float64 (default dtype float64, ``Tensor.cuda`` / ``.to('cuda')`` identities).  The module's
``torch.rand_like`` / ``randint_like`` / ``randint`` are answered from ONE uniform tensor ``u`` by the layout documented in
``semi_detr_amd/dn_query.py``: ``rand_like`` of a vector is ``u[:, 0]``, of a (K, 4) matrix ``u[:, 6:10]``; ``randint_like``
with a dtype is ``u[:, 2:6] >= 0.5`` (the reference maps it to +-1), without one ``new_label[chosen_indice]`` with
``new_label = min(int(u[:, 1] * num_classes), num_classes - 1)`` in fp32; ``randint(0, 80, (1,))`` is ``int(u_img[b] * 80)``
of the next empty image.  ``u``, the embedding weight, the boxes and the projector rows are drawn in float32 and up-cast, so
every threshold decision is exact.

Per case ``<case>.``: ``kind`` (0 cdn, 1 plus, 2 unsup), ``counts``, ``labels``, ``boxes``, ``weight``, ``u`` (flat: K * 10,
then one value per image for kinds 1 and 2), ``params`` (dn_number, label_noise_ratio, box_noise_scale, num_queries,
num_classes, hidden_dim), the outputs (``query_label`` float32 -- they are copies --, ``query_bbox`` float64, ``mask``
packed with np.packbits + ``tgt``, ``meta`` = pad_size, num_dn_group, ``pad_mask``) and the float64 gradient ``grad_weight`` of
``sum(query_label * g_label)`` with ``g_label = dn_ref64.grad_pattern(shape, 1)`` (not stored).  Kind 2 adds the pseudo / detected boxes, the image shapes, the recorded
``rois`` the extractor received and ``proj`` rows the projector returned, ``step`` (curr_step, warm_up_step, prior), the
consistency outputs (``label_1``, ``bbox_1``, ``known_bid_1/2``, ``map_1/2``, ``loss_weights``) and ``grad_proj``
(the gradient of ``sum(label_1 * grad_pattern(shape, 2))`` w.r.t. the projector rows).
"""
import ast
import io
import os
import sys
import textwrap
import types
import zipfile

import numpy as np
import torch
from torch import nn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle.gen_golden import REF  # noqa: E402
sys.path.insert(0, os.path.join(ROOT, "tests"))
from dn_ref64 import grad_pattern  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "dn_query.npz")
F32 = np.float32


def _function_source(path, name):
    src = open(path).read()
    for node in ast.walk(ast.parse(src)):
        if isinstance(node, ast.FunctionDef) and node.name == name:
            return textwrap.dedent(ast.get_source_segment(src, node, padded=True))
    raise KeyError(name)


class Noise:
    """Answers the reference's random calls from ``u``."""

    def __init__(self):
        self.u = self.u_img = None
        self.empty, self.num_classes = [], 80

    def arm(self, u, u_img, empty, num_classes):
        self.u, self.u_img, self.empty, self.num_classes = u, u_img, list(empty), num_classes

    def rand_like(self, t, **kw):
        u = torch.from_numpy(self.u.astype(np.float64))
        out = u[:, 0] if t.dim() == 1 else u[:, 6:10]
        assert out.shape == t.shape, (out.shape, t.shape)
        return out.clone()

    def randint_like(self, t, *a, **kw):
        if "dtype" in kw:
            return torch.from_numpy((self.u[:, 2:6] >= F32(0.5)).astype(np.float64))
        nl = np.minimum((self.u[:, 1] * F32(self.num_classes)).astype(F32).astype(np.int64), self.num_classes - 1)
        return torch.from_numpy(nl)[t]

    def randint(self, lo, hi, size, **kw):
        assert (lo, hi, tuple(size)) == (0, 80, (1,))
        b = self.empty.pop(0)
        return torch.tensor([int((self.u_img[b] * F32(80)).astype(F32))])


class TorchProxy:
    def __init__(self, noise):
        self._n = noise

    def __getattr__(self, k):
        if k in ("rand_like", "randint_like", "randint"):
            return getattr(self._n, k)
        return getattr(torch, k)


def load_reference(noise):
    torch.set_default_dtype(torch.float64)
    torch.Tensor.cuda = lambda self, *a, **k: self
    _to = torch.Tensor.to
    torch.Tensor.to = lambda self, *a, **k: self if a and a[0] == "cuda" else _to(self, *a, **k)
    mmd = REF + "/thirdparty/mmdetection/mmdet"
    ns = {"torch": torch}
    exec(_function_source(mmd + "/models/utils/transformer.py", "inverse_sigmoid"), ns)
    exec(_function_source(mmd + "/core/bbox/transforms.py", "bbox_xyxy_to_cxcywh"), ns)
    for name in ("mmdet", "mmdet.models", "mmdet.models.utils"):
        sys.modules.setdefault(name, types.ModuleType(name))
    tr = types.ModuleType("mmdet.models.utils.transformer")
    tr.inverse_sigmoid = ns["inverse_sigmoid"]
    sys.modules["mmdet.models.utils.transformer"] = tr
    proxy = TorchProxy(noise)
    comp = types.ModuleType("ref_dn_components")
    exec(compile(open(REF + "/detr_od/models/dense_heads/dn_components.py").read(), "dn_components.py", "exec"), comp.__dict__)
    comp.torch = proxy
    uns = {"torch": proxy, "inverse_sigmoid": ns["inverse_sigmoid"], "bbox_xyxy_to_cxcywh": ns["bbox_xyxy_to_cxcywh"]}
    exec(_function_source(REF + "/detr_ssod/models/dino_detr_ssod.py", "prepare_unsup_cdn"), uns)
    return comp.prepare_for_cdn, comp.prepare_for_cdn_plus, uns["prepare_unsup_cdn"]


def groups_of(dn_number, max_count):          # dn_components.py:21-35
    n = dn_number * 2
    if max_count == 0:
        n = 1
    elif n >= 100:
        n = n // (max_count * 2)
    elif n < 1:
        n = 1
    return n or 1


def rand_boxes(rng, n, edges=False):
    """normalised cxcywh; ``edges``: boxes that touch 0 / 1, a zero-size box, a full-image box"""
    c = rng.random((n, 2)) * 0.6 + 0.2
    wh = rng.random((n, 2)) * 0.3 + 0.02
    b = np.concatenate([c, wh], 1).astype(F32)
    if edges and n >= 4:
        b[0] = [0.1, 0.2, 0.2, 0.4]            # x1 = y1 = 0 exactly
        b[1] = [0.9, 0.75, 0.2, 0.5]           # x2 = y2 = 1 (to rounding)
        b[2] = [0.5, 0.5, 0.0, 0.0]            # zero size: the eps clamp
        b[3] = [0.5, 0.5, 1.0, 1.0]            # the whole image
        if n >= 5:
            b[4] = [1.0, 0.0, 0.05, 0.05]      # centre on the corner
    return b


def pack(d, pre, name, v):
    d[pre + name] = np.asarray(v)


def run_cdn(fn, noise, rng, d, case, kind, counts, dn_number=100, ratio=0.5, scale=1.0, nq=30, nc=80, H=32, edges=False):
    pre = case + "."
    eff = [max(c, 1) for c in counts] if kind else list(counts)
    groups = groups_of(dn_number, max(eff))
    K = 2 * groups * sum(eff)
    u = rng.random((K, 10), dtype=F32)
    u_img = rng.random(len(counts), dtype=F32)
    weight = rng.standard_normal((nc + 1, H)).astype(F32)
    labels = [rng.integers(0, nc, c).astype(np.int64) for c in counts]
    boxes = [rand_boxes(rng, c, edges) for c in counts]
    noise.arm(u, u_img, [b for b, c in enumerate(counts) if c == 0], nc)
    enc = nn.Embedding(nc + 1, H)
    enc.weight.data = torch.from_numpy(weight.astype(np.float64))
    targets = {"labels": [torch.from_numpy(x) for x in labels],
               "boxes": [torch.from_numpy(x.astype(np.float64)) for x in boxes]}
    ql, qb, mask, meta = fn((targets, dn_number, ratio, scale), True, nq, nc, H, enc)
    g = grad_pattern(tuple(ql.shape), 1)
    gw = np.zeros((nc + 1, H))
    if ql.numel():
        (ql * torch.from_numpy(g.astype(np.float64))).sum().backward()
        gw = enc.weight.grad.numpy()
    assert meta["num_dn_group"] == groups and (ql.shape[1] == 0 or ql.shape[1] == 2 * groups * max(eff))
    pack(d, pre, "kind", kind)
    pack(d, pre, "counts", np.asarray(counts, np.int64))
    pack(d, pre, "labels", np.concatenate(labels) if labels else np.zeros(0, np.int64))
    pack(d, pre, "boxes", np.concatenate(boxes).reshape(-1, 4))
    pack(d, pre, "weight", weight)
    pack(d, pre, "u", np.concatenate([u.reshape(-1), u_img]) if kind else u.reshape(-1))
    pack(d, pre, "params", np.asarray([dn_number, ratio, scale, nq, nc, H], np.float64))
    ql_np = ql.detach().numpy()
    assert np.array_equal(ql_np.astype(F32).astype(np.float64), ql_np)
    pack(d, pre, "query_label", ql_np.astype(F32))
    pack(d, pre, "query_bbox", qb.detach().numpy().astype(np.float64))
    pack(d, pre, "mask", np.packbits(mask.numpy()))
    pack(d, pre, "tgt", mask.shape[0])
    pack(d, pre, "meta", np.asarray([meta["pad_size"], meta["num_dn_group"]], np.int64))
    if kind:
        pack(d, pre, "pad_mask", meta["pad_mask"].numpy().astype(np.int64))
    pack(d, pre, "grad_weight", gw)


class _Obj:
    pass


def run_unsup(fn, noise, rng, d, case, counts, shapes_tgt, shapes_src, curr_step, warm_up_step, prior, dn_number=100,
              ratio=0.5, scale=1.0, nq=30, nc=80, H=32):
    """``counts``: pseudo boxes per image (= detected boxes = the dn targets of the call site, dino_detr_ssod.py:372-394)."""
    pre = case + "."
    B = len(counts)
    eff = [max(c, 1) for c in counts]
    groups = groups_of(dn_number, max(eff))
    K2, K1 = 2 * groups * sum(eff), 5 * sum(eff)
    u = rng.random((K2, 10), dtype=F32)
    u_img = rng.random(B, dtype=F32)
    weight = rng.standard_normal((nc + 1, H)).astype(F32)
    proj = rng.standard_normal((K1, H)).astype(F32)

    def pix(n, hw, cols):
        h, w = hw[0], hw[1]
        xy = rng.random((n, 2)) * [w * 0.6, h * 0.6]
        box = np.concatenate([xy, xy + rng.random((n, 2)) * [w * 0.5, h * 0.5] + 2, rng.random((n, 1))], 1).astype(F32)
        if n:
            box[0, :4] = [0, 0, w, h + 3]                       # touches every border, one side beyond it
        return box[:, :cols]
    pseudo = [pix(c, s, 4) for c, s in zip(counts, shapes_tgt)]
    det = [pix(c, s, 5) for c, s in zip(counts, shapes_src)]
    labels = [rng.integers(0, nc, c).astype(np.int64) for c in counts]
    norm = []
    for p, s in zip(pseudo, shapes_tgt):                        # the call site's normalisation, :376-383, in fp32
        f = np.asarray([s[1], s[0], s[1], s[0]], F32)
        cxcywh = np.concatenate([(p[:, :2] + p[:, 2:]) / F32(2), p[:, 2:] - p[:, :2]], 1).astype(F32)
        norm.append((cxcywh / f).astype(F32).reshape(-1, 4))
    noise.arm(u, u_img, [b for b, c in enumerate(counts) if c == 0], nc)
    rec = {}
    self = _Obj()
    self.curr_step = curr_step
    self.teacher, self.student = _Obj(), _Obj()
    self.student.bbox_head = _Obj()
    self.student.bbox_head.warm_up_step = warm_up_step
    enc = nn.Embedding(nc + 1, H)
    enc.weight.data = torch.from_numpy(weight.astype(np.float64))
    self.student.bbox_head.label_enc = enc
    self.teacher.extract_feat = lambda img: "feats"
    self.prepare_feats = lambda feats, metas: (feats, None, None)
    proj_t = torch.from_numpy(proj.astype(np.float64)).requires_grad_(True)

    def extractor(feats, rois):
        rec["rois"] = rois.detach().numpy().copy()
        return "roi_feats"
    self.roi_extractor = extractor
    self.projector = lambda x: proj_t * 1.0
    img = torch.zeros(B, 3, 4, 4)
    tinfo = {"img": img, "img_metas": [{"img_shape": s} for s in shapes_src]}
    sinfo = {"img": img, "img_metas": [{"img_shape": s} for s in shapes_tgt]}
    targets = {"labels": [torch.from_numpy(x) for x in labels], "boxes": [torch.from_numpy(x.astype(np.float64)) for x in norm]}
    prior_info = None
    if prior:
        prior_info = {"loss_weights": torch.from_numpy(rng.integers(0, 2, (K1, 1)).astype(np.float64)),
                      "input_query_label_1": torch.from_numpy(rng.standard_normal((B, 5 * max(eff), H)).astype(F32).astype(np.float64))}
    l1, b1, l2, b2, mask, meta = fn(self, tinfo, sinfo, [torch.from_numpy(x.astype(np.float64)) for x in pseudo], labels,
                                    [torch.from_numpy(x.astype(np.float64)) for x in det], labels,
                                    dn_args=(targets, dn_number, ratio, scale), hidden_dim=H, num_queries=nq, num_classes=nc,
                                    prior_info=prior_info)
    g2 = grad_pattern(tuple(l2.shape), 1)
    g1 = grad_pattern(tuple(l1.shape), 2)
    loss = (l2 * torch.from_numpy(g2.astype(np.float64))).sum()
    if not prior:
        loss = loss + (l1 * torch.from_numpy(g1.astype(np.float64))).sum()
    loss.backward()
    pack(d, pre, "kind", 2)
    pack(d, pre, "counts", np.asarray(counts, np.int64))
    pack(d, pre, "labels", np.concatenate(labels))
    pack(d, pre, "boxes", np.concatenate(norm).reshape(-1, 4))
    pack(d, pre, "pseudo", np.concatenate(pseudo).reshape(-1, 4))
    pack(d, pre, "det", np.concatenate(det).reshape(-1, 5))
    pack(d, pre, "shapes_tgt", np.asarray(shapes_tgt, np.int64))
    pack(d, pre, "shapes_src", np.asarray(shapes_src, np.int64))
    pack(d, pre, "weight", weight)
    pack(d, pre, "proj", proj)
    pack(d, pre, "u", np.concatenate([u.reshape(-1), u_img]))
    pack(d, pre, "params", np.asarray([dn_number, ratio, scale, nq, nc, H], np.float64))
    pack(d, pre, "step", np.asarray([curr_step, warm_up_step, int(prior)], np.int64))
    if prior:
        pack(d, pre, "prior_loss_weights", prior_info["loss_weights"].numpy().astype(F32))
    else:
        pack(d, pre, "rois", rec["rois"].astype(np.float64))
        pack(d, pre, "grad_proj", proj_t.grad.numpy())
    pack(d, pre, "label_1", l1.detach().numpy().astype(F32))
    pack(d, pre, "bbox_1", b1.numpy().astype(np.float64))
    pack(d, pre, "query_label", l2.detach().numpy().astype(F32))
    pack(d, pre, "query_bbox", b2.detach().numpy().astype(np.float64))
    pack(d, pre, "mask", np.packbits(mask.numpy()))
    pack(d, pre, "tgt", mask.shape[0])
    pack(d, pre, "meta", np.asarray([meta["pad_size_1"], meta["pad_size_2"], meta["num_dn_group_1"], meta["num_dn_group_2"]],
                                    np.int64))
    pack(d, pre, "known_bid_1", meta["known_bid_1"].numpy().astype(np.float64))
    pack(d, pre, "known_bid_2", meta["known_bid_2"].numpy().astype(np.int64))
    pack(d, pre, "map_1", meta["map_known_indice_1"].numpy().astype(np.int64))
    pack(d, pre, "map_2", meta["map_known_indice_2"].numpy().astype(np.int64))
    pack(d, pre, "loss_weights", meta["loss_weights"].numpy().astype(F32))
    pack(d, pre, "grad_weight", enc.weight.grad.numpy())


def write_npz(path, d):
    """np.savez_compressed with fixed member timestamps, so that a rerun reproduces the file byte for byte."""
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as z:
        for k in sorted(d):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asanyarray(d[k]), allow_pickle=False)
            z.writestr(zipfile.ZipInfo(k + ".npy", date_time=(1980, 1, 1, 0, 0, 0)), buf.getvalue(), zipfile.ZIP_DEFLATED)


def main():
    noise = Noise()
    cdn, plus, unsup = load_reference(noise)
    rng = np.random.default_rng(20261016)
    d = {}
    run_cdn(cdn, noise, rng, d, "cdn_mixed", 0, [3, 0, 7, 1], nq=900)
    run_cdn(cdn, noise, rng, d, "cdn_big", 0, [120, 2], nq=40)
    run_cdn(cdn, noise, rng, d, "cdn_empty", 0, [0, 0], nq=20)
    run_cdn(cdn, noise, rng, d, "cdn_one", 0, [1], nq=20)
    run_cdn(cdn, noise, rng, d, "cdn_no_label_noise", 0, [4, 2], ratio=0.0)
    run_cdn(cdn, noise, rng, d, "cdn_no_box_noise", 0, [5, 2], scale=0.0, edges=True)
    run_cdn(cdn, noise, rng, d, "cdn_edges", 0, [6, 5, 50], edges=True)
    run_cdn(cdn, noise, rng, d, "cdn_h256", 0, [2, 1], dn_number=4, H=256)
    run_cdn(plus, noise, rng, d, "plus_mixed", 1, [3, 0, 7, 1], nq=900)
    run_cdn(plus, noise, rng, d, "plus_all_empty", 1, [0, 0, 0])
    run_cdn(plus, noise, rng, d, "plus_big", 1, [130, 0], nq=17)
    run_cdn(plus, noise, rng, d, "plus_edges", 1, [5, 0, 6], edges=True, nc=90)
    st, ss = [(800, 1199, 3), (640, 853, 3), (512, 512, 3)], [(750, 1000, 3), (600, 800, 3), (480, 640, 3)]
    run_unsup(unsup, noise, rng, d, "unsup_student", [2, 0, 3], st, ss, 10, 100, False)
    run_unsup(unsup, noise, rng, d, "unsup_teacher", [2, 0, 3], ss, ss, 10, 100, True)
    run_unsup(unsup, noise, rng, d, "unsup_student_late", [4, 1], st[:2], ss[:2], 100, 100, False, nq=900)
    run_unsup(unsup, noise, rng, d, "unsup_teacher_late", [0, 6], ss[:2], ss[:2], 500, 100, True)
    d["cases"] = np.asarray(sorted({k.split(".")[0] for k in d}))
    write_npz(OUT, d)
    print("wrote", OUT, os.path.getsize(OUT), "bytes,", len(d["cases"]), "cases")


if __name__ == "__main__":
    main()
