"""De-noising and consistency queries on the MI355X (``csrc/dn_query.hip``).

* ``prepare_for_cdn`` / ``prepare_for_cdn_plus`` replace the functions of the same name in
  detr_od/models/dense_heads/dn_components.py:6-125,128-274: same positional signature, same return tuple, same
  ``dn_meta`` keys, dtypes and shapes.
* ``prepare_unsup_cdn`` replaces ``DinoDetrSSOD.prepare_unsup_cdn`` (detr_ssod/models/dino_detr_ssod.py:484-760) and binds
  as that method: it still calls ``self.teacher.extract_feat``, ``self.prepare_feats``, ``self.roi_extractor`` and
  ``self.projector``.

Every size in these functions follows from the LENGTHS of the per-image lists, which are host values, so a call is one
``torch.rand`` draw plus one launch (two for ``prepare_unsup_cdn``) and reads nothing back.  The backward w.r.t. the label
embedding weight is a fixed-order sum without float atomics (bitwise reproducible), w.r.t. the projector output a gather.

Noise contract.  The reference draws four random tensors, one of a data-dependent shape.  Here ONE uniform tensor
``u`` of ``K * 10`` values in [0, 1) is drawn (``K = 2 * num_dn_group * sum of list lengths``), row ``k`` of ``u.view(K, 10)``
belonging to known row ``k``: column 0 = ``p`` (the label is replaced iff ``p < label_noise_ratio * 0.5``), column 1 ->
``new_label = min(int(u * num_classes), num_classes - 1)`` in fp32, columns 2..5 -> sign of x1, y1, x2, y2 (+1 iff
``u >= 0.5``), columns 6..9 = ``rand_part`` of x1, y1, x2, y2.  ``prepare_for_cdn_plus`` and ``prepare_unsup_cdn`` append one
value per image: the stand-in label of an image without boxes is ``int(u * 80)`` (80 as in the reference).  The same
distribution as the reference's, but a different use of the RNG stream: equal seeds give different noise.  ``noise=``
passes the tensor explicitly (any shape, ``K * 10 [+ B]`` values); ``generator=`` the generator of the draw.
"""
import ctypes

import torch

from . import _lib

MAX_IMAGES, NOISE_COLS = _lib.CONSTANTS["SEMIDETR_DN_MAX_IMAGES"], _lib.CONSTANTS["SEMIDETR_DN_NOISE_COLS"]
CONSISTENCY_GROUPS = 5                   # dn_number_1, dino_detr_ssod.py:533
_Layout, _Build, _Consistency = _lib.DnLayout, _lib.DnBuild, _lib.DnConsistency


def make_layout(counts, single_pad, groups):
    """``semidetr_dn_layout`` of per-image list lengths ``counts``."""
    if len(counts) > MAX_IMAGES:
        raise ValueError(f"dn_query: {len(counts)} images per call (at most {MAX_IMAGES})")
    lay = _Layout()
    lay.num_images, lay.single_pad, lay.groups = len(counts), int(single_pad), int(groups)
    at = 0
    for b, n in enumerate(counts):
        at += int(n)
        lay.offsets[b + 1] = at
    return lay


def dn_groups(dn_number, max_count):
    """``num_dn_group`` as the reference derives it (dn_components.py:21-35)."""
    n = dn_number * 2
    if max_count == 0:
        n = 1
    elif n >= 100:
        n = n // (max_count * 2)
    elif n < 1:
        n = 1
    return n if n != 0 else 1


def _require_cuda(t, what):
    if not t.is_cuda:
        raise RuntimeError(f"dn_query: {what} must live on the GPU (no CPU fallback)")


def _entry(t, dtype, dev):
    """A per-image list entry as a contiguous device tensor (a no-op for what the callers pass)."""
    t = t.detach()
    if t.device != dev or t.dtype != dtype:
        t = t.to(device=dev, dtype=dtype)
    return t.contiguous()


def _noise(noise, generator, numel, dev):
    if noise is None:
        return torch.rand(numel, dtype=torch.float32, device=dev, generator=generator)
    noise = noise.detach().reshape(-1)
    if noise.numel() != numel:
        raise ValueError(f"dn_query: noise has {noise.numel()} values, this call consumes {numel} (K * {NOISE_COLS} + one per "
                         f"image where empty images get a stand-in)")
    if noise.device != dev or noise.dtype != torch.float32:
        noise = noise.to(device=dev, dtype=torch.float32)
    return noise.contiguous()


class _DnBuildFn(torch.autograd.Function):
    """One ``semidetr_dn_build_f32`` launch.  Differentiable: ``query_label`` w.r.t. the embedding weight, ``cons_label``
    w.r.t. the projector rows."""

    @staticmethod
    def forward(ctx, weight, cons_rows, st):
        dev = weight.device
        B, pad2, pad1, H, K = st["B"], st["pad2"], st["pad1"], weight.shape[1], st["K"]
        w = weight.detach()
        w = w if w.dtype == torch.float32 else w.float()
        w = w.contiguous()
        p = st["params"]
        keep = [w]
        p.label_weight, p.num_embeddings, p.hidden_dim = w.data_ptr(), w.shape[0], H
        q_label = torch.empty((B, pad2, H), dtype=torch.float32, device=dev)
        q_bbox = torch.empty((B, pad2, 4), dtype=torch.float32, device=dev)
        ints = torch.empty((3, K), dtype=torch.int64, device=dev)          # known_bid, map_known_indice, noised labels
        tgt = pad1 + pad2 + st["num_queries"]
        mask = torch.empty((tgt, tgt), dtype=torch.bool, device=dev)
        pad_mask = torch.empty((B, pad2), dtype=torch.int64, device=dev) if st["want_pad_mask"] else None
        cons_label = None
        if cons_rows is not None:
            rows = cons_rows.detach()
            rows = (rows if rows.dtype == torch.float32 else rows.float()).contiguous()
            if rows.shape != (st["K1"], H):
                raise ValueError(f"dn_query: the projector returned {tuple(rows.shape)}, expected {(st['K1'], H)}")
            keep.append(rows)
            cons_label = torch.empty((B, pad1, H), dtype=torch.float32, device=dev)
            p.cons_rows, p.cons_label = rows.data_ptr(), cons_label.data_ptr()
        p.query_label, p.query_bbox = q_label.data_ptr(), q_bbox.data_ptr()
        p.known_bid, p.map_known_indice, p.noised_labels = ints[0].data_ptr(), ints[1].data_ptr(), ints[2].data_ptr()
        p.pad_mask = pad_mask.data_ptr() if pad_mask is not None else None
        p.attn_mask = mask.data_ptr()
        _lib.call("semidetr_dn_build_f32", dev, ctypes.byref(p))
        ctx.st = dict(B=B, pad2=pad2, H=H, K=K, E=w.shape[0], cons=st["cons"], w_dtype=weight.dtype,
                      rows_dtype=None if cons_rows is None else cons_rows.dtype)
        ctx.save_for_backward(ints)
        outs = (q_label, q_bbox, mask, ints[0], ints[1], ints[2], pad_mask, cons_label)
        ctx.mark_non_differentiable(*[o for o in outs[1:7] if o is not None])
        ctx.set_materialize_grads(False)
        return outs

    @staticmethod
    def backward(ctx, g_label, *rest):
        g_cons = rest[-1]
        (ints,) = ctx.saved_tensors
        st = ctx.st
        gw = grows = None
        if ctx.needs_input_grad[0] and g_label is not None:
            g = g_label.float().contiguous()
            gw = torch.empty((st["E"], st["H"]), dtype=torch.float32, device=g.device)
            _lib.call("semidetr_dn_label_backward_f32", ints.device, g, ints[0], ints[1], ints[2], st["K"], st["B"], st["pad2"],
                      st["H"], st["E"], gw)
            gw = gw.to(st["w_dtype"])
        if ctx.needs_input_grad[1] and g_cons is not None:
            g = g_cons.float().contiguous()
            cons = st["cons"]
            grows = torch.empty((cons.groups * cons.offsets[cons.num_images], st["H"]), dtype=torch.float32, device=g.device)
            _lib.call("semidetr_dn_gather_rows_f32", ints.device, ctypes.byref(cons), g, st["H"], grows)
            grows = grows.to(st["rows_dtype"])
        return gw, grows, None


def _label_weight(label_enc):
    weight = getattr(label_enc, "weight", None)
    if weight is None or weight.dim() != 2:
        raise TypeError("dn_query: label_enc must be an nn.Embedding (its weight is read directly)")
    _require_cuda(weight, "label_enc.weight")
    return weight


def _cdn(labels_list, boxes_list, standin, dn_number, label_noise_ratio, box_noise_scale, num_queries, num_classes,
         hidden_dim, weight, noise, generator, cons=None, cons_rows=None, want_pad_mask=False):
    """The contrastive de-noising part shared by the three functions (+ the scatter of ``cons_rows`` and the mask)."""
    dev = weight.device
    if weight.shape[1] != hidden_dim:
        raise ValueError(f"dn_query: hidden_dim {hidden_dim} but label_enc has {weight.shape[1]} channels")
    src = [int(t.shape[0]) for t in labels_list]
    if [int(t.shape[0]) for t in boxes_list] != src:
        raise ValueError("dn_query: targets['labels'] and targets['boxes'] disagree on the list lengths")
    B = len(src)
    counts = [max(n, 1) for n in src] if standin else src
    single_pad = max(counts)                               # an empty batch list raises here, as in the reference
    groups = dn_groups(dn_number, single_pad)
    pad2, N = single_pad * 2 * groups, sum(counts)
    K = 2 * groups * N
    pad1 = cons.single_pad * cons.groups if cons is not None else 0
    if pad2 == 0:                                          # prepare_for_cdn, every image empty: nothing to launch
        z = weight.new_zeros
        return dict(query_label=z((B, 0, hidden_dim), dtype=torch.float32), query_bbox=z((B, 0, 4), dtype=torch.float32),
                    attn_mask=z((num_queries, num_queries), dtype=torch.bool), groups=groups, pad=0, single_pad=0,
                    known_bid=z((0,), dtype=torch.int64), map_known_indice=z((0,), dtype=torch.int64), pad_mask=None,
                    cons_label=None, noised_labels=z((0,), dtype=torch.int64))
    u = _noise(noise, generator, K * NOISE_COLS + (B if standin else 0), dev)
    p = _Build()
    p.dn = make_layout(counts, single_pad, 2 * groups)
    if cons is not None:
        p.cons = cons
    keep = [u]
    box_stride = 4
    for b, n in enumerate(src):
        p.src_counts[b] = n
        if n:
            lab, box = _entry(labels_list[b], torch.int64, dev), _entry(boxes_list[b], torch.float32, dev)
            if box.dim() != 2 or box.shape[1] != 4:
                raise ValueError(f"dn_query: boxes must be (n, 4) normalised cxcywh, got {tuple(box.shape)}")
            keep += [lab, box]
            p.labels[b], p.boxes[b] = lab.data_ptr(), box.data_ptr()
    p.box_stride, p.num_known = box_stride, K
    p.num_classes, p.num_queries = int(num_classes), int(num_queries)
    p.noise = u.data_ptr()
    p.image_noise = u.data_ptr() + 4 * K * NOISE_COLS if standin else None
    p.label_noise_threshold = float(label_noise_ratio) * 0.5 if label_noise_ratio > 0 else 0.0
    p.box_noise_scale = float(box_noise_scale)
    st = dict(B=B, pad1=pad1, pad2=pad2, K=K, K1=0 if cons is None else cons.groups * cons.offsets[B], params=p,
              num_queries=int(num_queries), want_pad_mask=want_pad_mask, cons=cons, keep=keep)
    q_label, q_bbox, mask, bid, mp, noised, pad_mask, cons_label = _DnBuildFn.apply(weight, cons_rows, st)
    return dict(query_label=q_label, query_bbox=q_bbox, attn_mask=mask, groups=groups, pad=pad2, single_pad=single_pad,
                known_bid=bid, map_known_indice=mp, pad_mask=pad_mask, cons_label=cons_label, noised_labels=noised)


def prepare_for_cdn(dn_args, training, num_queries, num_classes, hidden_dim, label_enc, *, noise=None, generator=None):
    """dn_components.py:6-125.  ``noise``: ``K * 10`` uniform values (module docstring)."""
    if not training:
        return None, None, None, None
    targets, dn_number, label_noise_ratio, box_noise_scale = dn_args
    r = _cdn(list(targets["labels"]), list(targets["boxes"]), False, dn_number, label_noise_ratio, box_noise_scale,
             num_queries, num_classes, hidden_dim, _label_weight(label_enc), noise, generator)
    return r["query_label"], r["query_bbox"], r["attn_mask"], {"pad_size": r["pad"], "num_dn_group": r["groups"]}


def prepare_for_cdn_plus(dn_args, training, num_queries, num_classes, hidden_dim, label_enc, *, noise=None, generator=None):
    """dn_components.py:128-274: an image without ground truths gets a stand-in box and ``pad_mask`` 1.  ``noise``:
    ``K * 10 + B`` uniform values."""
    if not training:
        return None, None, None, None
    targets, dn_number, label_noise_ratio, box_noise_scale = dn_args
    r = _cdn(list(targets["labels"]), list(targets["boxes"]), True, dn_number, label_noise_ratio, box_noise_scale,
             num_queries, num_classes, hidden_dim, _label_weight(label_enc), noise, generator, want_pad_mask=True)
    return r["query_label"], r["query_bbox"], r["attn_mask"], {"pad_size": r["pad"], "num_dn_group": r["groups"],
                                                                "pad_mask": r["pad_mask"]}


def consistency_queries(pseudo_bboxes, det_bboxes, tgt_shapes, src_shapes, loss_weight=1.0, with_rois=True,
                        with_loss_weights=True):
    """The box half of the consistency queries (dino_detr_ssod.py:507-593): per-image pseudo boxes (n, 4) xyxy pixels of the
    target view, detected boxes (n, >= 4) of the source view, ``img_shape`` tuples of both -> dict(query_bbox (B, pad1, 4),
    known_bid (K1,) fp32, map_known_indice (K1,) int64, loss_weights (K1, 1), rois (K1, 5), layout, pad, single_pad).
    An image without boxes gets the central half of the image as its box, weight 0."""
    src = [int(t.shape[0]) for t in pseudo_bboxes]
    B = len(src)
    dev = pseudo_bboxes[0].device
    _require_cuda(pseudo_bboxes[0], "pseudo boxes")
    if with_rois and [int(t.shape[0]) for t in det_bboxes] != src:
        raise ValueError("dn_query: pseudo boxes and detected boxes disagree on the list lengths")
    counts = [max(n, 1) for n in src]
    single_pad = max(counts)
    lay = make_layout(counts, single_pad, CONSISTENCY_GROUPS)
    K1, pad1 = CONSISTENCY_GROUPS * sum(counts), CONSISTENCY_GROUPS * single_pad
    p = _Consistency()
    p.cons = lay
    keep = []
    det_stride = {int(t.shape[1]) for t, n in zip(det_bboxes, src) if n} if with_rois else set()
    if len(det_stride) > 1:                                # mixed (n, 4) / (n, 5) lists: one stride for the kernel
        det_bboxes, det_stride = [t[:, :4] for t in det_bboxes], {4}
    for b, n in enumerate(src):
        p.src_counts[b] = n
        h, w = tgt_shapes[b][0], tgt_shapes[b][1]
        p.tgt_wh[b][0], p.tgt_wh[b][1] = float(w), float(h)
        h, w = src_shapes[b][0], src_shapes[b][1]
        p.src_wh[b][0], p.src_wh[b][1] = float(w), float(h)
        if n:
            box = _entry(pseudo_bboxes[b], torch.float32, dev)
            if box.dim() != 2 or box.shape[1] != 4:
                raise ValueError(f"dn_query: pseudo boxes must be (n, 4) xyxy, got {tuple(box.shape)}")
            keep.append(box)
            p.pseudo_boxes[b] = box.data_ptr()
            if with_rois:
                det = _entry(det_bboxes[b], torch.float32, dev)
                keep.append(det)
                p.det_boxes[b] = det.data_ptr()
    p.pseudo_stride, p.det_stride, p.num_known = 4, (det_stride.pop() if det_stride else 4), K1
    q_bbox = torch.empty((B, pad1, 4), dtype=torch.float32, device=dev)
    bid = torch.empty((K1,), dtype=torch.float32, device=dev)
    mp = torch.empty((K1,), dtype=torch.int64, device=dev)
    lw = torch.empty((K1, 1), dtype=torch.float32, device=dev) if with_loss_weights else None
    rois = torch.empty((K1, 5), dtype=torch.float32, device=dev) if with_rois else None
    p.query_bbox, p.known_bid, p.map_known_indice = q_bbox.data_ptr(), bid.data_ptr(), mp.data_ptr()
    p.loss_weights = lw.data_ptr() if lw is not None else None
    p.rois = rois.data_ptr() if rois is not None else None
    p.loss_weight = float(loss_weight)
    _lib.call("semidetr_dn_consistency_f32", dev, ctypes.byref(p))
    return dict(query_bbox=q_bbox, known_bid=bid, map_known_indice=mp, loss_weights=lw, rois=rois, layout=lay, pad=pad1,
                single_pad=single_pad)


def prepare_unsup_cdn(self, teacher_info, student_info, pseudo_bboxes, pseudo_labels, det_bboxes, det_laebls, dn_args=None,
                      hidden_dim=256, num_queries=900, num_classes=80, prior_info=None, *, noise=None, generator=None):
    """``DinoDetrSSOD.prepare_unsup_cdn`` (dino_detr_ssod.py:484-760): the consistency queries followed by the contrastive
    de-noising queries.  ``noise``: ``K2 * 10 + B`` uniform values (module docstring)."""
    tgt_shapes = [m["img_shape"] for m in student_info["img_metas"]]
    src_shapes = [m["img_shape"] for m in teacher_info["img_metas"]]
    head = self.student.bbox_head
    warm = self.curr_step < head.warm_up_step
    first = prior_info is None
    c = consistency_queries(list(pseudo_bboxes), list(det_bboxes), tgt_shapes, src_shapes, loss_weight=1.0 if warm else 0.0,
                            with_rois=first, with_loss_weights=first or not warm)
    cons_rows = None
    if first:
        with torch.no_grad():
            mlvl_feats = self.teacher.extract_feat(teacher_info["img"])
            mlvl_feats, _, _ = self.prepare_feats(mlvl_feats, teacher_info["img_metas"])
            embed = self.roi_extractor(mlvl_feats, c["rois"])
        cons_rows = self.projector(embed)
        loss_weights = c["loss_weights"]
    else:
        # past the warm-up the reference returns zeros_like(prior weights): the kernel has written them (loss_weight 0)
        loss_weights = prior_info["loss_weights"] if warm else c["loss_weights"].view_as(prior_info["loss_weights"])
    targets, dn_number, label_noise_ratio, box_noise_scale = dn_args
    r = _cdn(list(targets["labels"]), list(targets["boxes"]), True, dn_number, label_noise_ratio, box_noise_scale,
             num_queries, num_classes, hidden_dim, _label_weight(head.label_enc), noise, generator, cons=c["layout"],
             cons_rows=cons_rows)
    label_1 = r["cons_label"] if first else prior_info["input_query_label_1"]
    dn_meta = {"pad_size_1": c["pad"], "pad_size_2": r["pad"], "num_dn_group_1": CONSISTENCY_GROUPS,
               "num_dn_group_2": r["groups"], "known_bid_1": c["known_bid"], "known_bid_2": r["known_bid"],
               "map_known_indice_1": c["map_known_indice"], "map_known_indice_2": r["map_known_indice"],
               "loss_weights": loss_weights}
    return label_1, c["query_bbox"], r["query_label"], r["query_bbox"], r["attn_mask"], dn_meta
