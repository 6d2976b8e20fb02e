"""A plain float64 statement of the detection decode at evaluation time -- ``get_bboxes`` / ``_get_bboxes_single`` with
``for_pseudo_label=False`` (detr_od/models/dense_heads/dino_detr_ssod_head.py:1316-1330, 1396-1413; dino_detr_head.py:
1129-1137, 1143-1152) and mmdet's ``bbox2result`` (mmdet/core/bbox/transforms.py:100-117) -- with per-element bounds on what an
fp32 implementation may differ by, the seeded inputs of tests/golden/detect.npz, and mutants.  numpy only.

Decisions.  The k detections of an image are the k largest of its Q * C logits by (logit descending, flat index q * C + c
ascending), NaN above +inf, -0 == +0.  No arithmetic is involved, so an implementation that selects on the fp32 logits equals
this statement index for index.  The reference selects on fp32 sigmoids with ``torch.topk``, which leaves the order among equal
scores open; sigmoid is monotone, so wherever the reference's k + 1 best fp32 scores are pairwise distinct its choice and order
are this statement's, and elsewhere this statement is one of the results it admits.

Values, with u = 2^-24 (one rounding) and inputs that are exact fp32 numbers.
  x1 = (cx - 0.5 w) W: 0.5 w is exact, the difference rounds once, the product once: |err| <= (2 u + u^2) |x1|.  The clamp to
  [0, W] does not enlarge a difference (W is an integer, exact), so the same bound E holds behind it.  The division by the fp32
  scale factor s rounds once more: |err| <= E / s (1 + u) + u |clamp / s|.  Times 1.01 for the second-order terms.
  score = 1 / (1 + exp(-x)): exp within one ulp (2 u), the sum u, the quotient u, all relative and damped by e / (1 + e) <= 1:
  4 u score + 2^-126 (tests/query_select_ref64.py states the same bound for the same sigmoid).
Labels, indices, the class partition and the offsets are integers: exact.
"""
import zlib

import numpy as np

U = 2.0 ** -24
TINY = 2.0 ** -126
F32 = np.float32

MUTANTS = ("ties_high", "swap_divmod", "clamp_first", "rescale_whhw", "unstable_partition", "offsets_off_by_one",
           "first_layer")
TIE_KINDS = ("dup_chunks", "quantized", "all_equal", "saturated", "inf_nan", "zeros")


def sigmoid(x):
    with np.errstate(over="ignore"):
        return 1.0 / (1.0 + np.exp(-np.asarray(x, np.float64)))


def seeded_inputs(seed, kind, L, B, Q, C, k):
    """-> (all_cls_scores (L, B, Q, C), all_bbox_preds (L, B, Q, 4)) float32, from the seed alone.

    ``plain``: every image's logits are a random permutation of a jittered grid on [-10, 0), whose neighbours are ~1e-4 apart:
    their fp32 sigmoids are pairwise distinct.  The tie kinds start from that and overwrite logits.  Boxes: centres in
    [-0.2, 1.2), sizes in [0, 0.8) -- so boxes leave the image on every side -- with w = 0 for every 7th query, h = 0 for every
    11th (zero-size boxes)."""
    rng = np.random.default_rng(int(seed))
    n = Q * C
    cls = np.empty((L, B, n), F32)
    for l in range(L):
        for b in range(B):
            grid = -10.0 + 10.0 * (np.arange(n) + 0.5 * rng.random(n)) / n
            cls[l, b] = grid[rng.permutation(n)].astype(F32)
    box = np.concatenate([rng.random((L, B, Q, 2)) * 1.4 - 0.2, rng.random((L, B, Q, 2)) * 0.8], -1).astype(F32)
    box[:, :, ::7, 2] = 0
    box[:, :, ::11, 3] = 0
    last = cls[-1]                                               # the tie kinds concern the layer that is used
    if kind == "dup_chunks":                                     # k + 37 copies of one top value, on and around every 8192nd
        pos = sorted({p for m in range(0, n, 8192) for p in (m - 1, m, m + 1) if 0 <= p < n} | {n - 1})
        pos = (pos + [p for p in range(5, n, max(n // (k + 37), 1)) if p not in set(pos)])[:k + 37]
        last[:, pos] = F32(1.5)
    elif kind == "quantized":                                    # ~40 distinct values: ties everywhere, the k-th included
        last[:] = np.round(last * 4) / 4
    elif kind == "all_equal":
        last[:] = F32(0.5)
    elif kind == "saturated":                                    # distinct logits above 17: every fp32 sigmoid is 1.0
        last[:] = last + F32(40)
    elif kind == "inf_nan":
        last[:, 3::max(n // 5, 1)] = np.inf
        last[:, 1::max(n // 7, 1)] = -np.inf
        last[0, n // 2] = np.nan
    elif kind == "zeros":                                        # -0 and +0 alternate at the top, more of them than k
        pos = np.arange(2, n, max(n // (k + 9), 1))[:k + 9]
        last[:, pos] = np.where(np.arange(len(pos)) % 2 == 0, F32(-0.0), F32(0.0))
    elif kind != "plain":
        raise KeyError(kind)
    return cls.reshape(L, B, Q, C), box


def checksum(cls, box):
    return np.int64(zlib.crc32(np.ascontiguousarray(cls).tobytes() + np.ascontiguousarray(box).tobytes()))


def select(logits, k, mutant=None):
    """logits (B, Q * C) -> indices (B, k) sorted by (logit descending, flat index ascending); NaN above +inf; -0 == +0."""
    lg = np.asarray(logits, np.float64)
    B, n = lg.shape
    out = np.zeros((B, k), np.int64)
    idx = np.arange(n)
    for b in range(B):
        nan = np.isnan(lg[b])
        kv = np.where(nan, 0.0, lg[b]) + 0.0
        out[b] = np.lexsort((-idx if mutant == "ties_high" else idx, -kv, ~nan))[:k]
    return out


def decode(logits, boxes, idx, img_hw, scale, mutant=None):
    """logits (B, Q, C), boxes (B, Q, 4), idx (B, k), img_hw (B, 2) (height, width), scale (B, 4) or None ->
    dict(dets (B, k, 5) float64, bound (B, k, 5), labels (B, k) int64)."""
    B, Q, C = logits.shape
    lg, bx = np.asarray(logits, np.float64).reshape(B, -1), np.asarray(boxes, np.float64)
    n = np.arange(B)[:, None]
    if mutant == "swap_divmod":
        labels, q = idx // C, np.minimum(idx % C, Q - 1)
    else:
        labels, q = idx % C, idx // C
    score = sigmoid(lg[n, idx])
    cx, cy, w, h = (bx[n, q, j] for j in range(4))
    xyxy = np.stack([cx - 0.5 * w, cy - 0.5 * h, cx + 0.5 * w, cy + 0.5 * h], -1)
    hw = np.asarray(img_hw, np.float64)
    top = np.stack([hw[:, 1], hw[:, 0], hw[:, 1], hw[:, 0]], -1)[:, None, :]
    if mutant == "clamp_first":
        scaled = np.clip(xyxy, 0, top) * top
        clamped = scaled
    else:
        scaled = xyxy * top
        clamped = np.clip(scaled, 0, top)
    E = 1.01 * 2 * U * np.abs(scaled)
    if scale is not None:
        s = np.asarray(scale, np.float64)[:, None, :]
        if mutant == "rescale_whhw":
            s = s[..., [0, 1, 1, 0]]
        clamped = clamped / s
        E = 1.01 * (E / s + U * np.abs(clamped))
    dets = np.concatenate([clamped, score[..., None]], -1)
    bound = np.concatenate([E + TINY, np.where(np.isnan(score), TINY, 4 * U * score + TINY)[..., None]], -1)      # NaN stays NaN
    return dict(dets=dets, bound=bound, labels=labels.astype(np.int64))


def group(labels, C, mutant=None):
    """bbox2result as a permutation: labels (B, k) -> (order (B, k): grouped row j is row order[b, j], offsets (B, C + 1))."""
    B, k = labels.shape
    order, offsets = np.zeros((B, k), np.int64), np.zeros((B, C + 1), np.int32)
    for b in range(B):
        rank = -np.arange(k) if mutant == "unstable_partition" else np.arange(k)
        order[b] = np.lexsort((rank, labels[b]))
        counts = np.bincount(np.minimum(labels[b], C - 1), minlength=C)
        offsets[b, 1:] = np.cumsum(counts)
        if mutant == "offsets_off_by_one":
            offsets[b, :-1] = offsets[b, 1:]
    return order, offsets


def statement(all_cls, all_box, img_hw, scale, k, mutant=None):
    """The whole path on (L, B, Q, C) / (L, B, Q, 4) inputs -> dict(idx, dets, bound, labels, order, offsets, grouped)."""
    layer = 0 if mutant == "first_layer" else -1
    cls, box = np.asarray(all_cls[layer], F32), np.asarray(all_box[layer], F32)
    B, Q, C = cls.shape
    idx = select(cls.reshape(B, -1), k, mutant)
    out = decode(cls, box, idx, img_hw, scale, mutant)
    order, offsets = group(out["labels"], C, mutant)
    n = np.arange(B)[:, None]
    out.update(idx=idx, order=order, offsets=offsets, grouped=out["dets"][n, order])
    return out


def split(grouped, offsets, num_classes):
    """(k, 5) grouped rows + (C + 1,) offsets of one image -> bbox2result's list of per-class arrays."""
    C = len(offsets) - 1
    return [grouped[offsets[c]:offsets[c + 1]] if c < C else grouped[:0] for c in range(num_classes)]
