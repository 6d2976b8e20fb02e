"""float64 numpy restatement of the de-noising / consistency query builders, with vectorised indexing, and the fp32 error
bounds the GPU tests hold the kernels to.  It reproduces tests/golden/dn_query.npz (the reference's own functions run in
float64, tools/gen_dn_golden.py): integers and masks exactly, floats to 1e-12.

Noise layout (semi_detr_amd/dn_query.py): ``u (K, 10)``: 0 = p, 1 -> new label, 2..5 -> signs, 6..9 = rand_part; one more
value per image for the stand-in label of an empty image.

fp32 error bound of ``input_query_bbox`` (derived once, scaled by no test).  ``e = 2**-24`` is the unit roundoff.  The
pre-log value ``v`` (a noised cx, cy, w or h) comes from exactly representable inputs in [0, 1] through, per corner
``c = centre -+ size/2`` (|c| <= 1.5: e * 1.5), ``r = rand_part + 1`` (< 2: 2e), ``r * d`` (d <= 0.5: 2e carried + e),
``* scale`` (3e * scale), the sum (|.| <= 1.5 + scale: 1.5e + 3e * scale carried, e * (1.5 + scale) rounded): 3e + 4e * scale
per clamped corner; the clamp adds nothing; a centre ``(c0 + c2) / 2`` carries that once plus e, a size ``c2 - c0`` carries it
twice plus e.  So ``delta = (7 + 8 * scale) * e`` covers all four (fused multiply-adds round less often, not more).  For the
consistency boxes ``v = (x1 +- x2) [/ 2] / W``: two roundings relative to the unclamped value, ``delta = 3e * max(1, |v_raw|)``.
``inverse_sigmoid`` then forms ``x1 = max(v, eps)``, ``x2 = max(1 - v, eps)`` (one more rounding e; eps itself is rounded:
2e * eps) and ``log(x1 / x2)`` (division: relative e, i.e. e absolute in the log; logf: 2 ulp of the result):

    |err| <= (delta + 2e * eps) / x1w + (delta + e) / x2w + 4e * (1 + |ref|)

with ``x1w = max(v - delta, eps)``, ``x2w = max(1 - v - delta - e, eps)`` the worst points of ``[v - delta, v + delta]`` (v
clamped to [0, 1]): at the eps clamp the slope is 1e5, away from it ~1, so a flat tolerance would be wrong in both directions.
Copies (``input_query_label`` rows, the gather backward) are bit-exact.  The embedding-weight gradient is an ordered sum of
n terms per element: ``(n - 1) * e * sum |terms|``.
"""
import numpy as np

E32 = 2.0 ** -24
EPS = 1e-5
GROUPS_1 = 5


def grad_pattern(shape, salt):
    """Deterministic fp32-exact pseudo-random values in [-2, 2): what the fixtures' upstream gradients are (not stored)."""
    n = int(np.prod(shape))
    i = (np.arange(n, dtype=np.uint64) + np.uint64(salt)) * np.uint64(2654435761) % np.uint64(2 ** 32)
    return (((i >> np.uint64(16)).astype(np.float64) - 32768.0) / 16384.0).astype(np.float32).reshape(shape)


def dn_groups(dn_number, max_count):
    n = dn_number * 2
    if max_count == 0:
        n = 1
    elif n >= 100:
        n = n // (max_count * 2)
    elif n < 1:
        n = 1
    return n or 1


def inverse_sigmoid(x, eps=EPS):
    x = np.clip(x, 0.0, 1.0)
    return np.log(np.maximum(x, eps) / np.maximum(1.0 - x, eps))


def logit_bound(v, delta):
    """The bound above for pre-log values ``v`` (float64, unclamped) carrying the absolute error ``delta``."""
    v = np.clip(v, 0.0, 1.0)
    ref = inverse_sigmoid(v)
    x1w = np.maximum(v - delta, EPS)
    x2w = np.maximum(1.0 - v - delta - E32, EPS)
    return (delta + 2 * E32 * EPS) / x1w + (delta + E32) / x2w + 4 * E32 * (1.0 + np.abs(ref))


def layout(counts, single_pad, groups):
    """(known_bid, map_known_indice, source row) of the K = groups * N known rows, in the reference's order."""
    counts = np.asarray(counts, np.int64)
    bid = np.repeat(np.arange(len(counts)), counts)
    within = np.concatenate([np.arange(c) for c in counts]) if len(counts) else np.zeros(0, np.int64)
    g = np.arange(groups)
    return (np.tile(bid, groups), (within[None, :] + single_pad * g[:, None]).reshape(-1), np.tile(np.arange(len(bid)), groups))


def attn_mask(pad1, single1, pad2, single2x2, num_queries):
    """Closed form of both mask loops (dn_components.py:100-112 with pad1 = 0; dino_detr_ssod.py:722-743): a query sees its
    own group and the matching part; the matching part sees only itself."""
    P = pad1 + pad2
    tgt = P + num_queries
    idx = np.arange(tgt)
    grp = np.where(idx < pad1, idx // max(single1, 1), np.where(idx < P, 10 ** 6 + (idx - pad1) // max(single2x2, 1), -1))
    return (idx[None, :] < P) & ((idx[:, None] >= P) | (grp[:, None] != grp[None, :]))


def cdn(counts, labels, boxes, weight, u, dn_number, ratio, scale, num_queries, num_classes, standin, pad1=0, single1=0):
    """prepare_for_cdn (``standin`` False) / prepare_for_cdn_plus / the second half of prepare_unsup_cdn.  ``u`` flat."""
    counts = [int(c) for c in counts]
    B = len(counts)
    u = np.asarray(u, np.float32).reshape(-1)
    labels, boxes = np.asarray(labels, np.int64), np.asarray(boxes, np.float64).reshape(-1, 4)
    eff = [max(c, 1) for c in counts] if standin else counts
    single_pad = max(eff)
    groups = dn_groups(dn_number, single_pad)
    K = 2 * groups * sum(eff)
    u_img = u[K * 10:]
    u = u[:K * 10].reshape(K, 10)
    lab, box, at = [], [], 0
    for b, c in enumerate(counts):
        if c == 0 and standin:
            lab.append(np.asarray([int(np.float32(u_img[b]) * np.float32(80))], np.int64))
            box.append(np.full((1, 4), 0.5))
        else:
            lab.append(labels[at:at + c])
            box.append(boxes[at:at + c])
        at += c
    lab, box = np.concatenate(lab) if lab else np.zeros(0, np.int64), np.concatenate(box) if box else np.zeros((0, 4))
    pad = single_pad * 2 * groups
    H = weight.shape[1]
    out = dict(pad=pad, groups=groups, single_pad=single_pad, K=K,
               pad_mask=np.repeat((np.asarray(counts) == 0).astype(np.int64)[:, None], pad, 1) if standin else None,
               mask=attn_mask(pad1, single1, pad, 2 * single_pad, num_queries))
    bid, mp, srow = layout(eff, single_pad, 2 * groups)
    noised = lab[srow].copy()
    if ratio > 0:
        flip = u[:, 0].astype(np.float64) < ratio * 0.5
        new = np.minimum((u[:, 1] * np.float32(num_classes)).astype(np.float32).astype(np.int64), num_classes - 1)
        noised[flip] = new[flip]
    kb = box[srow]
    v = kb.copy()
    if scale > 0:
        xy = np.concatenate([kb[:, :2] - kb[:, 2:] / 2, kb[:, :2] + kb[:, 2:] / 2], 1)
        diff = np.concatenate([kb[:, 2:] / 2, kb[:, 2:] / 2], 1)
        part = u[:, 6:10].astype(np.float64)
        part[(np.arange(K) // max(len(lab), 1)) % 2 == 1] += 1.0
        part *= np.where(u[:, 2:6] >= np.float32(0.5), 1.0, -1.0)
        xy = np.clip(xy + part * diff * scale, 0.0, 1.0)
        v = np.concatenate([(xy[:, :2] + xy[:, 2:]) / 2, xy[:, 2:] - xy[:, :2]], 1)
    delta = (7 + 8 * max(scale, 0.0)) * E32
    ql, qb, bound = np.zeros((B, pad, H), np.float32), np.zeros((B, pad, 4)), np.zeros((B, pad, 4))
    if K:
        ql[bid, mp] = weight[noised]
        qb[bid, mp] = inverse_sigmoid(v)
        bound[bid, mp] = logit_bound(v, delta)
    out.update(query_label=ql, query_bbox=qb, bbox_bound=bound, known_bid=bid, map_known_indice=mp, noised=noised, pre_log=v)
    return out


def grad_weight(g_label, known_bid, map_known_indice, noised, num_embeddings):
    """(gradient of sum(query_label * g_label) w.r.t. the weight, its ordered-sum fp32 bound), float64."""
    g = np.asarray(g_label, np.float64)
    rows = g[known_bid, map_known_indice] if len(noised) else np.zeros((0, g.shape[-1]))
    grad, mag = np.zeros((num_embeddings, g.shape[-1])), np.zeros((num_embeddings, g.shape[-1]))
    np.add.at(grad, noised, rows)
    np.add.at(mag, noised, np.abs(rows))
    n = np.bincount(noised, minlength=num_embeddings).astype(np.float64)
    return grad, np.maximum(n - 1, 0)[:, None] * E32 * mag


def consistency(counts, pseudo, det, shapes_tgt, shapes_src, loss_weight=1.0):
    """The first half of prepare_unsup_cdn (dino_detr_ssod.py:507-593)."""
    counts = [int(c) for c in counts]
    B = len(counts)
    pseudo = np.asarray(pseudo, np.float64).reshape(-1, 4)
    det = None if det is None else np.asarray(det, np.float64)
    eff = [max(c, 1) for c in counts]
    single = max(eff)
    pb, db, lw, fac, at = [], [], [], [], 0
    for b, c in enumerate(counts):
        (h, w), (hs, ws) = shapes_tgt[b][:2], shapes_src[b][:2]
        if c == 0:
            pb.append(np.asarray([[w / 4, h / 4, 3 * w / 4, 3 * h / 4]]))
            db.append(np.asarray([[ws / 4, hs / 4, 3 * ws / 4, 3 * hs / 4]]))
            lw.append(np.zeros(1))
        else:
            pb.append(pseudo[at:at + c])
            if det is not None:
                db.append(det[at:at + c, :4])
            lw.append(np.full(c, float(loss_weight)))
        fac.append(np.tile(np.asarray([[w, h, w, h]], np.float64), (eff[b], 1)))
        at += c
    pb, fac = np.concatenate(pb), np.concatenate(fac)
    raw = np.concatenate([(pb[:, :2] + pb[:, 2:]) / 2, pb[:, 2:] - pb[:, :2]], 1) / fac
    bid, mp, srow = layout(eff, single, GROUPS_1)
    pad = GROUPS_1 * single
    qb, bound = np.zeros((B, pad, 4)), np.zeros((B, pad, 4))
    v = raw[srow]
    qb[bid, mp] = inverse_sigmoid(v)
    bound[bid, mp] = logit_bound(v, 3 * E32 * np.maximum(1.0, np.abs(v)))
    out = dict(query_bbox=qb, bbox_bound=bound, known_bid=bid.astype(np.float64), map_known_indice=mp, pad=pad, single_pad=single,
               loss_weights=np.concatenate(lw)[srow][:, None], layout=(bid, mp, srow), K=len(bid))
    if det is not None:
        out["rois"] = np.concatenate([bid[:, None].astype(np.float64), np.concatenate(db)[srow]], 1)
    return out


def scatter_rows(rows, lay, B, pad):
    bid, mp, _ = lay
    out = np.zeros((B, pad, rows.shape[1]), rows.dtype)
    out[bid, mp] = rows
    return out


def load_cases(path):
    z = np.load(path)
    cases = {}
    for k in z.files:
        if "." in k:
            c, name = k.split(".", 1)
            cases.setdefault(c, {})[name] = z[k]
    return cases


def unpack_mask(case):
    tgt = int(case["tgt"])
    return np.unpackbits(case["mask"])[:tgt * tgt].reshape(tgt, tgt).astype(bool)
