"""The de-noising / consistency query builders on the MI355X (csrc/dn_query.hip) against the reference's fixtures
(tests/golden/dn_query.npz) and the fp64 restatement with its fp32 error bounds (tests/dn_ref64.py)."""
import ctypes
import os
import types

import numpy as np
import pytest
import torch

import dn_ref64 as R
from test_dn_query_ref import CASES, CDN, NAMES, UNSUP, _params, ref_case

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")


def _split(a, counts):
    offs = np.concatenate([[0], np.cumsum(counts)]).astype(int)
    return [torch.from_numpy(np.ascontiguousarray(a[i:j])).to(DEV) for i, j in zip(offs[:-1], offs[1:])]


def _embedding(c):
    enc = torch.nn.Embedding(*c["weight"].shape).to(DEV)
    enc.weight.data = torch.from_numpy(c["weight"]).to(DEV)
    return enc


def _dn_args(c):
    dn_number, ratio, scale, nq, nc, H = _params(c)
    counts = [int(x) for x in c["counts"]]
    t = {"labels": _split(c["labels"], counts), "boxes": _split(c["boxes"].astype(np.float32), counts)}
    return (t, dn_number, ratio, scale), nq, nc, H


def _np(t):
    return t.detach().cpu().numpy()


def _check_bbox(got, want, bound, what):
    err = np.abs(_np(got).astype(np.float64) - want)
    worst = (err / np.where(bound > 0, bound, 1.0))[bound > 0].max(initial=0.0)
    print(f"[dn_query] {what}: worst err / bound = {worst:.3f}")
    assert (err <= bound).all(), (what, worst)


@pytest.mark.parametrize("name", CDN)
def test_cdn_and_plus_reproduce_the_fixture(name):
    import semi_detr_amd as s
    c = CASES[name]
    r, _ = ref_case(c)
    args, nq, nc, H = _dn_args(c)
    enc = _embedding(c)
    fn = s.prepare_for_cdn_plus if int(c["kind"]) else s.prepare_for_cdn
    noise = torch.from_numpy(c["u"]).to(DEV)
    ql, qb, mask, meta = fn(args, True, nq, nc, H, enc, noise=noise)
    assert (ql.dtype, qb.dtype, mask.dtype) == (torch.float32, torch.float32, torch.bool)
    assert [meta["pad_size"], meta["num_dn_group"]] == list(c["meta"]) and sorted(meta) == \
        (["num_dn_group", "pad_mask", "pad_size"] if int(c["kind"]) else ["num_dn_group", "pad_size"])
    assert _np(ql).tobytes() == c["query_label"].tobytes() and ql.shape == c["query_label"].shape
    assert np.array_equal(_np(mask), R.unpack_mask(c))
    assert qb.shape == c["query_bbox"].shape
    _check_bbox(qb, c["query_bbox"], r["bbox_bound"], name)
    if int(c["kind"]):
        assert meta["pad_mask"].dtype == torch.int64 and np.array_equal(_np(meta["pad_mask"]), c["pad_mask"])
    if meta["pad_size"] == 0:
        return
    # backward: fixed-order sum, within the ordered-sum bound and bitwise equal across two runs
    g = torch.from_numpy(R.grad_pattern(ql.shape, 1)).to(DEV)
    grads = []
    for _ in range(2):
        enc.weight.grad = None
        ql2, *_ = fn(args, True, nq, nc, H, enc, noise=noise)
        ql2.backward(g)
        grads.append(_np(enc.weight.grad).copy())
    assert grads[0].tobytes() == grads[1].tobytes()
    want, bound = R.grad_weight(_np(g), r["known_bid"], r["map_known_indice"], r["noised"], c["weight"].shape[0])
    assert np.abs(want - c["grad_weight"]).max() <= 1e-12
    assert (np.abs(grads[0].astype(np.float64) - want) <= bound + 0.0).all()


def _unsup_self(c, rec):
    step, warm, prior = (int(x) for x in c["step"])
    head = types.SimpleNamespace(warm_up_step=warm, label_enc=_embedding(c))
    proj = torch.from_numpy(c["proj"]).to(DEV).requires_grad_(True)

    def extractor(feats, rois):
        rec["rois"] = rois
        return "roi_feats"
    return types.SimpleNamespace(curr_step=step, student=types.SimpleNamespace(bbox_head=head),
                                 teacher=types.SimpleNamespace(extract_feat=lambda img: "feats"),
                                 prepare_feats=lambda f, m: (f, None, None), roi_extractor=extractor,
                                 projector=lambda x: proj * 1.0), proj


@pytest.mark.parametrize("name", UNSUP)
def test_unsup_reproduces_the_fixture(name):
    import semi_detr_amd as s
    c = CASES[name]
    r, cons = ref_case(c)
    step, warm, prior = (int(x) for x in c["step"])
    args, nq, nc, H = _dn_args(c)
    counts = [int(x) for x in c["counts"]]
    B = len(counts)
    rec = {}
    self, proj = _unsup_self(c, rec)
    img = torch.zeros(B, 3, 4, 4, device=DEV)
    tinfo = {"img": img, "img_metas": [{"img_shape": tuple(x)} for x in c["shapes_src"].tolist()]}
    sinfo = {"img": img, "img_metas": [{"img_shape": tuple(x)} for x in c["shapes_tgt"].tolist()]}
    prior_info = None
    if prior:
        prior_info = {"loss_weights": torch.from_numpy(c["prior_loss_weights"]).to(DEV),
                      "input_query_label_1": torch.from_numpy(c["label_1"]).to(DEV)}
    l1, b1, l2, b2, mask, meta = s.prepare_unsup_cdn(self, tinfo, sinfo, _split(c["pseudo"], counts), args[0]["labels"],
                                                     _split(c["det"], counts), args[0]["labels"], dn_args=args, hidden_dim=H,
                                                     num_queries=nq, num_classes=nc, prior_info=prior_info,
                                                     noise=torch.from_numpy(c["u"]).to(DEV))
    assert sorted(meta) == sorted(["pad_size_1", "pad_size_2", "num_dn_group_1", "num_dn_group_2", "known_bid_1", "known_bid_2",
                                   "map_known_indice_1", "map_known_indice_2", "loss_weights"])
    assert [meta["pad_size_1"], meta["pad_size_2"], meta["num_dn_group_1"], meta["num_dn_group_2"]] == list(c["meta"])
    assert _np(l1).tobytes() == c["label_1"].tobytes() and _np(l2).tobytes() == c["query_label"].tobytes()
    assert np.array_equal(_np(mask), R.unpack_mask(c))
    _check_bbox(b1, c["bbox_1"], cons["bbox_bound"], name + " consistency")
    _check_bbox(b2, c["query_bbox"], r["bbox_bound"], name + " dn")
    assert meta["known_bid_1"].dtype == torch.float32 and np.array_equal(_np(meta["known_bid_1"]), c["known_bid_1"])
    assert meta["known_bid_2"].dtype == torch.int64 and np.array_equal(_np(meta["known_bid_2"]), c["known_bid_2"])
    assert np.array_equal(_np(meta["map_known_indice_1"]), c["map_1"]) and meta["map_known_indice_1"].dtype == torch.int64
    assert np.array_equal(_np(meta["map_known_indice_2"]), c["map_2"])
    assert meta["loss_weights"].shape == c["loss_weights"].shape and np.array_equal(_np(meta["loss_weights"]), c["loss_weights"])
    if prior:
        return
    assert np.array_equal(_np(rec["rois"]).astype(np.float64), c["rois"]) and rec["rois"].dtype == torch.float32
    g2 = torch.from_numpy(R.grad_pattern(l2.shape, 1)).to(DEV)
    g1 = torch.from_numpy(R.grad_pattern(l1.shape, 2)).to(DEV)
    torch.autograd.backward([l2, l1], [g2, g1])
    assert np.array_equal(_np(proj.grad).astype(np.float64), c["grad_proj"])          # a gather: exact
    want, bound = R.grad_weight(_np(g2), r["known_bid"], r["map_known_indice"], r["noised"], c["weight"].shape[0])
    assert (np.abs(_np(self.student.bbox_head.label_enc.weight.grad).astype(np.float64) - want) <= bound).all()


def test_c_abi_directly_on_a_fixture_case():
    """semidetr_dn_build_f32 by hand (no Python front end): cdn_mixed, every output."""
    from semi_detr_amd import _lib
    from semi_detr_amd import dn_query as d
    c = CASES["cdn_mixed"]
    r, _ = ref_case(c)
    dn_number, ratio, scale, nq, nc, H = _params(c)
    counts = [int(x) for x in c["counts"]]
    labs, boxes = _split(c["labels"], counts), _split(c["boxes"].astype(np.float32), counts)
    w, u = torch.from_numpy(c["weight"]).to(DEV), torch.from_numpy(c["u"]).to(DEV)
    p = d._Build()
    p.dn = d.make_layout(counts, r["single_pad"], 2 * r["groups"])
    for b, n in enumerate(counts):
        p.src_counts[b] = n
        if n:
            p.labels[b], p.boxes[b] = labs[b].data_ptr(), boxes[b].data_ptr()
    K, pad, B = r["K"], r["pad"], len(counts)
    p.box_stride, p.num_known, p.label_weight, p.num_embeddings, p.hidden_dim = 4, K, w.data_ptr(), w.shape[0], H
    p.num_classes, p.num_queries, p.noise = nc, nq, u.data_ptr()
    p.label_noise_threshold, p.box_noise_scale = ratio * 0.5, scale
    ql = torch.full((B, pad, H), 7.0, device=DEV)
    qb = torch.full((B, pad, 4), 7.0, device=DEV)
    ints = torch.full((3, K), -7, dtype=torch.int64, device=DEV)
    mask = torch.full((pad + nq, pad + nq), 1, dtype=torch.uint8, device=DEV)
    p.query_label, p.query_bbox, p.attn_mask = ql.data_ptr(), qb.data_ptr(), mask.data_ptr()
    p.known_bid, p.map_known_indice, p.noised_labels = ints[0].data_ptr(), ints[1].data_ptr(), ints[2].data_ptr()
    _lib.check(_lib.lib().semidetr_dn_build_f32(_lib.current_stream_ptr(), ctypes.byref(p)), "semidetr_dn_build_f32")
    torch.cuda.synchronize()
    assert _np(ql).tobytes() == c["query_label"].tobytes()
    assert np.array_equal(_np(mask).astype(bool), R.unpack_mask(c))
    assert np.array_equal(_np(ints[0]), r["known_bid"]) and np.array_equal(_np(ints[1]), r["map_known_indice"])
    assert np.array_equal(_np(ints[2]), r["noised"])
    _check_bbox(qb, c["query_bbox"], r["bbox_bound"], "C ABI cdn_mixed")


def _bench_shaped(B, seed):
    rng = np.random.default_rng(seed)
    counts = [int(x) for x in rng.integers(10, 31, B)]
    labs = [torch.from_numpy(rng.integers(0, 80, n)).to(DEV) for n in counts]
    boxes = [torch.from_numpy(np.concatenate([rng.random((n, 2)) * 0.6 + 0.2, rng.random((n, 2)) * 0.3 + 0.02], 1)
                              .astype(np.float32)).to(DEV) for n in counts]
    return counts, {"labels": labs, "boxes": boxes}


@pytest.mark.parametrize("B", [4, 1])
def test_bench_shaped_calls_do_not_synchronise(B):
    import semi_detr_amd as s
    counts, t = _bench_shaped(B, B)
    enc = torch.nn.Embedding(81, 256).to(DEV)
    pix = [torch.cat([b[:, :2] * 500, b[:, :2] * 500 + b[:, 2:] * 400 + 2], 1).contiguous() for b in t["boxes"]]
    det = [torch.cat([p, p[:, :1]], 1).contiguous() for p in pix]
    metas = [{"img_shape": (800, 1200, 3)}] * B
    info = {"img": torch.zeros(B, 3, 8, 8, device=DEV), "img_metas": metas}
    K1 = 5 * sum(counts)
    rows = torch.randn(K1, 256, device=DEV, requires_grad=True)
    head = types.SimpleNamespace(warm_up_step=100, label_enc=enc)
    self = types.SimpleNamespace(curr_step=3, student=types.SimpleNamespace(bbox_head=head),
                                 teacher=types.SimpleNamespace(extract_feat=lambda img: None),
                                 prepare_feats=lambda f, m: (f, None, None), roi_extractor=lambda f, r: None,
                                 projector=lambda x: rows)
    gen = torch.Generator(device=DEV)
    gen.manual_seed(1)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        for fn in (s.prepare_for_cdn, s.prepare_for_cdn_plus):
            ql, qb, mask, meta = fn((t, 100, 0.5, 1.0), True, 900, 80, 256, enc, generator=gen)
            ql.sum().backward()
        out = s.prepare_unsup_cdn(self, info, info, pix, t["labels"], det, t["labels"], dn_args=(t, 100, 0.5, 1.0), generator=gen)
        (out[0].sum() + out[2].sum()).backward()
        prior = {"loss_weights": out[5]["loss_weights"], "input_query_label_1": out[0].detach()}
        with torch.no_grad():
            out2 = s.prepare_unsup_cdn(self, info, info, pix, t["labels"], det, t["labels"], dn_args=(t, 100, 0.5, 1.0),
                                       prior_info=prior, generator=gen)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    groups = 200 // (2 * max(counts))
    assert meta["pad_size"] == 2 * groups * max(counts) and mask.shape == (meta["pad_size"] + 900,) * 2
    assert out[0].shape == (B, 5 * max(counts), 256) and out2[0] is prior["input_query_label_1"]
    assert out[4].shape == (5 * max(counts) + meta["pad_size"] + 900,) * 2
    assert torch.equal(out[4], out2[4]) and rows.grad is not None and enc.weight.grad is not None


def test_generator_determinism_and_noise_statistics():
    import semi_detr_amd as s
    counts, t = _bench_shaped(4, 9)
    enc = torch.nn.Embedding(81, 32).to(DEV)
    outs = []
    for _ in range(2):
        gen = torch.Generator(device=DEV)
        gen.manual_seed(1234)
        outs.append(s.prepare_for_cdn_plus((t, 100, 0.5, 1.0), True, 30, 80, 32, enc, generator=gen))
    for a, b in zip(outs[0][:3], outs[1][:3]):
        assert torch.equal(a, b)
    # a large draw: the flipped share is label_noise_ratio / 2 (a flip may redraw the same label: 1/80 of them), and a
    # negative's corner moves by |rand_part| in [1, 2) half-sizes
    n = 20
    labs = [torch.full((n,), 80, dtype=torch.long, device=DEV)] * 4         # label 80 is never drawn: every flip shows
    boxes = [torch.tensor([[0.5, 0.5, 0.1, 0.1]], device=DEV).repeat(n, 1)] * 4
    from semi_detr_amd import dn_query as d
    share, lo, hi, total = 0.0, 9.0, 0.0, 0
    for seed in range(20):
        gen = torch.Generator(device=DEV)
        gen.manual_seed(seed)
        r = d._cdn(labs, boxes, False, 100, 0.5, 0.2, 30, 80, 32, enc.weight, None, gen)
        K = r["noised_labels"].numel()
        share += float((r["noised_labels"] != 80).sum())
        total += K
        box = torch.sigmoid(r["query_bbox"][r["known_bid"], r["map_known_indice"]].double())     # noised cxcywh
        x1 = box[:, 0] - box[:, 2] / 2
        part = ((x1 - 0.45) / (0.05 * 0.2)).abs()                           # |rand_part| of x1
        neg = (torch.arange(K, device=DEV) // (4 * n)) % 2 == 1
        lo, hi = min(lo, float(part[neg].min())), max(hi, float(part[neg].max()))
        assert float(part[~neg].max()) < 1.0 + 1e-3
    share /= total
    sigma = (0.25 * 0.75 / total) ** 0.5
    assert abs(share - 0.25) < 5 * sigma, (share, total)
    assert 1.0 - 1e-3 <= lo and hi < 2.0 + 1e-3 and hi > 1.9 and lo < 1.1, (lo, hi)


def test_producer_dn_meta_feeds_loss_set():
    """the dn_meta prepare_for_cdn_plus writes is the one loss_set's dn segment reads"""
    import semi_detr_amd as s
    from test_gpu_set_loss import _call_loss, _e2e_inputs, _head
    d = _e2e_inputs(11, single_pad=14, groups=14)                          # gt counts [7, 0]: 14 groups of 2 * 7
    norm = []
    for g, m in zip(d["gts"], d["metas"]):
        h, w = m["img_shape"][:2]
        f = g.new_tensor([w, h, w, h])
        norm.append((torch.cat([(g[:, :2] + g[:, 2:]) / 2, g[:, 2:] - g[:, :2]], 1) / f).contiguous())
    enc = torch.nn.Embedding(81, 256).to(DEV)
    ql, qb, mask, meta = s.prepare_for_cdn_plus(({"labels": d["labs"], "boxes": norm}, 100, 0.5, 1.0), True, 300, 80, 256, enc)
    assert meta["pad_size"] == d["pad"] == 196 and meta["num_dn_group"] == 14
    assert ql.shape == (2, 196, 256) and mask.shape == (496, 496)
    assert int(meta["pad_mask"][0].sum()) == 0 and int(meta["pad_mask"][1].sum()) == 196
    d["dn_meta"] = meta
    out = _call_loss(_head(), d)
    total = sum(v for k, v in out.items() if "dn_" in k)
    total.backward()
    assert all(torch.isfinite(v) for v in out.values()) and float(out["dn_loss_bbox"]) > 0
    assert torch.isfinite(d["out_cls"].grad).all() and float(d["out_cls"].grad[:, :, :196].abs().sum()) > 0
