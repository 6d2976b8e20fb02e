"""CPU: tests/dn_ref64.py reproduces every case of tests/golden/dn_query.npz (the reference's own functions in float64),
both closed-form attention masks equal the reference's, the fp32 error bound accepts a float32 run of the reference's op
sequence and rejects mutants, ``registry.bind_dn_queries`` rebinds a fake module tree, and the dn_query C entry points reject
bad arguments on the host."""
import ctypes
import os
import sys
import types

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import dn_ref64 as R  # noqa: E402
import dn_torch_restated as T  # noqa: E402

CASES = R.load_cases(os.path.join(HERE, "golden", "dn_query.npz"))
NAMES = sorted(CASES)
CDN = [n for n in NAMES if int(CASES[n]["kind"]) < 2]
UNSUP = [n for n in NAMES if int(CASES[n]["kind"]) == 2]


def _params(c):
    dn_number, ratio, scale, nq, nc, H = c["params"]
    return int(dn_number), float(ratio), float(scale), int(nq), int(nc), int(H)


def ref_case(c):
    """dn_ref64 on a fixture case -> (cdn dict, consistency dict or None)."""
    dn_number, ratio, scale, nq, nc, H = _params(c)
    cons = None
    pad1 = single1 = 0
    if int(c["kind"]) == 2:
        step, warm, prior = (int(x) for x in c["step"])
        cons = R.consistency(c["counts"], c["pseudo"], c["det"], c["shapes_tgt"], c["shapes_src"], 1.0 if step < warm else 0.0)
        pad1, single1 = cons["pad"], cons["single_pad"]
    r = R.cdn(c["counts"], c["labels"], c["boxes"], c["weight"], c["u"], dn_number, ratio, scale, nq, nc,
              standin=int(c["kind"]) > 0, pad1=pad1, single1=single1)
    return r, cons


def test_fixture_covers_the_cases_the_feature_names():
    assert len(NAMES) == 16 and len(UNSUP) == 4
    assert int(CASES["cdn_empty"]["meta"][0]) == 0                                  # pad_size 0
    assert int(CASES["cdn_big"]["meta"][1]) == 1 and int(CASES["plus_big"]["meta"][1]) == 1
    assert int(CASES["cdn_one"]["meta"][1]) == 100
    assert _params(CASES["cdn_h256"])[5] == 256 and _params(CASES["cdn_no_label_noise"])[1] == 0
    assert _params(CASES["cdn_no_box_noise"])[2] == 0
    assert os.path.getsize(os.path.join(HERE, "golden", "dn_query.npz")) < (1 << 20)


@pytest.mark.parametrize("name", NAMES)
def test_ref64_reproduces_the_reference(name):
    c = CASES[name]
    r, cons = ref_case(c)
    assert np.array_equal(r["query_label"], c["query_label"])
    assert r["query_bbox"].shape == c["query_bbox"].shape
    assert np.abs(r["query_bbox"] - c["query_bbox"]).max(initial=0.0) <= 1e-12
    assert np.array_equal(r["mask"], R.unpack_mask(c))
    E = c["weight"].shape[0]
    g = R.grad_pattern(c["query_label"].shape, 1)
    gw, _ = R.grad_weight(g, r["known_bid"], r["map_known_indice"], r["noised"], E)
    assert np.abs(gw - c["grad_weight"]).max() <= 1e-12
    if int(c["kind"]) < 2:
        assert [r["pad"], r["groups"]] == list(c["meta"])
        if int(c["kind"]) == 1:
            assert np.array_equal(r["pad_mask"], c["pad_mask"])
        return
    step, warm, prior = (int(x) for x in c["step"])
    assert [cons["pad"], r["pad"], R.GROUPS_1, r["groups"]] == list(c["meta"])
    assert np.abs(cons["query_bbox"] - c["bbox_1"]).max() <= 1e-12
    assert np.array_equal(cons["known_bid"], c["known_bid_1"]) and np.array_equal(cons["map_known_indice"], c["map_1"])
    assert np.array_equal(r["known_bid"], c["known_bid_2"]) and np.array_equal(r["map_known_indice"], c["map_2"])
    if prior:
        want = c["prior_loss_weights"] if step < warm else np.zeros_like(c["prior_loss_weights"])
        assert np.array_equal(c["loss_weights"], want)
    else:
        assert np.array_equal(cons["loss_weights"], c["loss_weights"])
        assert np.array_equal(cons["rois"], c["rois"])
        B = len(c["counts"])
        assert np.array_equal(R.scatter_rows(c["proj"], cons["layout"], B, cons["pad"]), c["label_1"])
        g1 = R.grad_pattern(c["label_1"].shape, 2).astype(np.float64)
        assert np.array_equal(g1[cons["layout"][0], cons["layout"][1]], c["grad_proj"])


@pytest.mark.parametrize("counts", [[3, 0, 7, 1], [120, 2], [1], [50, 50]])
def test_closed_form_mask_against_the_group_loops(counts):
    """the closed form against the loops of dn_torch_restated (which the fixtures pin to the reference's masks below)"""
    w = torch.zeros(81, 4)
    labs = [torch.zeros(n, dtype=torch.long) for n in counts]
    boxes = [torch.full((n, 4), 0.5) for n in counts]
    groups = R.dn_groups(100, max(counts))
    u = torch.rand(2 * groups * sum(counts) * 10)
    for pad1, single1 in ((0, 0), (15, 3)):
        _, _, mask, pad, g, _ = T.cdn(labs, boxes, w, u, 100, 0.5, 1.0, 37, 80, False, pad1=pad1, single1=single1)
        assert np.array_equal(mask.numpy(), R.attn_mask(pad1, single1, pad, 2 * max(counts), 37))


def _float32_run(c, mutate=None):
    dn_number, ratio, scale, nq, nc, H = _params(c)
    counts = [int(x) for x in c["counts"]]
    offs = np.concatenate([[0], np.cumsum(counts)])
    labs = [torch.from_numpy(c["labels"][a:b]) for a, b in zip(offs[:-1], offs[1:])]
    boxes = [torch.from_numpy(c["boxes"][a:b].astype(np.float32)) for a, b in zip(offs[:-1], offs[1:])]
    return T.cdn(labs, boxes, torch.from_numpy(c["weight"]), torch.from_numpy(c["u"]), dn_number, ratio, scale, nq, nc,
                 int(c["kind"]) > 0, mutate=mutate)


def test_bound_accepts_float32_and_rejects_mutants(capsys):
    worst = 0.0
    rejected = {m: 0 for m in ("eps", "neg", "sign", "fp16")}
    for name in NAMES:
        c = CASES[name]
        if int(c["meta"][0 if int(c["kind"]) < 2 else 1]) == 0:
            continue
        r, _ = ref_case(c)
        ql, qb, *_ = _float32_run(c)
        assert np.array_equal(ql.numpy(), c["query_label"])
        err = np.abs(qb.numpy().astype(np.float64) - c["query_bbox"])
        ratio = (err[r["bbox_bound"] > 0] / r["bbox_bound"][r["bbox_bound"] > 0]).max()
        worst = max(worst, ratio)
        assert (err <= r["bbox_bound"]).all(), (name, ratio)
        for m in rejected:
            _, qm, *_ = _float32_run(c, mutate=m)
            rejected[m] += int((np.abs(qm.numpy().astype(np.float64) - c["query_bbox"]) > r["bbox_bound"]).any())
    with capsys.disabled():
        print(f"\n[dn_query] float32 restatement: worst err / bound = {worst:.3f}; cases rejecting each mutant: {rejected}")
    assert worst <= 1.0
    scaled = sum(1 for n in NAMES if _params(CASES[n])[2] > 0 and int(CASES[n]["meta"][0 if int(CASES[n]["kind"]) < 2 else 1]))
    assert rejected["neg"] == scaled and rejected["sign"] == scaled and rejected["fp16"] >= scaled
    assert rejected["eps"] >= 3                         # the cases whose boxes reach the eps clamp


def test_consistency_bound_accepts_float32():
    for name in UNSUP:
        c = CASES[name]
        _, cons = ref_case(c)
        counts = [int(x) for x in c["counts"]]
        offs = np.concatenate([[0], np.cumsum(counts)])
        ps = [torch.from_numpy(c["pseudo"][a:b]) for a, b in zip(offs[:-1], offs[1:])]
        ds = [torch.from_numpy(c["det"][a:b]) for a, b in zip(offs[:-1], offs[1:])]
        qb, bid, mp, lw, rois = T.consistency(ps, ds, c["shapes_tgt"].tolist(), c["shapes_src"].tolist(), torch.zeros(1))
        assert (np.abs(qb.numpy().astype(np.float64) - c["bbox_1"]) <= cons["bbox_bound"]).all()
        assert np.array_equal(mp.numpy(), c["map_1"]) and np.array_equal(bid.numpy(), c["known_bid_1"])
        assert np.array_equal(rois.numpy().astype(np.float64), cons["rois"])


def test_bind_dn_queries_on_a_fake_module_tree(monkeypatch):
    import semi_detr_amd as s
    from semi_detr_amd import registry
    done, skipped = registry.bind_dn_queries()
    assert done == [] and skipped == ["prepare_for_cdn", "prepare_for_cdn_plus", "DinoDetrSSOD.prepare_unsup_cdn"]

    def mod(name, **attrs):
        m = types.ModuleType(name)
        m.__path__ = []
        for k, v in attrs.items():
            setattr(m, k, v)
        monkeypatch.setitem(sys.modules, name, m)
        return m
    for pkg in ("detr_od", "detr_od.models", "detr_od.models.dense_heads", "detr_ssod", "detr_ssod.models"):
        mod(pkg)
    old = lambda *a, **k: "reference"  # noqa: E731
    comp = mod("detr_od.models.dense_heads.dn_components", prepare_for_cdn=old, prepare_for_cdn_plus=old)
    head = mod("detr_od.models.dense_heads.dino_detr_head", prepare_for_cdn=old)
    ssod_head = mod("detr_od.models.dense_heads.dino_detr_ssod_head", prepare_for_cdn_plus=old)
    det = mod("detr_ssod.models.dino_detr_ssod", DinoDetrSSOD=type("DinoDetrSSOD", (), {"prepare_unsup_cdn": old}))
    done, skipped = registry.bind_dn_queries()
    assert skipped == [] and done == ["prepare_for_cdn", "prepare_for_cdn_plus", "DinoDetrSSOD.prepare_unsup_cdn"]
    assert head.prepare_for_cdn is s.prepare_for_cdn and comp.prepare_for_cdn is s.prepare_for_cdn
    assert ssod_head.prepare_for_cdn_plus is s.prepare_for_cdn_plus and comp.prepare_for_cdn_plus is s.prepare_for_cdn_plus
    assert det.DinoDetrSSOD.prepare_unsup_cdn is s.prepare_unsup_cdn
    assert s.prepare_for_cdn(None, False, 900, 80, 256, None) == (None, None, None, None)
    assert s.prepare_for_cdn_plus(None, False, 900, 80, 256, None) == (None, None, None, None)


def _good_build():
    from semi_detr_amd import dn_query as d
    p = d._Build()
    p.dn = d.make_layout([3, 1], 3, 4)
    p.src_counts[0], p.src_counts[1] = 3, 1
    for b in range(2):
        p.labels[b], p.boxes[b] = 4096, 4096           # never dereferenced: every call below fails its host-side checks
    p.box_stride, p.num_known = 4, 16
    p.label_weight, p.num_embeddings, p.hidden_dim, p.num_classes, p.num_queries = 4096, 81, 32, 80, 30
    p.noise = 4096
    p.query_label = p.query_bbox = p.known_bid = p.map_known_indice = p.noised_labels = 4096
    return p


def test_c_abi_argument_checks_need_no_gpu():
    from semi_detr_amd import _lib
    from semi_detr_amd import dn_query as d
    lib = _lib.lib()
    bad = lambda p: lib.semidetr_dn_build_f32(None, ctypes.byref(p))  # noqa: E731
    assert lib.semidetr_dn_build_f32(None, None) == -1 and b"null pointer" in lib.semidetr_last_error()
    for field in ("label_weight", "noise", "query_label", "query_bbox", "known_bid", "map_known_indice", "noised_labels"):
        p = _good_build()
        setattr(p, field, None)
        assert bad(p) == -1 and b"null pointer" in lib.semidetr_last_error(), field
    p = _good_build()
    p.num_known = 15                                    # K inconsistent with the offsets
    assert bad(p) == -1 and b"inconsistent with the offsets" in lib.semidetr_last_error()
    p = _good_build()
    p.dn.num_images = 65                                # B over the cap
    assert bad(p) == -1 and b"65 images" in lib.semidetr_last_error()
    p = _good_build()
    p.dn.groups = 3                                     # positive + negative halves
    p.num_known = 12
    assert bad(p) == -1 and b"even" in lib.semidetr_last_error()
    p = _good_build()
    p.dn.offsets[1] = 4                                 # more rows than single_pad
    assert bad(p) == -1 and b"single_pad" in lib.semidetr_last_error()
    p = _good_build()
    p.src_counts[1] = 0                                 # a stand-in image needs its noise value
    assert bad(p) == -1 and b"image_noise" in lib.semidetr_last_error()
    p = _good_build()
    p.query_bbox = 4100
    assert bad(p) == -1 and b"aligned" in lib.semidetr_last_error()
    p = _good_build()
    p.cons_rows = 4096                                  # rows without a layout / destination
    assert bad(p) == -1
    with pytest.raises(ValueError, match="at most 64"):
        d.make_layout([1] * 65, 1, 2)
    c = d._Consistency()
    assert lib.semidetr_dn_consistency_f32(None, None) == -1
    c.cons = d.make_layout([2], 2, 5)
    c.num_known = 9
    assert lib.semidetr_dn_consistency_f32(None, ctypes.byref(c)) == -1 and b"inconsistent" in lib.semidetr_last_error()
    c.num_known = 10
    assert lib.semidetr_dn_consistency_f32(None, ctypes.byref(c)) == -1 and b"null pointer" in lib.semidetr_last_error()
    P = ctypes.c_void_p
    assert lib.semidetr_dn_label_backward_f32(None, None, P(1), P(1), P(1), 4, 1, 4, 32, 81, P(1)) == -1
    assert lib.semidetr_dn_label_backward_f32(None, P(1), P(1), P(1), P(1), 0, 1, 4, 32, 81, P(1)) == -1
    lay = d.make_layout([2], 2, 5)
    assert lib.semidetr_dn_gather_rows_f32(None, ctypes.byref(lay), None, 32, P(1)) == -1
    lay.groups = 0
    assert lib.semidetr_dn_gather_rows_f32(None, ctypes.byref(lay), P(1), 32, P(1)) == -1


def test_cpu_tensors_have_no_fallback():
    import semi_detr_amd as s
    enc = torch.nn.Embedding(81, 32)
    t = {"labels": [torch.zeros(2, dtype=torch.long)], "boxes": [torch.full((2, 4), 0.5)]}
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        s.prepare_for_cdn((t, 100, 0.5, 1.0), True, 30, 80, 32, enc)
    with pytest.raises(TypeError, match="nn.Embedding"):
        s.prepare_for_cdn((t, 100, 0.5, 1.0), True, 30, 80, 32, lambda x: x)


def test_dn_kernels_use_no_scratch_and_no_float_atomics():
    from test_cabi_host import ROOT, _code_object_kernels
    meta = _code_object_kernels(os.path.join(ROOT, "semi-detr_amd", "csrc", "libsemidetr_hip.so"))
    dn = {n: k for n, k in meta.items() if n.startswith("dn_")}
    assert sorted(dn) == ["dn_build_kernel", "dn_consistency_kernel", "dn_gather_rows_kernel", "dn_label_bwd_kernel"]
    for n, k in dn.items():
        assert not k[".vgpr_spill_count"] and not k[".sgpr_spill_count"] and not k[".private_segment_fixed_size"], n
    src = open(os.path.join(ROOT, "semi-detr_amd", "csrc", "dn_query.hip")).read()
    assert "atomic" not in src.replace("float atomics", "")
