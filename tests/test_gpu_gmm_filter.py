"""The cost-GMM double filter on the MI355X (csrc/gmm_filter.hip) against the reference's fixtures (tests/golden/gmm.npz) and
the fp64 restatement (tests/gmm_ref64.py)."""
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN
from gmm_ref64 import double_filter_sets, fit_gmm_ref64

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
Z = np.load(os.path.join(GOLDEN, "gmm.npz"))
FIT_NAMES = [str(n) for n in Z["fit_names"]]
LISTS = ("gt_bboxes_list", "gt_labels_list", "gt_scores_list", "unsup_bboxes_gmm_list", "unsup_labels_gmm_list",
         "unsup_scores_gmm_list", "det_bboxes_gmm_list", "det_labels_gmm_list", "det_scores_gmm_list")


def _case(name):
    return {k.split(".", 2)[2]: Z[k] for k in Z.files if k.startswith(f"fit.{name}.")}


def _assigner():
    import semi_detr_amd as s
    return s.HungarianAssigner(cls_cost=dict(type="FocalLossCost", weight=2.0),
                               reg_cost=dict(type="BBoxL1Cost", weight=5.0, box_format="xywh"),
                               iou_cost=dict(type="IoUCost", iou_mode="giou", weight=2.0))


def _sorted_details(costs, det):
    order = np.argsort(costs, kind="stable")
    return det["labels"].cpu().numpy()[order], det["scores"].cpu().numpy()[order]


@pytest.mark.parametrize("name", FIT_NAMES)
def test_fit_reproduces_reference_fixture(name):
    import semi_detr_amd as s
    c = _case(name)
    thr, det = s.fit_gmm_threshold(torch.from_numpy(c["costs"]).to(DEV), max_iter=int(c["max_iter"]), return_details=True)
    assert thr.shape == (1,) and thr.dtype == torch.float32
    assert thr.cpu().numpy()[0].tobytes() == np.float32(c["thr"]).tobytes(), (thr.item(), c["thr"])
    if "labels" in c:
        lab, sc = _sorted_details(c["costs"], det)
        np.testing.assert_array_equal(lab, c["labels"])
        assert int(det["n_iter"]) == int(c["n_iter"]) and bool(det["converged"]) == bool(c["converged"])
        np.testing.assert_allclose(sc, c["scores"], rtol=1e-10, atol=1e-12)


def test_fit_agrees_with_ref64_on_random_sets():
    import semi_detr_amd as s
    rng = np.random.default_rng(5)
    near_ties = 0
    for t in range(300):
        n = int(rng.integers(2, 2500 if t % 10 == 0 else 400))
        k = t % 3
        c = (np.concatenate([rng.normal(1, 0.3, n), rng.normal(4, 1, n // 3)]) if k == 0 else
             rng.gamma(1.5, 1.0, n) * 3 if k == 1 else rng.normal(5, 0.5, n)).astype(np.float32)
        r = fit_gmm_ref64(c)
        thr, det = s.fit_gmm_threshold(torch.from_numpy(c).to(DEV), return_details=True)
        lab, sc = _sorted_details(c, det)
        same = (thr.item() == r["thr"] and np.array_equal(lab, r["labels"]) and int(det["n_iter"]) == r["n_iter"])
        if not same:
            assert r["margin"] < 1e-9, (t, n, thr.item(), r["thr"], r["margin"])
            near_ties += 1
            continue
        np.testing.assert_allclose(sc, r["scores"], rtol=1e-10, atol=1e-12)      # atol: scores that cross zero
    print(f"random GMM fits: {near_ties} of 300 differ on a deciding margin < 1e-9")


def test_segment_buffer_equals_concatenation():
    import semi_detr_amd as s
    rng = np.random.default_rng(9)
    parts = [rng.normal(1, 0.3, 40), rng.normal(4, 1, 0), rng.normal(3.5, 0.8, 25)]
    parts[1] = rng.normal(2, 1, 13)
    cap = 48
    buf = np.full((3, cap), np.nan, np.float32)           # padding must never be read
    for i, p in enumerate(parts):
        buf[i, :len(p)] = p
    counts = torch.tensor([len(p) for p in parts], dtype=torch.int32, device=DEV)
    thr_s, det_s = s.fit_gmm_threshold_segments(torch.from_numpy(buf).to(DEV), counts, return_details=True)
    cat = np.concatenate(parts).astype(np.float32)
    thr_c, det_c = s.fit_gmm_threshold(torch.from_numpy(cat).to(DEV), return_details=True)
    assert thr_s.item() == thr_c.item() == fit_gmm_ref64(cat)["thr"]
    n = cat.size
    assert torch.equal(det_s["labels"][:n], det_c["labels"]) and int(det_s["n_iter"]) == int(det_c["n_iter"])
    np.testing.assert_allclose(det_s["scores"][:n].cpu().numpy(), det_c["scores"].cpu().numpy(), rtol=1e-12)


def _split(flat, counts):
    out, o = [], 0
    for c in counts:
        out.append(flat[o:o + c])
        o += c
    return out


def test_unsup_gmm_filter_end_to_end_fixture():
    import semi_detr_amd as s
    counts = [int(c) for c in Z["e2e.counts"]]
    g = {k: [torch.from_numpy(np.ascontiguousarray(a)).to(DEV) for a in _split(Z[f"e2e.{k}"], counts)]
         for k in ("gt_bboxes", "gt_labels", "gt_scores", "det_bboxes", "det_labels", "det_scores")}
    metas = [dict(img_shape=(int(h), int(w), 3)) for h, w in Z["e2e.img_hw"]]
    res = s.unsup_gmm_filter(torch.from_numpy(Z["e2e.cls"]).to(DEV), torch.from_numpy(Z["e2e.bbox"]).to(DEV),
                             g["gt_bboxes"], g["gt_labels"], g["gt_scores"], g["det_bboxes"], g["det_labels"],
                             g["det_scores"], metas, _assigner())
    np.testing.assert_array_equal([len(v) for v in res.match_gt_inds_list], Z["e2e.match_counts"])
    np.testing.assert_array_equal(torch.cat(res.match_gt_inds_list).cpu().numpy(), Z["e2e.match_inds"])
    np.testing.assert_allclose(torch.cat(res.match_gt_cost_list).cpu().numpy(), Z["e2e.match_cost"], rtol=1e-5, atol=1e-5)
    np.testing.assert_allclose(res.thr.cpu().numpy(), Z["e2e.thr"], rtol=1e-5, atol=1e-5)
    for k, lst in zip(LISTS, res[:9]):
        np.testing.assert_array_equal([len(v) for v in lst], Z[f"e2e.{k}.counts"], err_msg=k)
        assert torch.cat(lst).cpu().numpy().tobytes() == Z[f"e2e.{k}"].tobytes(), k


def _bench_inputs(seed=0, B=4, Q=900, C=80):
    g = torch.Generator().manual_seed(seed)
    hw = [(800, 1333), (800, 1200), (750, 1333), (800, 1066)][:B]
    G = [300, 0, 57, 181][:B]
    cls = torch.randn(B, Q, C, generator=g) * 2
    bbox = torch.cat([torch.rand(B, Q, 2, generator=g), torch.rand(B, Q, 2, generator=g) * 0.3 + 0.02], -1)
    gts, labs, scores, dets = [], [], [], []
    for b in range(B):
        h, w = hw[b]
        xy = torch.rand(G[b], 2, generator=g) * torch.tensor([w * 0.8, h * 0.8])
        box = torch.cat([xy, xy + torch.rand(G[b], 2, generator=g) * 200 + 8], -1)
        gts.append(torch.cat([box, torch.rand(G[b], 1, generator=g)], -1))        # (G, 5): the filter takes [:, :4]
        labs.append(torch.randint(0, C, (G[b],), generator=g))
        scores.append(torch.rand(G[b], generator=g))
        dets.append(box + torch.randn(G[b], 4, generator=g))
    metas = [dict(img_shape=(h, w, 3)) for h, w in hw]
    to = lambda ts: [t.to(DEV) for t in ts]  # noqa: E731
    return cls.to(DEV), bbox.to(DEV), to(gts), to(labs), to(scores), to(dets), metas


def _host_composition(cls, bbox, gts, labs, scores, dets, metas, base_thr=0.4):
    """assign_batch(return_cost=True), per-image .cpu(), gmm_ref64 and torch set logic."""
    _, costs, res = _assigner().assign_batch(bbox, cls, [t[:, :4] for t in gts], labs, metas, return_cost=True)
    po = res["pair_offsets"]
    rows, cols = res["rows"].cpu(), res["cols"].cpu()
    mc, mi = [], []
    for b in range(len(gts)):
        cb = costs[b].cpu()
        r, c = rows[po[b]:po[b + 1]], cols[po[b]:po[b + 1]]
        mc.append(cb[r, c])
        mi.append(c)
    thr = fit_gmm_ref64(torch.cat(mc).numpy())["thr"]
    out = {k: [] for k in LISTS}
    for b in range(len(gts)):
        base, union = (torch.from_numpy(i) for i in double_filter_sets(mc[b].numpy(), mi[b].numpy(),
                                                                         scores[b].cpu().numpy(), thr, base_thr))
        gb, gl, gs = gts[b].cpu()[:, :4], labs[b].cpu(), scores[b].cpu()
        db, dl, ds = dets[b].cpu()[:, :4], labs[b].cpu(), scores[b].cpu()
        for k, v in zip(LISTS, (gb[base], gl[base], gs[base], gb[union], gl[union], gs[union], db[union], dl[union],
                                ds[union])):
            out[k].append(v)
    return out, thr, mc, mi


def test_unsup_gmm_filter_bench_shape_matches_host_composition():
    import semi_detr_amd as s
    cls, bbox, gts, labs, scores, dets, metas = _bench_inputs()
    want, thr, mc, mi = _host_composition(cls, bbox, gts, labs, scores, dets, metas)
    res = s.unsup_gmm_filter(cls, bbox, gts, labs, scores, dets, labs, scores, metas, _assigner())
    assert res.thr.item() == thr
    for b in range(len(gts)):
        assert torch.equal(res.match_gt_cost_list[b].cpu(), mc[b]) and torch.equal(res.match_gt_inds_list[b].cpu(), mi[b])
    for i, k in enumerate(LISTS):
        for b in range(len(gts)):
            got = res[i][b].cpu()
            assert got.shape == want[k][b].shape and got.dtype == want[k][b].dtype, (k, b)
            assert got.numpy().tobytes() == want[k][b].numpy().tobytes(), (k, b)
    assert len(res.gt_bboxes_list[1]) == 0 and len(res.unsup_bboxes_gmm_list[1]) == 0


def test_unsup_gmm_filter_pending_has_no_host_sync():
    import semi_detr_amd as s
    cls, bbox, gts, labs, scores, dets, metas = _bench_inputs(seed=1)
    asg = _assigner()
    want = s.unsup_gmm_filter(cls, bbox, gts, labs, scores, dets, labs, scores, metas, asg)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        pending = s.unsup_gmm_filter(cls, bbox, gts, labs, scores, dets, labs, scores, metas, asg, wait=False)
    finally:
        torch.cuda.set_sync_debug_mode(0)
    got = pending.result()
    assert torch.equal(got.thr, want.thr)
    for a, b in zip(got[:9], want[:9]):
        assert all(torch.equal(x, y) for x, y in zip(a, b))


def test_fit_gmm_method_binding():
    import types
    import semi_detr_amd as s
    c = _case("bimodal")
    self = types.SimpleNamespace(covariance_type="diag")
    cost_ = torch.from_numpy(c["costs"])                 # the call site's gathered costs are on the CPU
    thr_ = cost_.new_tensor(s.fit_gmm(self, cost_).cpu())
    assert thr_.numpy().tobytes() == np.float32(c["thr"]).reshape(1).tobytes()
