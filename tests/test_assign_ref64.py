"""The fp64 statements and admissibility checkers of tests/assign_ref64.py, checked without a GPU:
  * satisfiable: the C oracle's result on every case of tests/assign_cases.py (the cases of test_gpu_assign_admissible.py)
    and every reference fixture under tests/golden is admissible;
  * they bite: every listed mutant of the statement, or of the oracle's output, is rejected, and the rejecting case is named;
  * not vacuous: on the ordinary cases the share of decisions that may go either way is at most 1 %, from inputs alone."""
import numpy as np
import pytest

import assign_cases as ac
import assign_ref64 as ar
import oracle

_npz, h_inputs, o_inputs = ac.golden, ac.h_inputs, ac.o_inputs


def oracle_hungarian(p):
    gi, lab, _, _ = oracle.hungarian_assign(p["bbox_pred"], p["cls"], p["gt_bboxes"], p["gt_labels"], p["img_w"], p["img_h"])
    cost = None
    if len(p["gt_labels"]):
        cost = oracle.match_cost(p["bbox_pred"], p["cls"], p["gt_bboxes"], p["gt_labels"], p["img_w"], p["img_h"])
    return gi, lab, cost


def oracle_o2m(p, topk, dyn, alpha=1.0, beta=6.0):
    C = p["cls"].shape[1]
    gi, lab, mo, am = oracle.o2m_assign(p["bbox_pred"], p["cls"], p["gt_bboxes"], p["gt_labels"], p["img_w"], p["img_h"],
                                        topk=topk, alpha=alpha, beta=beta, dynamic_k=dyn)
    lf, bt, nm = oracle.o2m_targets(gi, mo, am, p["gt_bboxes"], p["gt_labels"], p["img_w"], p["img_h"], C)
    return dict(gt_inds=gi.copy(), labels=lab.copy(), max_overlaps=mo.copy(), assign_metrics=am.copy(), labels_full=lf,
                bbox_targets=bt, norm_metrics=nm)


def oracle_nms(nb, b):
    h, w = nb["shapes"][b]
    return oracle.pseudo_nms(nb["logits"][b], nb["bbox"][b], h, w, score_thr=nb["score_thr"], iou_thr=nb["iou_thr"],
                             max_num=nb["max_per_img"])


def check_nms(nb, b, dets, labels, **kw):
    h, w = nb["shapes"][b]
    return ar.check_nms(nb["logits"][b], nb["bbox"][b], h, w, dets, labels, score_thr=nb["score_thr"], iou_thr=nb["iou_thr"],
                        max_per_img=nb["max_per_img"], iou_exact=nb["iou_exact"], **kw)


# ----------------------------------------------------------------------------------------------------------------------
# satisfiable
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("batch", ac.hungarian_batches(), ids=lambda b: b["name"])
def test_oracle_hungarian_admissible(batch):
    for p in batch["problems"]:
        gi, lab, cost = oracle_hungarian(p)
        try:
            ar.check_hungarian(h_inputs(p), gi, lab, cost, num_pos=int((gi > 0).sum()))
        except ar.Inadmissible as e:
            raise AssertionError(f"{batch['name']} / {p['name']}: {e}") from None


def test_oracle_cost_parts_admissible_both_pred_contracts():
    """cls / reg / iou one by one (the calls of dino_detr_ssod.py:265-271), 'xywh' and 'xyxy' L1, 'iou' and 'giou', and the
    pred_xyxy contract: the statement given x1 y1 x2 y2 must agree with the one given cxcywh up to both bounds."""
    for p in ac.ordinary_hungarian()[:3] + ac.adversarial_problems(48, 8, "logit", 1):
        if not len(p["gt_labels"]):
            continue
        for fmt, mode in (("xywh", "giou"), ("xyxy", "iou")):
            ref = ar.match_cost(**h_inputs(p), box_format=fmt, iou_mode=mode)
            parts = oracle.match_cost(p["bbox_pred"], p["cls"], p["gt_bboxes"], p["gt_labels"], p["img_w"], p["img_h"],
                                      box_format=fmt, iou_mode=mode, parts=True)
            for key, got in zip(("cost", "cls", "reg", "iou"), parts):
                ar._within(f"{p['name']} {fmt} {mode} {key}", got, ref[key])
        b = p["bbox_pred"].astype(np.float32)
        xyxy = np.concatenate([b[:, :2] - np.float32(0.5) * b[:, 2:], b[:, :2] + np.float32(0.5) * b[:, 2:]], -1)
        f = np.asarray([p["img_w"], p["img_h"]] * 2, np.float32)
        a = ar.match_cost(xyxy * f, p["cls"], p["gt_bboxes"], p["gt_labels"], 1.0, 1.0, pred_xyxy=True)["iou"]
        c = ar.match_cost(**h_inputs(p))["iou"]
        assert np.all(~(np.abs(a[0] - c[0]) > ar.bound(a) + ar.bound(c))), p["name"]


def test_cost_fixtures_admissible():
    for name, g in _npz("cost.npz").items():
        if "bbox_pred" not in g or not len(g["gt_labels"]):
            continue
        w, h = (float(v) for v in g["img_wh"])
        inputs = dict(bbox_pred=g["bbox_pred"], cls_pred=g["cls_pred"], gt_bboxes=g["gt_bboxes"], gt_labels=g["gt_labels"],
                      img_w=w, img_h=h)
        ref = ar.match_cost(**inputs)
        for key in ("cls", "reg", "iou"):
            if f"cost_{key}" in g:                          # the two largest fixtures hold the total only
                ar._within(f"{name} cost_{key}", g[f"cost_{key}"], ref[key])
        ar.check_hungarian(inputs, g["assigned_gt_inds"], g["assigned_labels"], g["cost"], ref=ref)


@pytest.mark.parametrize("batch", ac.o2m_batches(), ids=lambda b: b["name"])
def test_oracle_o2m_admissible(batch):
    for p in batch["problems"]:
        for mode, topk, dyn in batch["modes"]:
            try:
                ar.check_o2m(o_inputs(p), oracle_o2m(p, topk, dyn), p["cls"].shape[1], topk, dyn)
            except ar.Inadmissible as e:
                raise AssertionError(f"{batch['name']} / {p['name']} / {mode}: {e}") from None


def test_o2m_fixtures_admissible():
    for name, g in _npz("o2m.npz").items():
        ih, iw = (float(v) for v in g["img_hw"])
        inputs = dict(bbox_pred=g["bbox_pred"], cls_prob=g["cls_prob"], gt_bboxes=g["gt_bboxes"], gt_labels=g["gt_labels"],
                      img_w=iw, img_h=ih)
        C = g["cls_prob"].shape[1]
        for tag, topk, dyn in (("", 13, False), ("t1_", 1, False), ("tk_", 13, True)):
            res = {k: g[tag + k] for k in ("gt_inds", "labels", "max_overlaps", "assign_metrics")}
            if not tag:
                res.update({k: g[k] for k in ("labels_full", "bbox_targets", "norm_metrics")})
            try:
                ar.check_o2m(inputs, res, C, topk, dyn)
            except ar.Inadmissible as e:
                raise AssertionError(f"o2m.npz {name} {tag}: {e}") from None


@pytest.mark.parametrize("nb", ac.nms_batches(), ids=lambda b: b["name"])
def test_oracle_nms_and_filter_admissible(nb):
    for b in range(len(nb["shapes"])):
        dets, labels = oracle_nms(nb, b)
        try:
            check_nms(nb, b, dets, labels)
            keep, thr = oracle.pseudo_label_filter(dets)
            ar.check_pseudo_filter(dets, labels, dets[keep, :4], labels[keep], dets[keep, 4], thr)
        except ar.Inadmissible as e:
            raise AssertionError(f"{nb['names'][b]}: {e}") from None


def test_nms_pseudo_transform_fixtures_admissible():
    for name, g in _npz("nms.npz").items():
        ar.check_nms(g["logits"], g["bbox_pred"], float(g["img_hw"][0]), float(g["img_hw"][1]), g["dets"], g["labels"],
                     max_per_img=int(g["max_per_img"]))
    for name, g in _npz("pseudo.npz").items():
        k = g["keep"]
        ar.check_pseudo_filter(g["proposal"], g["labels"], g["proposal"][k, :4], g["labels"][k], g["proposal"][k, 4],
                               g["thr"] if len(g["proposal"]) else None)
    for name, g in _npz("transform.npz").items():
        if len(g["boxes"]):
            ar.check_transform(g["boxes"][:, :4], g["M"], float(g["out_shape"][0]), float(g["out_shape"][1]), g["out"])


def test_oracle_filter_and_transform_cases_admissible():
    for name, _, prop, labels in ac.filter_cases():
        keep, thr = oracle.pseudo_label_filter(prop)
        st = ar.check_pseudo_filter(prop, labels, prop[keep, :4], labels[keep], prop[keep, 4], thr if len(prop) else None)
        if name in ("K1", "K0"):
            assert st["kept"] == 0 and (name == "K0" or np.isnan(thr))
    for name, boxes, M, (h, w) in ac.transform_cases():
        ar.check_transform(boxes, M, h, w, oracle.transform_bboxes(boxes, M, h, w))


def test_iou_at_threshold_case_is_exact_in_fp32():
    """The premise of iou_exact: the case's IoU is 0.5 in fp32 arithmetic as in fp64, and the oracle keeps both boxes."""
    nb = [b for b in ac.nms_batches() if b["name"] == "iou_at_threshold_exact"][0]
    f = np.float32
    a, b = np.asarray([0, 0, 64, 64], f), np.asarray([0, 0, 64, 32], f)
    inter = (min(a[2], b[2]) - max(a[0], b[0])) * (min(a[3], b[3]) - max(a[1], b[1]))
    iou32 = inter / ((a[2] - a[0]) * (a[3] - a[1]) + (b[2] - b[0]) * (b[3] - b[1]) - inter)
    assert iou32.dtype == np.float32 and iou32 == f(0.5) == f(nb["iou_thr"])
    s, box, _ = ar.nms_quantities(nb["logits"][0], nb["bbox"][0], 128, 128)
    assert [float(c[0][0]) for c in box] == [0, 0, 64, 64] and [float(c[0][1]) for c in box] == [0, 0, 64, 32]
    dets, labels = oracle_nms(nb, 0)
    assert len(dets) == 3


# ----------------------------------------------------------------------------------------------------------------------
# the checkers bite
# ----------------------------------------------------------------------------------------------------------------------
def _first_rejecting(cases, run):
    for name, case in cases:
        try:
            run(case)
        except ar.Inadmissible as e:
            return name, str(e)
    return None, None


def _small_hungarian():
    ordinary = [(p["name"], p) for p in ac.ordinary_hungarian() if 0 < len(p["gt_labels"]) <= 15][:4]
    adv = [(p["name"], p) for p in ac.adversarial_problems(48, 8, "logit", 1)]
    return ordinary, adv


# eps is inert at ordinary logits (its relative effect on 1 - p + eps is 1e-12 / (1 - p), below u for |x| < 16), and the clamp of
# the enclosing area only acts when prediction and gt are the same point: those two mutants are rejected on the adversarial
# cases that reach them; every other one on an ordinary random case.
@pytest.mark.parametrize("mutant,pool", [("no_eps", "adversarial"), ("iou_not_giou", "ordinary"), ("earea_noclamp", "adversarial"),
                                         ("l1_unnormalised", "ordinary"), ("alpha_swapped", "ordinary"), ("fp16", "ordinary")])
def test_hungarian_mutants_rejected(mutant, pool):
    ordinary, adv = _small_hungarian()

    def run(p):
        gi, lab, cost = oracle_hungarian(p)
        if mutant == "fp16":
            ar.check_hungarian(h_inputs(p), gi, lab, cost.astype(np.float16).astype(np.float32))
        else:
            ar.check_hungarian(h_inputs(p), gi, lab, cost, mutant=mutant)
    name, why = _first_rejecting(ordinary if pool == "ordinary" else adv, run)
    assert name is not None, f"mutant {mutant} is not rejected on any {pool} case"
    print(f"mutant {mutant}: rejected on {name}: {why[:120]}")


@pytest.mark.parametrize("how", ["statement", "output"])
def test_o2m_metric_filter_dropped_rejected_where_topk_takes_every_query(how):
    """`metric > 0` of the static modes (o2m_assigner.py:135) carries no allowance: a surely disjoint pair has metric (0, 0).  At
    Q = k = 13 the top-k takes every query, so only the filter keeps the disjoint ones in the background.  Dropped from the
    statement, the oracle's backgrounds become certain bidders; dropped from the output (every zero-metric background query made
    positive for a gt, with IoU and metric 0, what a kernel with `>= 0` returns), they are no possible bidders."""
    rejected = []
    for p in ac.adversarial_problems(13, 4, "prob", 3):
        res = oracle_o2m(p, 13, False)
        C = p["cls"].shape[1]
        for k in ("labels_full", "bbox_targets", "norm_metrics"):
            res.pop(k)
        try:
            if how == "statement":
                ar.check_o2m(o_inputs(p), res, C, 13, False, mutant="metric_filter_dropped")
            else:
                m = ar.o2m(**o_inputs(p))["met"][0]
                zero = np.nonzero((res["gt_inds"] == 0) & (m == 0).any(1))[0]
                if not len(zero):
                    continue
                for q in zero:
                    g = int(np.nonzero(m[q] == 0)[0][0])
                    res["gt_inds"][q], res["labels"][q] = g + 1, p["gt_labels"][g]
                    res["max_overlaps"][q], res["assign_metrics"][q] = 0.0, 0.0
                ar.check_o2m(o_inputs(p), res, C, 13, False)
        except ar.Inadmissible as e:
            rejected.append(p["name"])
            why = str(e)
    print(f"mutant metric_filter_dropped ({how}): rejected on {rejected}: {why[:120]}")
    # (dup_predictions and all_equal have no surely disjoint background query: nothing there for the filter to decide)
    assert "G1" in rejected and "G_eq_Q" in rejected and len(rejected) >= 12, rejected


@pytest.mark.parametrize("mutant", ["topk_plus", "topk_minus", "exponents_swapped", "ties_to_smaller_iou", "dynamic_k_rounded"])
def test_o2m_mutants_rejected(mutant):
    cases = [(p["name"], p) for p in (ac._o2m_random(107, 900, 80, 7), ac._o2m_random(130, 900, 80, 30))]
    dyn = mutant == "dynamic_k_rounded"

    def run(p):
        res = oracle_o2m(p, 13, dyn)
        C = p["cls"].shape[1]
        if mutant != "ties_to_smaller_iou":
            return ar.check_o2m(o_inputs(p), res, C, 13, dyn, mutant=mutant)
        d = ar.o2m_decisions(o_inputs(p), 13, dyn)
        multi = np.nonzero(d["certain"].sum(1) > 1)[0]
        if not len(multi):                                # no query bids for two gts in this case
            return
        for q in multi:
            g = int(np.argmin(np.where(d["certain"][q], d["iou"][0][q], np.inf)))
            res["gt_inds"][q], res["labels"][q] = g + 1, p["gt_labels"][g]
            res["max_overlaps"][q], res["assign_metrics"][q] = d["iou"][0][q, g], d["met"][0][q, g]
        for k in ("labels_full", "bbox_targets", "norm_metrics"):
            res.pop(k)
        ar.check_o2m(o_inputs(p), res, C, 13, dyn)
    name, why = _first_rejecting(cases, run)
    assert name is not None, f"mutant {mutant} is not rejected"
    print(f"mutant {mutant}: rejected on {name}: {why[:120]}")


@pytest.mark.parametrize("mutant", ["class_agnostic", "suppress_ge", "kept_dropped", "below_threshold_kept", "max_per_img_wrong_end"])
def test_nms_mutants_rejected(mutant):
    lg, bx, shapes = ac.nms_random_batch(3, 2, 200, 6, -1.0)
    nb = ac._nms("random_2x200x6", True, lg, bx, shapes, max_per_img=50)
    if mutant == "suppress_ge":
        nb = [b for b in ac.nms_batches() if b["name"] == "iou_at_threshold_exact"][0]

    def run(b):
        dets, labels = oracle_nms(nb, b)
        if mutant == "class_agnostic":
            return check_nms(nb, b, dets, labels, mutant=mutant)
        if mutant == "suppress_ge":                       # what a kernel with `>=` returns: the lower-scored box is gone
            dets, labels = np.delete(dets, 1, 0), np.delete(labels, 1)
        elif mutant == "kept_dropped":
            dets, labels = np.delete(dets, 3, 0), np.delete(labels, 3)
        elif mutant == "below_threshold_kept":
            h, w = nb["shapes"][b]
            full = oracle.pseudo_nms(nb["logits"][b], nb["bbox"][b], h, w, score_thr=0.001, max_num=2048)
            i = int(np.nonzero(full[0][:, 4] < 0.009)[0][0])
            dets, labels = oracle.pseudo_nms(nb["logits"][b], nb["bbox"][b], h, w, max_num=2048)
            dets, labels = np.concatenate([dets, full[0][i:i + 1]]), np.concatenate([labels, full[1][i:i + 1]])
            return ar.check_nms(nb["logits"][b], nb["bbox"][b], h, w, dets, labels, max_per_img=2048)
        elif mutant == "max_per_img_wrong_end":
            h, w = nb["shapes"][b]
            dets, labels = oracle.pseudo_nms(nb["logits"][b], nb["bbox"][b], h, w, max_num=2048)
            assert len(dets) > 50
            dets, labels = dets[-50:], labels[-50:]
        check_nms(nb, b, dets, labels)
    name, why = _first_rejecting([(nb["names"][b], b) for b in range(len(nb["shapes"]))], run)
    assert name is not None, f"mutant {mutant} is not rejected"
    print(f"mutant {mutant}: rejected on {name}: {why[:120]}")


def test_filter_and_transform_mutants_rejected():
    cases = [(n, (p, l)) for n, o, p, l in ac.filter_cases() if o]

    def run(c):
        prop, labels = c
        keep, thr = oracle.pseudo_label_filter(prop)
        ar.check_pseudo_filter(prop, labels, prop[keep, :4], labels[keep], prop[keep, 4], thr, mutant="population_std")
    name, why = _first_rejecting(cases, run)
    assert name is not None, "population std is not rejected"
    print(f"mutant population_std: rejected on {name}: {why[:120]}")
    name, why = _first_rejecting([(n, (b, M, hw)) for n, b, M, hw in ac.transform_cases()],
                                 lambda c: ar.check_transform(c[0], c[1], *c[2], oracle.transform_bboxes(c[0], c[1], *c[2]),
                                                              mutant="two_corners"))
    assert name is not None, "two-corner warp is not rejected"
    print(f"mutant two_corners: rejected on {name}: {why[:120]}")


# ----------------------------------------------------------------------------------------------------------------------
# not vacuous
# ----------------------------------------------------------------------------------------------------------------------
def test_ordinary_cases_leave_at_most_one_percent_open():
    """From inputs and bounds alone, no kernel involved.  Hungarian: the allowance on the fp64 optimum against the gap to the
    second-best assignment (small problems: one re-solve per optimal pair)."""
    worst = {}
    for p in ac.ordinary_hungarian():
        if 0 < len(p["gt_labels"]) <= 15:
            allow, gap = ar.hungarian_ambiguity(h_inputs(p))
            worst["hungarian"] = max(worst.get("hungarian", 0.0), allow / gap)
            assert allow <= 0.01 * gap, (p["name"], allow, gap)
    for batch in ac.o2m_batches():
        if batch["ordinary"]:
            for p in batch["problems"]:
                for mode, topk, dyn in batch["modes"]:
                    if len(p["gt_labels"]):
                        share = ar.o2m_ambiguity(o_inputs(p), topk, dyn)
                        worst["o2m"] = max(worst.get("o2m", 0.0), share)
                        assert share <= 0.01, (p["name"], mode, share)
    for nb in ac.nms_batches():
        if nb["ordinary"]:
            for b, (h, w) in enumerate(nb["shapes"]):
                share = ar.nms_ambiguity(nb["logits"][b], nb["bbox"][b], h, w, nb["score_thr"], nb["iou_thr"])
                worst["nms"] = max(worst.get("nms", 0.0), share)
                assert share <= 0.01, (nb["names"][b], share)
    for name, ordinary, prop, _ in ac.filter_cases():
        if ordinary:
            share = ar.pseudo_ambiguity(prop)
            worst["filter"] = max(worst.get("filter", 0.0), share)
            assert share <= 0.01, (name, share)
    print("worst open share per family:", {k: f"{v:.2e}" for k, v in worst.items()})
