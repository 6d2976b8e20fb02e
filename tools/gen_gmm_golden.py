#!/usr/bin/env python
"""Generate tests/golden/gmm.npz from the REFERENCE's own ``DinoDetrSSOD._fit_gmm`` and ``DinoDetrSSOD.unsup_loss``
(detr_ssod/models/dino_detr_ssod.py:832-890, :203-353), imported by path through ``oracle/gen_golden.load_dino_detr_ssod``.
Runs only where the reference tree, scikit-learn and scipy are installed; the fixtures it writes are data.

    python tools/gen_gmm_golden.py

* ``fit.<case>.*``: ``_fit_gmm`` called unbound on a stand-in ``self`` (covariance_type 'diag') -> ``thr``; a parallel
  ``GaussianMixture`` with the same arguments -> ``labels`` / ``scores`` (for the SORTED costs), ``n_iter``, ``converged``.
  ``maxiter2`` is the one case the reference cannot produce (its fit always allows 100 iterations, and no natural cost set
  found by a seed search runs out of them): sklearn with ``max_iter=2``, the threshold by ``_fit_gmm``'s pick rule.
* ``e2e.*``: ``unsup_loss`` itself, driven unbound on three small seeded images with the DINO config's ``assigner2`` cost
  weights (the reference's own match-cost classes, imported by ``oracle.gen_golden.import_reference``); ``get_dist_info`` /
  ``concat_all_gather`` are stubbed for one rank, and ``prepare_unsup_cdn`` is a stub that reads the nine lists, ``thr_`` and
  the matched costs / gt indices out of its caller's frame and stops the call.
"""
import os
import sys
import types
import warnings

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle.gen_golden import import_reference, load_dino_detr_ssod  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "gmm.npz")


def sk_fit(costs, max_iter=100):
    import sklearn.mixture as skm
    x = np.sort(np.asarray(costs, np.float32)).reshape(-1, 1)
    g = skm.GaussianMixture(2, weights_init=np.array([0.5, 0.5]), means_init=np.array([x.min(), x.max()]).reshape(2, 1),
                            precisions_init=np.array([1.0, 1.0]).reshape(2, 1), covariance_type="diag", reg_covar=1e-5,
                            max_iter=max_iter)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        g.fit(x)
    return g.predict(x), g.score_samples(x), g.n_iter_, g.converged_, x[:, 0]


def fit_cases():
    r = np.random.default_rng(2024)
    return {
        "bimodal": np.concatenate([r.normal(1.0, 0.3, 60), r.normal(4.0, 0.8, 20)]),
        "heavy_tail": r.lognormal(0.5, 1.2, 120),
        "near_unimodal": r.normal(5.0, 0.5, 240),
        "n0": np.zeros(0),
        "n1": np.array([2.75]),
        "n2": np.array([3.0, 1.0]),
        "n3": np.array([0.6, 0.5, 2.0]),
        "duplicates": np.array([1.0, 5.0, 1.0, 2.0, 5.0, 1.0, 2.0, 5.0]),
        "all_equal": np.full(10, 2.5),
        "empty_comp0": np.array([1.0] + [1.0001] * 9),
        "empty_comp0_b": np.array([2.0, 2.0, 2.0, 2.0, 2.00001]),
        "n2400": np.concatenate([r.normal(1.2, 0.35, 1700), r.normal(3.5, 0.9, 700)]),
        "maxiter2": np.concatenate([r.normal(1.0, 0.5, 50), r.normal(2.5, 0.7, 30)]),
    }


def pick(labels, scores, x):
    """_fit_gmm's threshold rule (dino_detr_ssod.py:876-889) on sorted costs."""
    m = labels == 0 if (labels == 0).any() else labels == 1
    return x[m][int(torch.from_numpy(scores[m]).topk(1)[1])]


def gen_fit(ref, d):
    stand_in = types.SimpleNamespace(covariance_type="diag")
    names = []
    for name, c in fit_cases().items():
        c = c.astype(np.float32)
        max_iter = 2 if name == "maxiter2" else 100
        if max_iter == 100:
            thr = ref.DinoDetrSSOD._fit_gmm(stand_in, torch.from_numpy(c))
        d[f"fit.{name}.costs"] = c
        d[f"fit.{name}.max_iter"] = np.int64(max_iter)
        if c.size >= 2:
            lab, sc, it, cv, x = sk_fit(c, max_iter)
            if max_iter != 100:
                thr = pick(lab, sc, x)
            d[f"fit.{name}.labels"], d[f"fit.{name}.scores"] = lab.astype(np.int64), sc
            d[f"fit.{name}.n_iter"], d[f"fit.{name}.converged"] = np.int64(it), np.bool_(cv)
        d[f"fit.{name}.thr"] = np.asarray(thr, np.float32).reshape(())
        names.append(name)
    d["fit_names"] = np.asarray(names)


def e2e_inputs(seed=7):
    g = torch.Generator().manual_seed(seed)
    B, Q, C = 3, 40, 12
    hw = [(480, 640), (512, 512), (400, 600)]
    G = [9, 0, 6]
    gts, labs, scores, dets = [], [], [], []
    bbox = torch.rand(B, Q, 4, generator=g) * torch.tensor([1.0, 1.0, 0.3, 0.3]) + torch.tensor([0.0, 0.0, 0.05, 0.05])
    cls = torch.randn(B, Q, C, generator=g) * 1.5
    for b in range(B):
        h, w = hw[b]
        n = G[b]
        # pseudo gts: half sit on a query (low cost), half are random (high cost)
        q = torch.randperm(Q, generator=g)[:n]
        cxcywh = bbox[b, q].clone()
        cxcywh[n // 2:] = torch.rand(n - n // 2, 4, generator=g) * torch.tensor([1.0, 1.0, 0.3, 0.3]) + 0.05
        cxcywh[:n // 2] += torch.randn(n // 2, 4, generator=g) * 0.01
        xyxy = torch.cat([cxcywh[:, :2] - cxcywh[:, 2:] / 2, cxcywh[:, :2] + cxcywh[:, 2:] / 2], -1)
        gts.append((xyxy * torch.tensor([w, h, w, h], dtype=torch.float32)).float())
        labs.append(torch.randint(0, C, (n,), generator=g))
        scores.append(torch.rand(n, generator=g) * 0.8)
        dets.append(gts[-1] + torch.randn(n, 4, generator=g) * 2.0)
        if n:
            cls[b, q[:n // 2], labs[-1][:n // 2]] += 4.0
    return cls, bbox, hw, gts, labs, scores, dets


class _Captured(Exception):
    pass


def gen_e2e(ref, mc, tr, d):
    cls, bbox, hw, gts, labs, scores, dets = e2e_inputs()
    B = cls.shape[0]
    metas = [dict(img_shape=(h, w, 3)) for h, w in hw]
    captured = {}

    def prepare_unsup_cdn(*a, **k):
        captured.update(sys._getframe(1).f_locals)
        raise _Captured()

    ref.bbox_cxcywh_to_xyxy = tr.bbox_cxcywh_to_xyxy
    ref.bbox_xyxy_to_cxcywh = tr.bbox_xyxy_to_cxcywh
    ref.get_dist_info = lambda: (0, 1)
    ref.concat_all_gather = lambda t: t
    assigner2 = types.SimpleNamespace(cls_cost=mc.FocalLossCost(weight=2.0),
                                      reg_cost=mc.BBoxL1Cost(weight=5.0, box_format="xywh"),
                                      iou_cost=mc.IoUCost(iou_mode="giou", weight=2.0))
    head = types.SimpleNamespace(assigner2=assigner2, warm_up_step=0, in_warm_up=False, dn_number=100,
                                 dn_label_noise_ratio=0.5, dn_box_noise_scale=1.0)
    self = types.SimpleNamespace(student=types.SimpleNamespace(bbox_head=head),
                                 teacher=types.SimpleNamespace(extract_feat=lambda img: None),
                                 train_cfg=types.SimpleNamespace(pseudo_label_initial_score_thr=0.4), curr_step=0,
                                 covariance_type="diag", prepare_unsup_cdn=prepare_unsup_cdn)
    self._fit_gmm = lambda pts, device=None: ref.DinoDetrSSOD._fit_gmm(self, pts, device)
    student_info = dict(img=torch.zeros(1), backbone_feature=None, img_metas=metas,
                        outs=(cls[None], bbox[None], None, None, None, None))
    teacher_info = dict(det_bboxes=dets, det_labels=labs, det_scores=scores, img=torch.zeros(1), img_metas=metas)
    try:
        ref.DinoDetrSSOD.unsup_loss(self, student_info, teacher_info, gts, labs, scores)
        raise AssertionError("prepare_unsup_cdn was not reached")
    except _Captured:
        pass
    cat = lambda ts, w=None: torch.cat([t.reshape(-1, w) if w else t.reshape(-1) for t in ts]).numpy()  # noqa: E731
    d["e2e.cls"], d["e2e.bbox"] = cls.numpy(), bbox.numpy()
    d["e2e.img_hw"] = np.asarray(hw, np.int64)
    d["e2e.counts"] = np.asarray([len(t) for t in gts], np.int64)
    d["e2e.gt_bboxes"], d["e2e.gt_labels"], d["e2e.gt_scores"] = cat(gts, 4), cat(labs), cat(scores)
    d["e2e.det_bboxes"], d["e2e.det_labels"], d["e2e.det_scores"] = cat(dets, 4), cat(labs), cat(scores)
    d["e2e.thr"] = np.asarray(captured["thr_"], np.float32).reshape(-1)
    d["e2e.match_counts"] = np.asarray([len(t) for t in captured["match_gt_cost_list"]], np.int64)
    d["e2e.match_cost"] = cat(captured["match_gt_cost_list"]).astype(np.float32)
    d["e2e.match_inds"] = cat(captured["match_gt_inds_list"]).astype(np.int64)
    for name in ("gt_bboxes_list", "gt_labels_list", "gt_scores_list", "unsup_bboxes_gmm_list", "unsup_labels_gmm_list",
                 "unsup_scores_gmm_list", "det_bboxes_gmm_list", "det_labels_gmm_list", "det_scores_gmm_list"):
        lst = captured[name]
        assert len(lst) == B
        d[f"e2e.{name}.counts"] = np.asarray([len(t) for t in lst], np.int64)
        d[f"e2e.{name}"] = cat(lst, 4 if "bboxes" in name else None)


def main():
    import sklearn
    _, _, mc, tr, _ = import_reference()
    ref = load_dino_detr_ssod()
    d = {"sklearn_version": np.asarray(sklearn.__version__)}
    gen_fit(ref, d)
    gen_e2e(ref, mc, tr, d)
    np.savez_compressed(OUT, **d)
    print(OUT, os.path.getsize(OUT))


if __name__ == "__main__":
    main()
