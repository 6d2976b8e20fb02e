#!/usr/bin/env python
"""Times the cost-GMM double filter of the unsupervised loss on bench-shaped inputs (4 images, Q 900, C 80, 0-300 pseudo gts):

1. the reference-shaped host path: the project's cost matrix + LSAP, a per-image ``.cpu()`` of the matched costs,
   scikit-learn's GaussianMixture when importable (otherwise tests/gmm_ref64.py), host set logic;
2. ``unsup_gmm_filter``: wall time per call (cost + LSAP + the three new launches + one pinned read-back), and the GPU
   time of the fit launch alone from event pairs on that call's matched costs.

    python tools/gmm_filter_probe.py [--iters 50] [--out bench_out/gmm_probe.json]
"""
import argparse
import json
import os
import sys
import time
import warnings

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import semi_detr_amd as s  # noqa: E402
from gmm_ref64 import double_filter_sets, fit_gmm_ref64  # noqa: E402


def inputs(seed=0, B=4, Q=900, C=80, dev="cuda:0"):
    g = torch.Generator().manual_seed(seed)
    hw = [(800, 1333), (800, 1200), (750, 1333), (800, 1066)][:B]
    G = [300, 0, 57, 181][:B]
    cls = torch.randn(B, Q, C, generator=g) * 2
    bbox = torch.cat([torch.rand(B, Q, 2, generator=g), torch.rand(B, Q, 2, generator=g) * 0.3 + 0.02], -1)
    gts, labs, scores = [], [], []
    for b in range(B):
        h, w = hw[b]
        xy = torch.rand(G[b], 2, generator=g) * torch.tensor([w * 0.8, h * 0.8])
        gts.append(torch.cat([xy, xy + torch.rand(G[b], 2, generator=g) * 200 + 8], -1).to(dev))
        labs.append(torch.randint(0, C, (G[b],), generator=g).to(dev))
        scores.append(torch.rand(G[b], generator=g).to(dev))
    return cls.to(dev), bbox.to(dev), gts, labs, scores, [dict(img_shape=(h, w, 3)) for h, w in hw]


def sk_threshold(costs):
    import sklearn.mixture as skm
    x = np.sort(costs).reshape(-1, 1)
    gm = skm.GaussianMixture(2, weights_init=np.array([0.5, 0.5]), means_init=np.array([x.min(), x.max()]).reshape(2, 1),
                             precisions_init=np.array([1.0, 1.0]).reshape(2, 1), covariance_type="diag", reg_covar=1e-5)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        gm.fit(x)
    lab, sc = gm.predict(x), gm.score_samples(x)
    m = lab == 0 if (lab == 0).any() else lab == 1
    return x[m, 0][int(np.argmax(sc[m]))]


def host_path(asg, cls, bbox, gts, labs, scores, metas, fit):
    _, costs, res = asg.assign_batch(bbox, cls, gts, labs, metas, return_cost=True)
    po = res["pair_offsets"]
    mc, mi = [], []
    for b in range(len(gts)):
        r, c = res["rows"][po[b]:po[b + 1]], res["cols"][po[b]:po[b + 1]]
        mc.append(costs[b].detach().cpu()[r.cpu(), c.cpu()])
        mi.append(c.cpu())
    thr = fit(torch.cat(mc).numpy())
    return [double_filter_sets(mc[b].numpy(), mi[b].numpy(), scores[b].cpu().numpy(), thr) for b in range(len(gts))]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    cls, bbox, gts, labs, scores, metas = inputs()
    asg = s.HungarianAssigner(cls_cost=dict(type="FocalLossCost", weight=2.0),
                              reg_cost=dict(type="BBoxL1Cost", weight=5.0, box_format="xywh"),
                              iou_cost=dict(type="IoUCost", iou_mode="giou", weight=2.0))
    try:
        import sklearn  # noqa: F401
        fit, fit_name = sk_threshold, "sklearn"
    except ImportError:
        fit, fit_name = (lambda c: fit_gmm_ref64(c)["thr"]), "gmm_ref64"
    run = lambda: s.unsup_gmm_filter(cls, bbox, gts, labs, scores, gts, labs, scores, metas, asg)  # noqa: E731
    for _ in range(5):
        host_path(asg, cls, bbox, gts, labs, scores, metas, fit)
        run()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(a.iters):
        host_path(asg, cls, bbox, gts, labs, scores, metas, fit)
    host_ms = (time.perf_counter() - t0) / a.iters * 1e3
    t0 = time.perf_counter()
    for _ in range(a.iters):
        res = run()
    dev_ms = (time.perf_counter() - t0) / a.iters * 1e3
    # GPU time of the fit launch alone, on this call's matched costs (one segment)
    costs = torch.cat(res.match_gt_cost_list)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    fits = []
    for _ in range(a.iters):
        e0.record()
        s.fit_gmm_threshold(costs)
        e1.record()
        e1.synchronize()
        fits.append(e0.elapsed_time(e1) * 1e3)
    _, det = s.fit_gmm_threshold(costs, return_details=True)
    out = dict(n_costs=int(costs.numel()), n_iter=int(det["n_iter"]), host_path_ms=host_ms, host_fit=fit_name,
               unsup_gmm_filter_wall_ms=dev_ms, fit_kernel_us_median=float(np.median(fits)),
               fit_kernel_us_min=float(np.min(fits)), device=torch.cuda.get_device_name(0))
    print(json.dumps(out))
    if a.out:
        os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(out, f)


if __name__ == "__main__":
    main()
