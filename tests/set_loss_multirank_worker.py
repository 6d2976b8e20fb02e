"""One rank of tests/test_gpu_set_loss_multirank.py (run by torch.distributed.run, two ranks on one GPU over gloo).
Each rank has its own targets; the check: one all-reduce per loss() and per set_losses(), the reduced normalisers are the
mean of both ranks' inputs, the losses are the float64 restatement finalized with them (classification normaliser
reduced only for warm-up or sync_cls_avg_factor), and FocalLoss does no collective."""
import json
import os
import sys

import numpy as np
import torch
import torch.distributed as dist

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import set_loss_ref64 as R  # noqa: E402
from test_gpu_set_loss import P2, _call_loss, _e2e_inputs, _head, _problem, _segments  # noqa: E402


def main():
    import semi_detr_amd as s
    from semi_detr_amd import dp
    rank, _, world = dp.init_distributed("gloo")
    assert world == 2
    calls = []
    real = dist.all_reduce

    def counting(*a, **k):
        calls.append(1)
        return real(*a, **k)
    dist.all_reduce = counting
    report = {}
    for warm, sync in ((False, False), (False, True), (True, False)):
        p = _problem(seed=40 + rank, nl=2, B=2, Q=50, single_pad=8, groups=3, warm=warm,
                     counts=[3 + rank * 4, rank * 2])
        params = dict(P2, sync_cls=sync)
        segs, _ = _segments(p, torch.device("cuda"), params)
        info = {}
        n0 = len(calls)
        terms = s.set_losses(segs, info=info)
        n_calls = len(calls) - n0
        local = info["norms"].clone()
        both = [torch.empty_like(local) for _ in range(2)]
        dist.all_gather(both, local)
        mean = ((both[0] + both[1]) / 2).cpu().numpy()
        red = info["norms_reduced"].cpu().numpy()
        st = info["stats"].cpu().numpy()
        got = torch.stack([torch.stack(r) for r in terms]).detach().cpu().numpy()
        kinds = [R.WARMUP if warm else R.MATCHED] * 3 + [R.DN] * 2
        want = []
        for t, kind in enumerate(kinds):
            nin = mean[t].copy()
            if not (kind == R.WARMUP or sync):
                nin[0] = local[t, 0].item()
            want.append(R.finalize(kind, st[t:t + 1], nin[None], 2.0, 5.0, 2.0)[0][0])
        want = np.asarray(want)
        report[f"warm{int(warm)}_sync{int(sync)}"] = dict(
            calls=n_calls, reduced_is_mean=bool(np.allclose(red, mean, rtol=1e-6, atol=0)),
            losses_ok=bool(np.all(np.abs(got - want) <= 3e-6 * np.maximum(np.abs(want), 1e-3))),
            ranks_differ=bool(not torch.equal(both[0], both[1])))
    h = _head()
    d = _e2e_inputs(60 + rank, nl=2, B=2, Q=120, single_pad=20, groups=5)
    n0 = len(calls)
    out = _call_loss(h, d)
    sum(out.values()).backward()
    report["loss_set_calls"] = len(calls) - n0
    n0 = len(calls)
    x = torch.randn(40, 80, device="cuda", requires_grad=True)
    s.FocalLoss(loss_weight=2.0)(x, torch.full((40,), 80, dtype=torch.long, device="cuda"), avg_factor=3.0).backward()
    report["focal_calls"] = len(calls) - n0
    torch.cuda.synchronize()
    print("RANK%d %s" % (rank, json.dumps(report)), flush=True)
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
