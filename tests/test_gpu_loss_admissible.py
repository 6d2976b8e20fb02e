"""The loss kernels (csrc/set_loss.hip, csrc/tal_loss.hip) against the fp64 statement of tests/loss_ref64.py, through the public
entry points: ``set_losses`` (matched, warm-up and dn segments in one launch, on every case of tests/loss_cases.py),
``TaskAlignedFocalLoss.forward_logits``, the probability contract of ``TaskAlignedFocalLoss``,
``task_aligned_focal_loss(reduction="sum")`` and ``FocalLoss``.  A result is ADMISSIBLE when every loss, statistic and gradient
element is within the bound the statement derives for it (loss_ref64's docstring: the running (value, err) arithmetic, exact ties
under torch's rule with no allowance, the hull of the branches where the operands' intervals merely meet), the count statistics
are exact, and whatever has no statement is finite (task-aligned losses: not negative).  No tolerance here is a literal.

Every case runs twice and must be bitwise equal.  With -s every test prints, per case, the worst err / bound of each output, the
number of box rows whose gradient used a hull and the share of elements without statement."""
import numpy as np
import pytest
import torch

import loss_cases as lc
import loss_ref64 as L

pytestmark = pytest.mark.gpu
F = np.float32
SET_CASES = lc.set_loss_cases()
TAL_CASES = lc.tal_cases()


def _t(a, dt=None):
    t = torch.from_numpy(np.ascontiguousarray(a)).cuda()
    return t if dt is None else t.to(dt)


def _leaf(a, unaligned=False):
    """-> (tensor handed to the kernel, function returning its gradient).  unaligned: a view 4 bytes off the 16-byte grid."""
    if not unaligned:
        x = _t(a).requires_grad_(True)
        return x, lambda: x.grad.cpu().numpy()
    flat = torch.zeros(a.size + 1, dtype=torch.float32, device="cuda")
    flat[1:] = _t(a).reshape(-1)
    flat.requires_grad_(True)
    x = flat[1:].view(a.shape)
    assert x.data_ptr() % 16 == 4
    return x, lambda: flat.grad[1:].view(a.shape).cpu().numpy()


def _guard(fn):
    try:
        return fn()
    except L.Inadmissible as e:
        raise AssertionError(str(e)) from None


def _run_set_loss(p, segs_idx=None):
    import semi_detr_amd as s
    from semi_detr_amd import set_loss as sl
    segs, grads = [], []
    for seg in (p["segs"] if segs_idx is None else [p["segs"][i] for i in segs_idx]):
        P = dict(seg["params"])
        nl, B, Q, C = seg["cls"].shape
        cls, gcls = _leaf(seg["cls"], p.get("unaligned", False))
        box, gbox = _leaf(seg["boxes"])
        wh = _t(seg["wh"])
        if seg["kind"] == L.DN:
            segs.append(s.SetLossSegment(sl.DN, cls, box, gt_bboxes=[_t(g) for g in seg["gts"]], gt_labels=[_t(g) for g in seg["labs"]],
                                         single_pad=seg["single_pad"], dn_groups=seg["groups"], img_wh=wh, **P))
        else:
            warm = seg["kind"] == L.WARMUP
            if warm:
                P.pop("alpha")
            flat = lambda a: None if a is None else _t(a.reshape((nl * B, Q) + a.shape[3:]))  # noqa: E731
            segs.append(s.SetLossSegment(sl.WARMUP if warm else sl.MATCHED, cls, box, labels=flat(seg["labels"]),
                                         label_weights=flat(seg["label_weights"]), bbox_targets=flat(seg["bbox_targets"]),
                                         bbox_weights=flat(seg["bbox_weights"]), metrics=flat(seg["metrics"]), img_wh=wh, **P))
        grads.append((gcls, gbox))
    info = {}
    terms = s.set_losses(segs, info=info)
    coef = p["coef"]
    assert len(terms) == len(coef)
    tot = sum(t * float(c) for row, cr in zip(terms, coef) for t, c in zip(row, cr))      # float(fp32) is exact: grad_out = coef
    tot.backward()
    got = torch.stack([torch.stack(r) for r in terms]).detach().cpu().numpy()
    return got, info["stats"].cpu().numpy(), [(a(), b()) for a, b in grads]


def _bitwise(a, b):
    ta, sa, ga = a
    tb, sb, gb = b
    ok = np.array_equal(ta.view(np.uint32), tb.view(np.uint32)) and np.array_equal(sa.view(np.uint64), sb.view(np.uint64))
    for (x1, y1), (x2, y2) in zip(ga, gb):
        ok = ok and np.array_equal(x1.view(np.uint32), x2.view(np.uint32)) and np.array_equal(y1.view(np.uint32), y2.view(np.uint32))
    return ok


@pytest.mark.parametrize("p", SET_CASES, ids=lambda c: c["name"])
def test_set_losses_admissible(p):
    out = _run_set_loss(p)
    rep = _guard(lambda: L.check_set_loss(p, *out))
    print("\n" + L.table(p["name"], rep))
    assert _bitwise(out, _run_set_loss(p)), f"{p['name']}: two runs differ"
    if p["name"] == "dn_G0":                            # no gt anywhere: exact zeros, not small numbers
        nl = p["segs"][2]["cls"].shape[0]
        assert not out[0][-nl:].any() and not out[2][2][0].any() and not out[2][2][1].any()


def _tal_entry(c, entry):
    from semi_detr_amd import TaskAlignedFocalLoss, task_aligned_focal_loss
    x = _t(c["logits"]).requires_grad_(True)
    lab, met = _t(c["labels"]), _t(c["metrics"])
    crit = TaskAlignedFocalLoss(use_sigmoid=True, gamma=c["gamma"], reduction="sum", loss_weight=1.0)
    if entry == "functional":
        loss = task_aligned_focal_loss(x, lab, met, gamma=c["gamma"], reduction="sum", from_logits=not c["input_is_prob"])
    elif c["input_is_prob"]:
        loss = crit(x, lab, met)
    else:
        loss = crit.forward_logits(x, lab, met)
    loss.backward()                                      # loss_weight 1, reduction sum: the upstream gradient is an exact 1
    return np.float32(loss.item()), x.grad.cpu().numpy()


@pytest.mark.parametrize("c", TAL_CASES, ids=lambda c: c["name"])
def test_tal_entries_admissible(c):
    """forward_logits (logit cases) / the module's probability contract (prob cases), and the functional form with
    reduction='sum', on every task-aligned case"""
    args = (c["logits"], c["labels"], c["metrics"], c["gamma"], c["input_is_prob"])
    print()
    for entry in ("module", "functional"):
        s, g = _tal_entry(c, entry)
        rep = _guard(lambda: L.check_tal(*args, s, g, name=f"{c['name']} ({entry})"))
        print(L.table(f"{c['name']} ({entry})", rep))
        s2, g2 = _tal_entry(c, entry)
        assert s.view(np.uint32) == s2.view(np.uint32) and np.array_equal(g.view(np.uint32), g2.view(np.uint32)), c["name"]


def test_tal_probability_contract_on_fp32_sigmoids():
    """TaskAlignedFocalLoss.forward as the reference calls it: the caller's fp32 sigmoid of ordinary logits goes in as p"""
    print()
    for c in TAL_CASES[:4]:
        with np.errstate(all="ignore"):
            prob = (F(1) / (F(1) + np.exp(-c["logits"]))).astype(F)
        cp = dict(c, logits=prob, input_is_prob=True)
        s, g = _tal_entry(cp, "module")
        rep = _guard(lambda: L.check_tal(prob, c["labels"], c["metrics"], c["gamma"], True, s, g, name=c["name"] + " (prob)"))
        print(L.table(c["name"] + " (prob)", rep))


@pytest.mark.parametrize("c", lc.focal_cases(), ids=lambda c: c["name"])
def test_focal_loss_admissible(c):
    import semi_detr_amd as s
    outs = []
    for _ in range(2):
        x = _t(c["logits"]).requires_grad_(True)
        crit = s.FocalLoss(use_sigmoid=True, gamma=c["gamma"], alpha=c["alpha"], reduction="sum", loss_weight=1.0)
        loss = crit(x, _t(c["labels"]), None if c["weights"] is None else _t(c["weights"]))
        loss.backward()
        outs.append((np.float32(loss.item()), x.grad.cpu().numpy()))
    rep = _guard(lambda: L.check_focal(c["logits"], c["labels"], c["weights"], c["alpha"], c["gamma"], *outs[0], name=c["name"]))
    print("\n" + L.table(c["name"], rep))
    assert outs[0][0].view(np.uint32) == outs[1][0].view(np.uint32) and np.array_equal(outs[0][1].view(np.uint32), outs[1][1].view(np.uint32))


@pytest.mark.parametrize("name", ["ordinary_a", "logits_g1.5"])
def test_two_copies_of_the_task_aligned_element(name):
    """The same rows through the tal_loss entry and through a warm-up segment of set_loss alone: tal_loss_kernel's body and
    set_loss.hip's tal_elem are separate copies of one formula, and each must be admissible against the ONE statement."""
    p = next(c for c in SET_CASES if c["name"] == name)
    seg = p["segs"][1]
    nl, B, Q, C = seg["cls"].shape
    gamma = seg["params"]["gamma"]
    c = dict(logits=seg["cls"].reshape(-1, C), labels=seg["labels"].reshape(-1), metrics=seg["metrics"].reshape(-1), gamma=gamma,
             input_is_prob=False)
    s, g = _tal_entry(c, "module")
    rep = _guard(lambda: L.check_tal(c["logits"], c["labels"], c["metrics"], gamma, False, s, g, name=name + " (tal_loss entry)"))
    print("\n" + L.table(name + " (tal_loss entry)", rep))
    sub = dict(p, segs=[seg], coef=p["coef"][nl:2 * nl], unaligned=False)
    rep = _guard(lambda: L.check_set_loss(sub, *_run_set_loss(sub)))
    print(L.table(name + " (warm-up segment)", rep))
