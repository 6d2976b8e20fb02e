"""The fp64 statement and admissibility checkers of tests/loss_ref64.py, checked without a GPU:
  * it IS the loss: its values equal tests/set_loss_ref64.py to 1e-12 on the existing small problems, the reference's fixtures
    (tests/golden/tal_loss.npz, tests/golden/set_loss.npz) lie within its bounds, and its derivatives equal fp64 central
    differences;
  * satisfiable: eval_f32 (an fp32 evaluation with a cast after every operation) and the C oracle's tal_loss are admissible on
    every case of tests/loss_cases.py;
  * it bites: every mutant of eval_f32 is rejected, and the rejecting case is printed by name;
  * not vacuous: no element without statement on the ordinary cases, at most 2 % of any output on an adversarial one, and a finite
    bound on every element a case names as its target (saturated task-aligned ones: finite, non-negative results instead)."""
import numpy as np
import pytest

import loss_cases as lc
import loss_ref64 as L
import oracle
import set_loss_fixture as fx
import set_loss_ref64 as R
from assign_cases import golden as _npz
from assign_ref64 import bound, inp

F = np.float32
SET_CASES = lc.set_loss_cases()
TAL_CASES = lc.tal_cases()
FOCAL_CASES = lc.focal_cases()
NONE_CAP = 0.02                                                     # the issue's cap on elements without statement


def _ids(cs):
    return [c["name"] for c in cs]


def _ref64_segment(seg, coef):
    """set_loss_ref64 on one segment of a loss_cases problem -> stats, scales, d cls, d boxes"""
    P = seg["params"]
    nl, B, Q, C = seg["cls"].shape
    eps = float(F(P["iou_eps"]))
    if seg["kind"] == R.DN:
        lab, lw, tg, bw = R.dn_targets(seg["gts"], seg["labs"], seg["single_pad"], seg["groups"], seg["wh"].astype(np.float64), C)
        rep = lambda a: np.broadcast_to(a, (nl,) + a.shape)  # noqa: E731
        args = (R.DN, seg["cls"], seg["boxes"], rep(lab), rep(lw), rep(tg), rep(bw), seg["wh"])
        kw = dict(alpha=P["alpha"], gamma=P["gamma"], eps=eps)
    else:
        args = (seg["kind"], seg["cls"], seg["boxes"], seg["labels"], seg["label_weights"], seg["bbox_targets"], seg["bbox_weights"],
                seg["wh"])
        kw = dict(metrics=seg["metrics"], alpha=P["alpha"], gamma=P["gamma"], eps=eps)
    st = R.segment(*args, **kw)
    bg = float(F(P["bg_cls_weight"]))
    losses, sc = R.finalize(seg["kind"], st, R.norm_inputs(seg["kind"], st, B * Q, bg), P["cls_weight"], P["l1_weight"], P["iou_weight"])
    _, gx, gb = R.segment(*args, **kw, coef=sc * np.asarray(coef, np.float64))
    return st, losses, gx, gb


@pytest.mark.parametrize("p", [c for c in SET_CASES if not c["saturated"]], ids=lambda c: c["name"])
def test_statement_equals_set_loss_ref64(p):
    """values and gradients against the bare fp64 restatement, 1e-12 (of the largest gradient of the tensor for the gradients:
    a comparison of two fp64 evaluations, not of a kernel).  dn targets that are not exact in fp32 differ by their roundings in
    the restatement, which divides in fp64: compared on the dyadic cases and on the matched / warm-up segments."""
    t0 = 0
    for seg in p["segs"]:
        nl = seg["cls"].shape[0]
        coef = p["coef"][t0:t0 + nl]
        t0 += nl
        if seg["kind"] == R.DN and p["name"] not in ("boxes_dyadic", "dn_G0"):
            continue
        ref = L.segment_statement(seg, coef)
        st, losses, gx, gb = _ref64_segment(seg, coef)
        np.testing.assert_allclose(ref["stats"][0], st, rtol=1e-12, atol=1e-300)
        np.testing.assert_allclose(ref["terms"][0], losses, rtol=1e-12, atol=1e-300)
        np.testing.assert_allclose(ref["gcls"][0], gx, rtol=1e-12, atol=1e-12 * max(np.abs(gx).max(), 1e-300))
        plain = np.isfinite(ref["gbox"][1]).all(-1)
        np.testing.assert_allclose(ref["gbox"][0][plain], gb[plain], rtol=1e-12, atol=1e-12 * max(np.abs(gb).max(), 1e-300))


def test_statement_equals_set_loss_ref64_on_the_existing_small_problems():
    from test_set_loss_ref import _case
    for kind in (R.MATCHED, R.WARMUP):
        c = _case(3 + kind, kind, big=5.0)
        nl = c["x"].shape[0]
        seg = dict(kind=kind, cls=c["x"], boxes=c["b"], labels=c["labels"], label_weights=c["lw"].astype(F),
                   bbox_targets=c["tg"].astype(F), bbox_weights=c["bw"].astype(F),
                   metrics=None if c["metrics"] is None else c["metrics"].astype(F), wh=c["wh"].astype(F), params=lc.P_DEF)
        coef = (np.random.default_rng(9).random((nl, 5)) + 0.5).astype(F)
        ref = L.segment_statement(seg, coef)
        st, losses, gx, gb = _ref64_segment(seg, coef)
        np.testing.assert_allclose(ref["stats"][0], st, rtol=1e-12, atol=1e-300)
        np.testing.assert_allclose(ref["gcls"][0], gx, rtol=1e-12, atol=1e-12 * np.abs(gx).max())
        np.testing.assert_allclose(ref["gbox"][0], gb, rtol=1e-12, atol=1e-12 * np.abs(gb).max())


def test_tal_fixtures_within_bounds():
    """The reference's own fp32 task_aigned_focal_loss and its autograd gradient.  loss = sum / avg_factor and grad / avg_factor
    there: one more fp32 rounding each, charged as 2u of the value; torch's fp32 sum is a tree no deeper than tal_depth."""
    for name, g in _npz("tal_loss.npz").items():
        avg = float(g["avg_factor"])
        s, gr, _ = L.tal_statement(g["logits"], g["labels"], g["metric"], 2.0, False)
        s = (s[0] / avg, bound(s) / avg + 2 * L.U * abs(s[0] / avg) + L.TINY)
        gr = (gr[0] / avg, bound(gr) / avg + 2 * L.U * np.abs(gr[0] / avg) + L.TINY)
        rep = {}
        L._check(name, "loss", np.asarray(float(g["loss"])), s, rep, nonneg=True)
        L._check(name, "grad_logits", g["grad_logits"], gr, rep)
        print(L.table("tal_loss.npz " + name, rep))
        assert rep["grad_logits"]["none"] <= NONE_CAP or name == "sat"


@pytest.mark.parametrize("name", fx.NAMES)
def test_set_loss_fixture_values_within_bounds(name):
    """The loss dict of the reference's own loss() on the fixture's stored targets against the statement's terms."""
    c = fx.case(name)
    nl, B, Q = c["nl"], c["B"], c["Q"]
    warm = bool(c["warm_up"])
    rows = fx.key_rows(c["keys"], nl)
    P = dict(lc.P_DEF)
    sh = lambda a, n: a.reshape((n, B, Q) + a.shape[2:])  # noqa: E731
    segs = []
    for nm, sl, n in (("all", slice(0, nl * B), nl), ("enc", slice(nl * B, (nl + 1) * B), 1)):
        x = c["all_cls"] if nm == "all" else c["enc_cls"][None]
        b = c["all_box"] if nm == "all" else c["enc_box"][None]
        segs.append(dict(kind=R.WARMUP if warm else R.MATCHED, cls=x, boxes=b, labels=sh(c["labels"][sl], n),
                         label_weights=None if warm else sh(c["label_weights"][sl], n), bbox_targets=sh(c["bbox_targets"][sl], n),
                         bbox_weights=sh(c["bbox_weights"][sl], n), metrics=sh(c["norm_metrics"][sl], n) if warm else None,
                         wh=c["wh"].astype(F), params=P))
    segs.append(dict(kind=R.DN, cls=c["dn_cls"], boxes=c["dn_box"], gts=c["gt_list"], labs=c["lab_list"],
                     single_pad=int(c["single_pad"]), groups=int(c["groups"]), wh=c["wh"].astype(F), params=P))
    v, e = [], []
    for seg in segs:
        ref = L.segment_statement(seg, np.ones((seg["cls"].shape[0], 5), F))
        v.append(ref["terms"][0]); e.append(bound(ref["terms"]))
    v, e = np.concatenate(v), np.concatenate(e)
    zero_dn = warm and bool(c["is_pseudo_label"])                       # head.py:536-541: the dn losses are zeros there
    for k, got in zip(c["keys"], c["values"]):
        r, t = rows[k]
        if zero_dn and "dn_" in k:
            assert got == 0.0
            continue
        # the reference divides a torch fp32 sum (a tree of at most log2(n) + 8 levels) by its normaliser and multiplies by the
        # weight: the statement's own bound plus those roundings of the value
        n = segs[0]["cls"][0].size
        extra = (np.log2(n) + 8 + 2) * 2 * L.U * abs(v[r, t]) + L.TINY
        assert abs(float(got) - v[r, t]) <= e[r, t] + extra, (name, k, float(got), v[r, t], e[r, t] + extra)


def _cd(fn, x, h):
    return (fn(x + h) - fn(x - h)) / (2 * h)


def test_derivatives_equal_central_differences():
    """fp64 central differences of the statement's own value, away from kinks (ordinary ranges, |x| <= 4; h from the usual
    third-root rule for fp64, compared to 1e-6 of the derivative's scale, six orders inside what h^2 f''' leaves)."""
    r = np.random.default_rng(0)
    h = 1e-5
    x = r.uniform(-4, 4, 200)
    z = np.zeros_like(x)
    for gamma in (2.0, 1.5, 1.0, 3.0):
        for t in (True, False):
            tt = np.full(x.shape, t)
            f = lambda y: L.focal_elem((y, z), tt, 0.25, gamma)[0][0]  # noqa: E731
            d = L.focal_elem((x, z), tt, 0.25, gamma)[1][0]
            np.testing.assert_allclose(d, _cd(f, x, h), rtol=1e-6, atol=1e-8)
        for st in (0.0, 0.3, 1.0):
            s = (np.full(x.shape, st), z)
            f = lambda y: L.tal_elem((y, z), s, gamma)[0][0]  # noqa: E731
            d = L.tal_elem((x, z), s, gamma)[1][0]
            ok = np.abs(st - 1 / (1 + np.exp(-x))) > 1e-2                  # the kink of |s - p|^gamma
            np.testing.assert_allclose(d[ok], _cd(f, x, h)[ok], rtol=1e-6, atol=1e-8)
            pr = r.uniform(0.05, 0.95, 200)
            f = lambda y: L.tal_elem((y, z), s, gamma, True)[0][0]  # noqa: E731
            d = L.tal_elem((pr, z), s, gamma, True)[1][0]
            ok = np.abs(st - pr) > 1e-2
            np.testing.assert_allclose(d[ok], _cd(f, pr, h)[ok], rtol=1e-6, atol=1e-8)
    # GIoU in cxcywh, random boxes (no ties), c = 1
    n = 300
    b = np.concatenate([r.uniform(0.2, 0.8, (n, 2)), r.uniform(0.05, 0.4, (n, 2))], -1)
    tg = np.concatenate([r.uniform(0.2, 0.8, (n, 2)), r.uniform(0.05, 0.4, (n, 2))], -1)
    zz = np.zeros(n)
    fw, fh = (np.full(n, 640.0), zz), (np.full(n, 480.0), zz)
    pair = lambda a: [(a[:, k], zz) for k in range(4)]  # noqa: E731
    loss, grad_fn, sels = L.giou_elem(pair(b), pair(tg), fw, fh, 1e-6)
    g = grad_fn([m for m, _ in sels], (np.ones(n), zz))
    for k in range(4):
        def f(delta):
            bb = b.copy()
            bb[:, k] += delta
            return L.giou_elem(pair(bb), pair(tg), fw, fh, 1e-6)[0][0]
        cd = (f(1e-6) - f(-1e-6)) / 2e-6
        far = np.ones(n, bool)                                            # no corner within 1e-4 of its counterpart
        for q in range(4):
            far &= np.abs(_corner(b, q) - _corner(tg, q)) > 1e-4
        np.testing.assert_allclose(g[k][0][far], cd[far], rtol=1e-5, atol=1e-7)


def _corner(b, q):
    return b[:, q % 2] + (0.5 if q >= 2 else -0.5) * b[:, q % 2 + 2]


def _caps(case, rep):
    for out, v in rep.items():
        cap = 0.0 if case.get("ordinary") else NONE_CAP
        assert v["none"] <= cap, f"{case['name']}: {out}: {v['none']:.2%} of the elements have no statement (cap {cap:.0%})"


@pytest.mark.parametrize("p", SET_CASES, ids=lambda c: c["name"])
def test_eval_f32_set_loss_admissible_and_not_vacuous(p):
    rep = L.check_set_loss(p, *L.eval_f32("set_loss", p))
    print("\n" + L.table(p["name"], rep))
    _caps(p, rep)
    t0 = 0
    for si, seg in enumerate(p["segs"]):
        nl = seg["cls"].shape[0]
        ref = L.segment_statement(seg, p["coef"][t0:t0 + nl])
        t0 += nl
        for (l, b, q) in p["targets"].get(si, ()):
            assert np.isfinite(ref["gbox"][1][l, b, q]).all(), (p["name"], si, "gbox", l, b, q)
            if not (p["saturated"] and seg["kind"] == R.WARMUP):
                assert np.isfinite(ref["gcls"][1][l, b, q]).all(), (p["name"], si, "gcls", l, b, q)
        if p["name"] == "dn_G0" and seg["kind"] == R.DN:
            for key in ("terms", "gcls", "gbox"):
                assert not ref[key][0].any() and not ref[key][1].any()            # exact zeros, no allowance


@pytest.mark.parametrize("c", TAL_CASES, ids=lambda c: c["name"])
def test_eval_f32_and_oracle_tal_admissible(c):
    args = (c["logits"], c["labels"], c["metrics"], c["gamma"], c["input_is_prob"])
    s, g = L.eval_f32("tal", *args)
    rep = L.check_tal(*args, s, g, name=c["name"] + " (eval_f32)")
    so, go = oracle.tal_loss(c["logits"], c["labels"], c["metrics"], gamma=c["gamma"], input_is_prob=c["input_is_prob"])
    rep_o = L.check_tal(*args, so, go, name=c["name"] + " (oracle)")
    print("\n" + L.table(c["name"], rep) + "\n" + L.table(c["name"] + " (oracle)", rep_o))
    _caps(c, rep)
    _, gr, _ = L.tal_statement(*args)
    if not c["saturated"]:
        for i in c["targets"]:
            assert np.isfinite(gr[1][i]), (c["name"], i)


@pytest.mark.parametrize("c", FOCAL_CASES, ids=lambda c: c["name"])
def test_eval_f32_focal_admissible(c):
    args = (c["logits"], c["labels"], c["weights"], c["alpha"], c["gamma"])
    rep = L.check_focal(*args, *L.eval_f32("focal", *args), name=c["name"])
    print("\n" + L.table(c["name"], rep))
    assert all(v["none"] == 0.0 for v in rep.values())                     # the softplus form has a statement at every logit


def test_two_copies_one_statement():
    """tal_elem of set_loss.hip and the body of tal_loss_kernel are judged by the same function: the warm-up segment's
    statistic 0 and the tal entry's sum are the same number in the statement."""
    p = SET_CASES[0]
    seg = p["segs"][1]
    nl, B, Q, C = seg["cls"].shape
    ref = L.segment_statement(seg, p["coef"][nl:2 * nl])
    s, _, _ = L.tal_statement(seg["cls"][0].reshape(-1, C), seg["labels"][0].reshape(-1), seg["metrics"][0].reshape(-1), 2.0, False)
    assert abs(ref["stats"][0][0, 0] - s[0]) <= 1e-12 * abs(s[0])


@pytest.mark.parametrize("mutant", L.MUTANTS)
def test_mutants_rejected(mutant):
    hits = []
    for p in SET_CASES:
        try:
            L.check_set_loss(p, *L.eval_f32("set_loss", p, mutant=mutant))
        except L.Inadmissible as e:
            hits.append(str(e))
    for c in TAL_CASES[:4] + TAL_CASES[5:]:
        args = (c["logits"], c["labels"], c["metrics"], c["gamma"], c["input_is_prob"])
        try:
            L.check_tal(*args, *L.eval_f32("tal", *args, mutant=mutant), name="tal " + c["name"])
        except L.Inadmissible as e:
            hits.append(str(e))
    for c in FOCAL_CASES:
        args = (c["logits"], c["labels"], c["weights"], c["alpha"], c["gamma"])
        try:
            L.check_focal(*args, *L.eval_f32("focal", *args, mutant=mutant), name="focal " + c["name"])
        except L.Inadmissible as e:
            hits.append(str(e))
    print(f"\n{mutant}: rejected by {len(hits)} cases, first: {hits[0] if hits else None}")
    assert hits, f"mutant {mutant} is admissible on every case"


def test_unit_of_the_exact_operations():
    """the exactness rule charges nothing for an fp32-representable result of exact operands, and a rounding otherwise"""
    a, b = inp(F(0.5)), inp(F(0.25))
    assert L.xsub(a, b)[1] == 0 and L.xmul(a, inp(F(512.0)))[1] == 0
    assert L.xdiv(inp(F(1.0)), inp(F(3.0)))[1] > 0 and L.xmul(inp(F(0.1)), inp(F(1333.0)))[1] > 0
