"""CPU: the fp64 reference with per-element bounds (tests/msda_ref64.py) that tests/test_gpu_msda_bounds.py judges the kernels by.

  * it is the op: equal to the C oracle's f64 path to 1e-12, and the reference's own fixtures (tests/golden/msda.npz, msda_full.npz)
    lie within its bound;
  * the bound can be met by honest fp32 arithmetic: the fp32 oracle passes it on every small configuration the GPU module uses;
  * it is tight enough to catch what a kernel rewrite might slip in: value read as fp16 / bf16, weights rounded to fp16, the
    smallest sample dropped, locations shifted by 1e-4 px, 1e-5 noise on the attention -- each fails it;
  * the GPU module's route table lists every kernel route the product dispatcher (semi-detr_amd/csrc/msda.hip, msda_dispatch.h) can report.
"""
import os
import re

import numpy as np
import pytest

import msda_ref64 as R
import oracle
from conftest import FULL_LEVELS, GOLDEN, Golden, full_shape_inputs, kink_mask, skipped_sample_mask
from test_gpu_msda_bounds import ROUTES, SMALL_CASES, make_case

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bundle(c):
    """(value, shapes, loc, attn, gout) of a make_case() case in the contract form (the fused prologue restated in fp32)."""
    if c["ref"] is None:
        return c["value"], c["shapes"], c["loc"], c["attn"], c["gout"]
    pro = R.prologue(c["ref"], c["off"], c["logits"], c["shapes"], c["off"].shape[4])
    return c["value"], c["shapes"], pro["loc"].astype(np.float32), pro["attn"].astype(np.float32), c["gout"]


def test_ref64_equals_the_oracle_in_fp64():
    for name in ("signed_dino", "boxes_window", "wide_level", "five_levels"):
        value, shp, loc, attn, gout = [a if a.dtype == np.int64 else a.astype(np.float64) for a in _bundle(make_case(SMALL_CASES[name]))]
        r = R.msda(value, shp, loc, attn, gout)
        want = [oracle.msda_forward(value, shp, loc, attn)] + list(oracle.msda_backward(value, shp, loc, attn, gout))
        for key, w in zip(("out", "grad_value", "grad_loc", "grad_attn"), want):
            np.testing.assert_allclose(r[key].val, w, rtol=1e-12, atol=1e-12 * max(1.0, float(np.abs(w).max())), err_msg=(name, key))


@pytest.mark.parametrize("case", Golden("msda.npz").names())
def test_ref64_and_the_reference_fixtures(case):
    """f64 fixtures: equal to 1e-12; f32 fixtures (the reference's own fp32 arithmetic): within the fp32 bound."""
    g = Golden("msda.npz")[case]
    r = R.msda(g["value"], g["shapes"], g["loc"], g["attn"], g["gout"])
    f64 = g["value"].dtype == np.float64
    keep = ~(kink_mask(g["loc"], g["shapes"]) | skipped_sample_mask(g["loc"], g["shapes"]))
    for key, fx in (("out", "out"), ("grad_value", "gvalue"), ("grad_attn", "gattn"), ("grad_loc", "gloc")):
        want, b = g[fx], r[key]
        if key == "grad_loc":
            want, b = want[keep], R.Bounded(b.val[keep], b.A[keep], b.n, b.C[keep])
        if f64:
            np.testing.assert_allclose(b.val, want, rtol=1e-12, atol=1e-12 * max(1.0, float(np.abs(want).max())), err_msg=key)
        else:
            R.check("fixture " + case, key, want, b)


def test_ref64_bounds_the_reference_full_shape_fixture():
    """tests/golden/msda_full.npz: the reference's fp32 CPU outputs at the BASELINE shape (N = 2, Lq = 300, S = 22 223)."""
    z = np.load(os.path.join(GOLDEN, "msda_full.npz"))
    value, loc, attn, gout = [t.numpy() for t in full_shape_inputs()]
    shp = np.asarray(FULL_LEVELS, np.int64)
    r = R.msda(value, shp, loc, attn, gout)
    R.check("fixture full", "out", z["out"], r["out"])
    R.check("fixture full", "grad_attn", z["gattn"], r["grad_attn"])
    gl = r["grad_loc"]
    keep = ~skipped_sample_mask(loc, shp)
    R.check("fixture full", "grad_loc", z["gloc"][keep], R.Bounded(gl.val[keep], gl.A[keep], gl.n, gl.C[keep], gl.skip[keep]))
    gv = r["grad_value"]
    rows = lambda x: np.broadcast_to(x, gv.val.shape).reshape(2, -1, 256)[:, ::61]      # noqa: E731
    R.check("fixture full", "grad_value rows", z["gvalue_rows"], R.Bounded(rows(gv.val), rows(gv.A), rows(gv.n), rows(gv.C)))


@pytest.mark.parametrize("name", sorted(SMALL_CASES))
def test_fp32_oracle_is_within_the_bound(name):
    """Honest fp32 arithmetic (the C oracle's f32 path, sequential sums) on every small configuration of the GPU module, fed what the
    kernel would see (the fused cases: the prologue rounded to fp32 first -- inside the bound's prologue allowance)."""
    c = make_case(SMALL_CASES[name])
    value, shp, loc, attn, gout = _bundle(c)
    if c["mask"] is not None:
        value = np.where(c["mask"][:, :, None, None], np.float32(0), value)
    if c["ref"] is None:
        r = R.msda(value, shp, loc, attn, gout)
    else:
        r = R.fused(value, shp, c["ref"], c["off"], c["logits"], gout, mask=c["mask"])
    o = oracle.msda_forward(value, shp, loc, attn)
    gv, gl, ga = oracle.msda_backward(value, shp, loc, attn, gout)
    if c["mask"] is not None:
        gv[c["mask"]] = 0
    worst = [R.check("oracle32 " + name, "out", o, r["out"]), R.check("oracle32 " + name, "grad_value", gv, r["grad_value"]),
             R.check("oracle32 " + name, "grad_attn", ga, r["grad_attn"]), R.check("oracle32 " + name, "grad_loc", gl, r["grad_loc"])]
    if c["ref"] is not None:
        pro = r["prologue"]
        worst.append(R.check("oracle32 " + name, "grad_offsets", (gl * pro["scale"]).astype(np.float32), r["grad_offsets"]))
        a = attn.astype(np.float64).reshape(r["grad_logits"].val.shape)
        g = ga.astype(np.float64).reshape(a.shape)
        glog = (a * (g - (a * g).sum(-1, keepdims=True))).astype(np.float32)
        worst.append(R.check("oracle32 " + name, "grad_logits", glog, r["grad_logits"]))
    print(name, ["%.3f" % w for w in worst])


# ---- mutants: each must break the bound of every result it touches

def _mutant_inputs():
    c = make_case(SMALL_CASES["signed_dino"])
    return c["value"], c["shapes"], c["loc"], c["attn"], c["gout"]


def _fp16(x):
    return x.astype(np.float16).astype(np.float64)


def _bf16(x):
    b = np.ascontiguousarray(x, np.float32).view(np.uint32)
    b = ((b + 0x7FFF + ((b >> 16) & 1)) & 0xFFFF0000).astype(np.uint32)      # round to nearest even
    return b.view(np.float32).astype(np.float64)


def _drop_smallest(a, c):
    """the sample of smallest |a| of every (query, head) row is left out entirely (all four corners)."""
    flat = np.abs(a).reshape(*a.shape[:3], -1)
    drop = np.zeros(flat.shape, bool)
    np.put_along_axis(drop, np.argmin(flat, -1)[..., None], True, -1)
    return a, np.where(drop.reshape(a.shape)[..., None], 0.0, c)


MUTANTS = {
    "value_fp16": dict(value=_fp16),
    "value_bf16": dict(value=_bf16),
    "weights_fp16": dict(hook=lambda a, c: (_fp16(a), _fp16(c))),
    "smallest_sample_dropped": dict(hook=_drop_smallest),
    "location_shift_1e-4px": dict(loc=None),
    "attention_noise_1e-5": dict(attn=None),
}


@pytest.mark.parametrize("mutant", sorted(MUTANTS))
def test_mutants_break_the_bound(mutant):
    value, shp, loc, attn, gout = _mutant_inputs()
    honest = R.msda(value, shp, loc, attn, gout)
    spec = MUTANTS[mutant]
    v2, l2, a2 = value.astype(np.float64), loc.astype(np.float64), attn.astype(np.float64)
    if "value" in spec:
        v2 = spec["value"](value)
    if "loc" in spec:
        W = shp[:, 1].astype(np.float64).reshape(-1, 1)
        l2 = l2.copy()
        l2[..., 0] += 1e-4 / W
    if "attn" in spec:
        a2 = a2 * (1 + 1e-5 * np.random.default_rng(1).standard_normal(a2.shape))
    bad = R.msda(v2, shp, l2, a2, gout, weights_hook=spec.get("hook"))
    # (grad_value does not read value; grad_attn does not read the attention)
    results = ["out", "grad_attn"] if "value" in spec else ["out", "grad_value", "grad_attn"]
    if mutant == "attention_noise_1e-5":
        results = ["out", "grad_value"]
    for key in results:
        worst = float(honest[key].ratio(bad[key].val).max())
        print(mutant, key, "%.3g" % worst)
        assert worst > 1.0, (mutant, key, worst)


# ---- the route table

def product_routes():
    """Every string the product build of msda.hip (with its product dispatch, msda_dispatch.h) can assign to g_last_kernels ("" and
    the SEMIDETR_SCATTER_SW knob's msda_sw_d32 routes excluded)."""
    src = "".join(open(os.path.join(ROOT, "semi-detr_amd", "csrc", name)).read() for name in ("msda.hip", "msda_dispatch.h"))
    found = set()
    for stmt in re.findall(r"g_last_kernels\s*=\s*([^;]*);", src):
        found.update(re.findall(r'"([^"]*)"', stmt))
    return {s for s in found if s and "msda_sw_d32" not in s}


def test_route_table_lists_every_product_route():
    routes = product_routes()
    assert len(routes) >= 12, routes
    assert routes == set(ROUTES), ("routes without a bounded GPU case:", routes - set(ROUTES), "stale:", set(ROUTES) - routes)
    for route, cases in ROUTES.items():
        assert cases, route


def test_every_product_route_has_a_lattice_case():
    """... and every one of them, with the 16-bit op's, also runs on exact lattice / skip-edge samples (tests/msda_lattice_cases.py,
    judged with msda_ref64's `exact` flag by tests/test_gpu_msda_lattice.py)."""
    import msda_h16_cases as C16
    import msda_lattice_cases as LC
    import test_gpu_msda_bounds as B
    routes = product_routes() | {C16.FWD1, C16.FWD2, C16.FWD4, C16.FWD_GENERIC, C16.BWD, C16.BWD_GENERIC}
    assert routes == set(LC.ROUTES), ("routes without a lattice case:", routes - set(LC.ROUTES), "stale:", set(LC.ROUTES) - routes)
    kinds = {s["kind"] for s in LC.ALL_CASES.values()}
    assert kinds == {"lattice", "nonfinite"}
    for route in (B.FWD_STRIP4, B.FWD_PATCH, B.FWD_WINDOW, B.FWD_GENERIC, C16.FWD4):      # the routes the non-finite kind must reach
        assert any(s["kind"] == "nonfinite" and s["fwd"] == route for s in LC.ALL_CASES.values()), route
