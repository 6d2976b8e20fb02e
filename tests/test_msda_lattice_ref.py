"""CPU: the lattice / skip-edge / non-finite cases (tests/msda_lattice_cases.py) and msda_ref64's `exact` flag that
tests/test_gpu_msda_lattice.py judges the kernels by.

  * the inputs are what they claim: every sample flagged exact has an fp32 pixel coordinate equal to the real one bit for bit,
    formed with two roundings or with one, and a fused one has offset +-0;
  * they are meaningful: shares of lattice, skip-edge, last-line, near and far samples per case, no exact sample left out of
    grad_loc, and almost nothing else left out either;
  * the extended reference is the op: equal to the C oracle in fp64 with NO excluded set (grad_loc included), exactly zero
    gradients on every skipped sample; and it can be met: the fp32 oracle lies within the bound on every case;
  * it sees what the suite could not: five wrong rules a rewrite could introduce each break it.
"""
import numpy as np
import pytest

import msda_h16_ref as H
import msda_lattice_cases as LC
import msda_ref64 as R
import oracle

LATTICE = [n for n, s in LC.ALL_CASES.items() if s["kind"] == "lattice"]


def _dtype_of(name):
    return "fp16" if name in LC.H16_CASES else None      # (the 16-bit cases: fp16 here, both types on the GPU)


def _contract_form(name, dtype=None, f32=True):
    """(value with padded pixels zeroed, shapes, loc, attn, gout) as the kernel's sampling core sees them: fused cases through the
    prologue restated in fp64 (f32: then rounded to fp32 -- inside the bound's prologue allowance; exact samples are unchanged)."""
    c = LC.inputs(name, dtype)
    ft = np.float32 if f32 and c["value"].dtype != np.float64 else np.float64
    value = c["value"] if c["mask"] is None else np.where(c["mask"][:, :, None, None], 0, c["value"])
    if c["ref"] is None:
        loc, attn = c["loc"], c["attn"]
    else:
        with np.errstate(invalid="ignore", over="ignore"):
            pro = R.prologue(c["ref"], c["off"], c["logits"], c["shapes"], c["off"].shape[4])
        loc, attn = pro["loc"], pro["attn"]
    return value.astype(ft), c["shapes"], loc.astype(ft), attn.astype(ft), c["gout"].astype(ft)


# ---- the inputs

@pytest.mark.parametrize("name", LATTICE)
def test_exact_samples_carry_no_rounding(name):
    s, c = LC.ALL_CASES[name], LC.inputs(name)
    exact, shp = c["exact"], c["shapes"]
    if s["io"] == "fused":
        assert np.all(c["off"][exact] == 0), "a fused sample is exact only with offset +-0"
        assert np.signbit(c["off"][exact]).any() and not np.signbit(c["off"][exact]).all(), "both +0 and -0 occur"
        l = np.broadcast_to(c["ref"][:, :, None, :, None, :2], exact.shape + (2,))
    else:
        l = c["loc"]
    l32 = l.astype(np.float32)
    assert np.array_equal(l32.astype(np.float64)[exact], l.astype(np.float64)[exact])
    assert exact.mean() > 0.45
    for ax in range(2):
        E = shp[:, 1 - ax].reshape(-1, 1)
        real = l32[..., ax].astype(np.float64) * E - 0.5       # exact in fp64: 24 x 7 bits, then one aligned subtraction
        two = l32[..., ax] * E.astype(np.float32) - np.float32(0.5)
        assert two.dtype == np.float32
        assert np.array_equal(two.astype(np.float64)[exact], real[exact]), "fl(fl(l E) - 0.5) rounds"
        assert np.array_equal(real.astype(np.float32).astype(np.float64)[exact], real[exact]), "l E - 0.5 is no fp32 number"


def _valid(name):
    s, c = LC.ALL_CASES[name], LC.inputs(name)
    fr = LC.MASK_FRACS[:s["N"]] if s["mask"] == "lattice_band" else None
    return LC._valid_extents(c["shapes"], fr, s["N"])


@pytest.mark.parametrize("name", LATTICE)
def test_sample_kinds_are_all_there(name):
    s, c = LC.ALL_CASES[name], LC.inputs(name)
    exact, shp = c["exact"], c["shapes"]
    loc, _ = LC.locations(name)
    x, y = R.pixel_coords(loc, shp)
    skip, sure = LC.skipped(name)
    Hf, Wf = shp[:, 0].reshape(-1, 1), shp[:, 1].reshape(-1, 1)
    on_line = (x == np.round(x)) | (y == np.round(y))
    shares = dict(lattice_on_map=float((exact & ~skip & on_line).mean()), skipped=float(skip.mean()))
    assert shares["lattice_on_map"] >= 0.20 and shares["skipped"] <= 0.45, shares
    assert int(sure.all((-1, -2)).sum()) >= 1, "a row all of whose samples are skipped"
    if LC.is_pow2_pyramid(s["levels"]):
        v = _valid(name)
        Wv, Hv = v[:, None, None, :, None, 0], v[:, None, None, :, None, 1]
        shares["skip_edge"] = float((exact & ((x == -1) | (y == -1) | (x == Wf) | (y == Hf))).mean())
        shares["last_line"] = float((exact & ~skip & ((x == Wv - 1) | (y == Hv - 1))).mean())
        assert shares["skip_edge"] >= 0.03 and shares["last_line"] >= 0.02, shares
        if s["mask"] is not None:      # ... and the first padded line of the masked images
            assert (exact & ~skip & ((x == Wv) & (Wv < Wf) | (y == Hv) & (Hv < Hf))).mean() >= 0.002
    if s["policy"] == "window":
        q = LC._query_pixels(shp)[None, :, None, :, None, :]
        far = np.maximum(np.abs(x - q[..., 0]), np.abs(y - q[..., 1]))[exact]
        shares["near"], shares["far"] = float((far <= 3).mean()), float((far >= 12).mean())
        assert shares["near"] >= 0.05 and shares["far"] >= 0.05, shares
    print(name, {k: round(v, 4) for k, v in shares.items()})


@pytest.mark.parametrize("name", [n for n in LC.ALL_CASES if n not in LATTICE])
def test_non_finite_cases_hold_every_kind(name):
    s, c = LC.ALL_CASES[name], LC.inputs(name)
    arr = c["off"] if s["io"] == "fused" else c["loc"]
    for v in LC.NON_FINITE:
        assert (np.isnan(arr).any() if np.isnan(v) else (arr == np.float32(v)).any()), v
    strange = ~(np.abs(arr) < 1e9).all(-1)
    assert 0.04 < strange.mean() < 0.08
    for k in ("value", "gout", "attn", "logits"):
        if c.get(k) is not None:
            assert np.isfinite(c[k][~c["mask"]] if k == "value" and c["mask"] is not None else c[k]).all(), k
    skip, sure = LC.skipped(name)
    assert sure[strange].all() and int(sure.all((-1, -2)).sum()) >= 1


# ---- the extended reference

@pytest.mark.parametrize("name", list(LC.ALL_CASES))
def test_reference_is_the_op_and_can_be_met(name):
    """One reference per case, three uses: equal to the fp64 oracle everywhere, zero on the skipped samples, and the fp32 oracle
    (16-bit cases: rounded once) within its bound."""
    s, dtype = LC.ALL_CASES[name], _dtype_of(name)
    c = LC.inputs(name, dtype)
    # (nothing may escape from floor / astype / inf - inf at a non-finite sample)
    with np.errstate(invalid="raise", over="raise", divide="raise"):
        ref = LC.reference(name, dtype)
    skip, sure = LC.skipped(name, dtype)
    exact = c["exact"]
    keys = ("out", "grad_value", "grad_loc", "grad_attn") if s["backward"] else ("out",)
    # fp64: no excluded set
    v64 = _contract_form(name, dtype, f32=False)
    want = [oracle.msda_forward(*v64[:4])] + (list(oracle.msda_backward(*v64, parallel=True)) if s["backward"] else [])
    if s["backward"] and c["mask"] is not None:
        want[1][c["mask"]] = 0
    for key, w in zip(keys, want):
        np.testing.assert_allclose(ref[key].val, w.reshape(ref[key].val.shape), rtol=1e-12,
                                   atol=1e-12 * max(1.0, float(np.abs(w).max())), err_msg=(name, key))
    if s["backward"]:
        gl = ref["grad_loc"]
        assert not (gl.skip[..., 0] & exact).any(), "an exact sample is excluded from grad_loc"
        if s["kind"] == "lattice":
            assert gl.skip.mean() <= 1e-3, gl.skip.mean()
        assert not ref["grad_attn"].val[skip].any() and not gl.val[skip].any() and not want[2][skip].any() and not want[3][skip].any()
        # ... and a skipped sample that no kernel can take has no allowance either: the bound there is `tiny`
        assert ref["grad_attn"].bound()[sure].max(initial=0.0) < 1e-30 and gl.bound()[sure].max(initial=0.0) < 1e-30
    dead = sure.all((-1, -2))
    assert not ref["out"].val.reshape(*dead.shape, -1)[dead].any()
    # fp32: within the bound
    v32 = _contract_form(name, dtype)
    dt = np.float64 if v32[0].dtype == np.float64 else np.float32
    got = [oracle.msda_forward(*v32[:4])] + (list(oracle.msda_backward(*v32, parallel=True)) if s["backward"] else [])
    if s["backward"] and c["mask"] is not None:
        got[1][c["mask"]] = 0
    worst = {}
    for key, g in zip(keys, got):
        if dtype is not None:
            worst[key] = H.check("oracle32 " + name, key, H.round16(g, dtype) if key in H.ROUNDED else g, ref[key])
        else:
            worst[key] = R.check("oracle32 " + name, key, g, ref[key], dt)
    if s["io"] == "fused" and s["backward"]:
        pro = ref["prologue"]
        with np.errstate(invalid="ignore", over="ignore"):
            goff = (got[2].astype(np.float64) * pro["scale"]).astype(np.float32)
        worst["grad_offsets"] = R.check("oracle32 " + name, "grad_offsets", goff, ref["grad_offsets"])
        a = v32[3].astype(np.float64).reshape(ref["grad_logits"].val.shape)
        g = got[3].astype(np.float64).reshape(a.shape)
        worst["grad_logits"] = R.check("oracle32 " + name, "grad_logits", (a * (g - (a * g).sum(-1, keepdims=True))).astype(np.float32),
                                       ref["grad_logits"])
    print(name, {k: round(v, 3) for k, v in worst.items()})


def test_defaults_are_untouched_by_the_flag():
    """exact = None: bit-identical to an all-False flag on lattice inputs (the flag alone changes anything), and no finite input
    takes the non-finite branch."""
    c = LC.inputs("generic_d16")
    a = R.msda(c["value"], c["shapes"], c["loc"], c["attn"], c["gout"])
    b = R.msda(c["value"], c["shapes"], c["loc"], c["attn"], c["gout"], exact=np.zeros(c["exact"].shape, bool))
    for k in a:
        for f in ("val", "A", "C"):
            assert np.array_equal(getattr(a[k], f), getattr(b[k], f)), (k, f)
    assert np.array_equal(a["grad_loc"].skip, b["grad_loc"].skip) and a["grad_loc"].skip[c["exact"]].mean() > 0.3
    assert not R.non_finite(c["loc"], c["shapes"]).any()


# ---- mutants: wrong rules at a lattice line, a skip edge, a padded pixel and a non-finite coordinate, stated in fp64 (only the
# named rule differs from the op).  Each must break the bound of at least one result of at least one case.
# With `exact` withheld (the bounded tests' judgement of the very same inputs) non_strict_skip and left_cell_on_a_line pass with
# err / bound 0 on every result -- asserted below: the kink exclusion and the edge allowance hide exactly them.  The other three
# are caught on these inputs with or without the flag (a replicated border moves `out` of ordinary samples too; NaN is NaN): what
# they needed was the inputs -- a weight-0 corner in a NaN-filled padded pixel, a non-finite coordinate -- which no case had.

def _op(value, shapes, loc, attn, gout, rule, mask=None, rows=slice(None)):
    """out, grad_loc, grad_attn of the queries `rows` in fp64 with one rule changed."""
    shapes, starts = R._level_table(shapes)
    N, S, M, D = value.shape
    Hf, Wf = shapes[:, 0].astype(np.float64)[:, None], shapes[:, 1].astype(np.float64)[:, None]
    Hi, Wi = shapes[:, 0][:, None], shapes[:, 1][:, None]
    out, ga, gl = [], [], []
    for n in range(N):
        v = np.asarray(value[n], np.float64)
        pad = np.zeros(S, bool) if mask is None else np.asarray(mask[n], bool)
        lc, a = np.asarray(loc[n, rows], np.float64), np.asarray(attn[n, rows], np.float64)
        with np.errstate(invalid="ignore", over="ignore"):
            x, y = lc[..., 0] * Wf - 0.5, lc[..., 1] * Hf - 0.5
            if rule == "non_finite_clamped":
                bx, by = ~(np.abs(x) <= R.F32_MAX), ~(np.abs(y) <= R.F32_MAX)
                x = np.where(bx, np.clip(np.nan_to_num(x, nan=0.0), 0, Wf - 1), x)
                y = np.where(by, np.clip(np.nan_to_num(y, nan=0.0), 0, Hf - 1), y)
            if rule == "non_strict_skip":
                inside = (x >= -1) & (y >= -1) & (x <= Wf) & (y <= Hf)
            else:
                inside = (x > -1) & (y > -1) & (x < Wf) & (y < Hf)
            x, y = np.where(inside, x, 0.0), np.where(inside, y, 0.0)
        x0, y0 = (np.ceil(x) - 1, np.ceil(y) - 1) if rule == "left_cell_on_a_line" else (np.floor(x), np.floor(y))
        lx, ly = x - x0, y - y0
        val = np.zeros(a.shape + (D,))
        dx, dy = np.zeros(a.shape + (D,)), np.zeros(a.shape + (D,))
        m = np.arange(M).reshape(1, M, 1, 1)
        for i in (0, 1):
            for j in (0, 1):
                cy, cx = (y0 + i).astype(np.int64), (x0 + j).astype(np.int64)
                w = (ly if i else 1 - ly) * (lx if j else 1 - lx)
                wx, wy = (ly if i else 1 - ly) * (1 if j else -1), (lx if j else 1 - lx) * (1 if i else -1)
                use = inside & (cy >= 0) & (cx >= 0) & (cy < Hi) & (cx < Wi)
                if rule == "border_replicated":
                    use, cy, cx = inside, np.clip(cy, 0, Hi - 1), np.clip(cx, 0, Wi - 1)
                pix = np.where(use, starts[:, None] + cy * Wi + cx, 0)
                vk = v[pix, m]
                # (honest: a padded corner reads as zero whatever its weight; the mutant only drops those it has a weight for)
                drop = pad[pix] & (w != 0) if rule == "weight0_times_nan" else pad[pix]
                vk = np.where((use & ~drop)[..., None], vk, 0.0)
                val += w[..., None] * vk
                dx += wx[..., None] * vk
                dy += wy[..., None] * vk
        g = np.asarray(gout[n, rows], np.float64).reshape(a.shape[0], M, 1, 1, D)
        out.append((a[..., None] * val).sum((2, 3)).reshape(a.shape[0], M * D))
        ga.append((g * val).sum(-1))
        gl.append(np.stack([Wf * a * (g * dx).sum(-1), Hf * a * (g * dy).sum(-1)], -1))
    return dict(out=np.stack(out), grad_loc=np.stack(gl), grad_attn=np.stack(ga))


def _rows_of(b, rows):
    cut = lambda z: z[:, rows] if isinstance(z, np.ndarray) and z.ndim > 1 else z      # noqa: E731
    return R.Bounded(cut(b.val), cut(b.A), cut(b.n), cut(b.C), None if b.skip is None else cut(b.skip))


MUTANTS = {      # rule -> (cases, queries judged)
    "non_strict_skip": (("generic_d16", "dec_thin"), slice(None)),
    "left_cell_on_a_line": (("generic_d16", "dec_strip4_bwd8_odd"), slice(None)),
    "border_replicated": (("generic_d16", "dec_thin"), slice(None)),
    "weight0_times_nan": (("patch_fused_mask",), slice(0, None, 8)),
    "non_finite_clamped": (("nf_dec_strip",), slice(None)),
}
HIDDEN_WITHOUT_THE_FLAG = ("non_strict_skip", "left_cell_on_a_line")


def test_the_honest_restatement_passes():
    """_op with no rule changed is the op: the mutants differ from it by their rule alone."""
    for name in ("generic_d16", "dec_strip4_bwd8_odd", "dec_thin", "nf_dec_strip"):
        ref, v = LC.reference(name), _contract_form(name, f32=False)
        for key, got in _op(*v, None).items():
            assert float(ref[key].ratio(got).max()) < 1e-3, (name, key)


@pytest.mark.parametrize("rule", sorted(MUTANTS))
def test_mutants_break_the_bound(rule):
    cases, rows = MUTANTS[rule]
    worst, hidden = {}, {}
    for name in cases:
        c, v = LC.inputs(name), _contract_form(name, f32=False)
        value = v[0] if c["mask"] is None else c["value"].astype(np.float64)      # (the mutant meets the NaN of the padded pixels)
        got = _op(value, *v[1:], rule, mask=c["mask"], rows=rows)
        ref, blind = LC.reference(name), LC.reference(name, with_exact=False)
        for key, g in got.items():
            worst[name, key] = float(_rows_of(ref[key], rows).ratio(g).max())
            hidden[name, key] = float(_rows_of(blind[key], rows).ratio(g).max())
    print(rule, {k: "%.3g" % x for k, x in worst.items()}, "exact withheld:", {k: "%.3g" % x for k, x in hidden.items()})
    assert max(worst.values()) > 1.0, (rule, worst)
    if rule in HIDDEN_WITHOUT_THE_FLAG:
        assert max(hidden.values()) <= 1.0, (rule, hidden)
        assert max(x for (_, key), x in worst.items() if key == "grad_loc") > 1e3, (rule, worst)
