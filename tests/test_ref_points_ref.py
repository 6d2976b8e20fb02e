"""CPU: the float64 statement of the reference-point kernels (tests/ref_points_ref64.py) against torch's float64 evaluation of
the restated op sequence (tests/ref_points_torch_restated.py), autograd included; the restatement against the reference's own
``inverse_sigmoid`` and ``gen_sineembed_for_position`` (the fixture tests/golden/ref_points.npz everywhere, the functions
themselves where the checkout is present); torch's fp32 results admissible on every fp32 case; eight deliberate mistakes
rejected; the share of open gradient elements; and the host surface of the new entry points: header, ``_lib`` and library in
agreement, every refusal with its reason.
"""
import ctypes
import importlib.util
import os
import re

import numpy as np
import pytest
import torch

import ref_points_cases as C
import ref_points_ref64 as R
import ref_points_torch_restated as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "ref_points.npz")


def _tool():
    spec = importlib.util.spec_from_file_location("gen_golden_ref_points", os.path.join(ROOT, "tools", "gen_golden_ref_points.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _same(name, a, b, tol=1e-11):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    assert a.shape == b.shape, (name, a.shape, b.shape)
    nan = np.isnan(a)
    assert np.array_equal(nan, np.isnan(b)), name
    with np.errstate(all="ignore"):
        bad = ~nan & ~(np.abs(a - b) <= tol * np.maximum(1.0, np.abs(b)))
    assert not bad.any(), f"{name}: {a[bad][:3]} against {b[bad][:3]}"


# ------------------------------------------------------------------------------------------------------------------
# statement against torch's float64
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", C.names())
def test_statement_equals_torch_float64(name):
    case = C.cases()[name]
    got = T.evaluate(case, torch.float64)
    mode = case["mode"]
    for s, seg in enumerate(case["segments"]):
        ref = R.exact(seg["ref"])
        y = ref if mode == C.NONE else R.refine(mode, R.exact(seg["delta"]) if mode == C.REFINE else None, ref, case["eps"])
        if mode != C.NONE:
            _same(f"new_ref[{s}]", y[0], got["new_ref"][s])
        y, coords, first = R.exact(y[0]), None, s == 0 and case["vr"] is not None
        if first:
            ref_input = R.scale(y, case["vr"])
            _same("ref_input", ref_input[0], got["ref_input"])
            coords = R.exact(ref_input[0][:, :, 0, :])
            _same("embed", R.embed(coords, case["dim_t"])[0], got["embed"])
        stmt, opened = R.grad(mode, y, ref, case["eps"], seg["g_new"], case["vr"], case.get("g_ref_input") if first else None,
                              case.get("g_embed") if first else None, case["dim_t"], coords)
        assert opened == 0
        _same(f"g_ref[{s}]", stmt["g_ref"][0], got["g_ref"][s], 1e-9)
        if mode == C.REFINE:
            _same(f"g_delta[{s}]", stmt["g_delta"][0], got["g_delta"][s], 1e-9)


# ------------------------------------------------------------------------------------------------------------------
# restatement against the reference
# ------------------------------------------------------------------------------------------------------------------
def _restated_outputs(data):
    x = torch.from_numpy(data["x"]).double()
    return {"inv": T.inverse_sigmoid(x).numpy(), "inv_eps3": T.inverse_sigmoid(x, eps=1e-3).numpy(),
            "embed4": T.gen_sineembed_for_position(torch.from_numpy(data["pos4"]).double()).numpy(),
            "embed2": T.gen_sineembed_for_position(torch.from_numpy(data["pos2"]).double()).numpy()}


def test_restatement_equals_the_fixture_of_the_references_functions():
    data = dict(np.load(GOLDEN))
    tool = _tool()
    for k, v in tool.inputs().items():
        assert np.array_equal(v, data[k]), f"the fixture's {k} is not what tools/gen_golden_ref_points.py writes"
    for k, v in _restated_outputs(data).items():
        _same(k, v, data[k], 1e-13)
    with pytest.raises(ValueError, match=r"Unknown pos_tensor shape\(-1\):3"):
        T.gen_sineembed_for_position(torch.zeros(2, 2, 3))


def test_restatement_equals_the_references_functions():
    tool = _tool()
    fns = tool.load_reference()
    if fns is None:
        pytest.skip("no reference checkout on this machine; the fixture above holds its outputs")
    data = tool.inputs()
    want = tool.outputs(fns, data)
    for k, v in _restated_outputs(data).items():
        assert np.array_equal(v, want[k], equal_nan=True), k        # the same ops in the same order: bit for bit
    for dtype in (torch.float32, torch.float64):
        x = torch.from_numpy(data["x"]).to(dtype)
        assert torch.equal(T.inverse_sigmoid(x), fns[0](x))
        assert torch.equal(T.gen_sineembed_for_position(x), fns[1](x))
        assert torch.equal(T.gen_sineembed_for_position(x[..., :2]), fns[1](x[..., :2]))
    with pytest.raises(ValueError, match=r"Unknown pos_tensor shape\(-1\):3"):
        fns[1](torch.zeros(2, 2, 3))


# ------------------------------------------------------------------------------------------------------------------
# admissibility, mutations, open elements
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", C.fp32_names())
def test_torch_fp32_is_admissible(name):
    case = C.cases()[name]
    ratios = R.check(case, T.evaluate(case, torch.float32), name)
    print(R.table(name, ratios))


def test_the_embed_bound_is_not_slack():
    """torch's fp32 embedding of 4000 random and special coordinates against float64: inside the bound, and within an order
    of magnitude of it"""
    rng = np.random.default_rng(7)
    coords = rng.random((1000, 1, 4)).astype(np.float32)
    coords.reshape(-1)[:6] = C.SPECIAL_COORDS
    got = T.gen_sineembed_for_position(torch.from_numpy(coords)).numpy()
    a = R.embed(R.exact(coords), C.table())
    R.within("embed", got, a)
    worst = R.ratio(got, a)
    print(f"  torch fp32 embed: worst |diff| / bound = {worst:.2f}")
    assert 0.1 < worst <= 1.0


MUTANT_CASE = {"sin_cos_swapped": "none_q65_b2_l4_w4_special", "xy_block_order": "none_q65_b2_l4_w4_special",
               "dim_t_j": "none_q65_b2_l4_w4_special", "ratio_after_embed": "none_q65_b2_l4_w4_special",
               "w_by_vr1": "none_q65_b2_l4_w4_special", "no_eps": "refine_q3_b3_l5_w4_special",
               "eps_on_x2_only": "refine_q3_b3_l5_w4_special", "clamp_grad_exclusive": "refine_q3_b3_l5_w4_special"}


@pytest.mark.parametrize("mutant", T.MUTANTS)
def test_mutation_is_rejected(mutant):
    assert len(T.MUTANTS) >= 8 and set(MUTANT_CASE) == set(T.MUTANTS)
    case = C.cases()[MUTANT_CASE[mutant]]
    R.check(case, T.evaluate(case, torch.float32), "unmutated")
    with pytest.raises(R.Inadmissible):
        R.check(case, T.evaluate(case, torch.float32, mutant=mutant), mutant)


def test_the_statement_can_be_mutated_too():
    """the statement with the exclusive clamp gradient rejects torch's (inclusive) gradient at the tie x == eps"""
    case = C.cases()["refine_q3_b3_l5_w4_special"]
    assert any((seg["ref"] == np.float32(C.EPS32)).any() for seg in case["segments"])
    with pytest.raises(R.Inadmissible, match="g_ref"):
        R.check(case, T.evaluate(case, torch.float32), "exclusive", mutant="clamp_grad_exclusive")


def test_open_gradient_elements_on_the_random_cases():
    assert len(C.random_names()) >= 4
    for name in C.random_names():
        case = C.cases()[name]
        ratios = R.check(case, T.evaluate(case, torch.float32), name)
        assert ratios["elements"] > 0 and ratios["open"] <= 0.01 * ratios["elements"], (name, ratios)


def test_a_straddled_kink_is_open_and_admits_both_branches():
    eps = C.EPS32
    ref = (np.asarray([[[eps, 0.5]]], np.float64), np.asarray([[[1e-9, 0.0]]], np.float64))      # eps +- 1e-9; 0.5 exact
    sl, opened = R.slope(ref, eps)
    assert opened.tolist() == [[[True, False]]]
    lo, hi = sl[0] - sl[1], sl[0] + sl[1]
    assert lo[0, 0, 0] <= 1.0 / (1.0 - eps) and hi[0, 0, 0] >= 1.0 / eps + 1.0 / (1.0 - eps)
    assert abs(sl[0][0, 0, 1] - 4.0) < 1e-12 and sl[1][0, 0, 1] < 1e-5


# ------------------------------------------------------------------------------------------------------------------
# host surface
# ------------------------------------------------------------------------------------------------------------------
def test_header_lib_and_library_agree_on_the_new_entry_points():
    from semi_detr_amd import _lib
    header = open(os.path.join(ROOT, "include", "semidetr_hip.h")).read()
    for macro, value in [("SEMIDETR_REF_MAX_SEGMENTS", _lib.REF_MAX_SEGMENTS), ("SEMIDETR_REF_MAX_LEVELS", _lib.REF_MAX_LEVELS)] + \
            list(_lib.REF_MODES.items()):
        assert int(re.search(r"#define\s+%s\s+(\d+)" % macro, header).group(1)) == value, macro
    assert int(re.search(r"#define\s+SEMIDETR_ABI_VERSION\s+(\d+)", header).group(1)) == 7 == _lib.lib().semidetr_abi_version()
    for fn in ("semidetr_ref_points_forward", "semidetr_ref_points_backward"):
        assert re.search(r"int %s\(void \*stream, const semidetr_ref_points \*params" % fn, header)
        res, args = _lib.SIGNATURES[fn]
        assert res is ctypes.c_int and args == [ctypes.c_void_p, ctypes.POINTER(_lib.RefPoints)]
        assert getattr(_lib.lib(), fn).argtypes == args
    assert _lib.STRUCTS["semidetr_ref_points"] is _lib.RefPoints and _lib.STRUCTS["semidetr_ref_segment"] is _lib.RefSegment
    assert ctypes.sizeof(_lib.RefPoints) == 80 + 8 * ctypes.sizeof(_lib.RefSegment)


def _block(**kw):
    """a block the library accepts up to the launch (fake, aligned, never dereferenced on the host), then ``kw`` over it"""
    from semi_detr_amd import _lib
    p = _lib.RefPoints()
    p.width, p.mode, p.num_segments, p.levels, p.eps = 4, 2, 1, 0, 1e-5
    sg = p.segment[0]
    sg.rows0, sg.rows1 = 3, 2
    sg.delta = sg.ref = sg.new_ref = sg.g_new = sg.g_delta = sg.g_ref = 4096
    for st in (sg.delta_stride, sg.ref_stride, sg.new_ref_stride, sg.g_new_stride):
        st[0], st[1] = 8, 4
    for k, v in kw.items():
        obj, _, field = k.rpartition("__")
        target = p if not obj else p.segment[0]
        if isinstance(v, tuple):
            arr = getattr(target, field)
            arr[0], arr[1] = v
        else:
            setattr(target, field, v)
    return p


REFUSALS = [
    (dict(width=3), "width 3 (2 and 4 are built)"),
    (dict(mode=7), "unknown mode 7"),
    (dict(num_segments=9), "9 segments (1 .. 8)"),
    (dict(num_segments=0), "0 segments (1 .. 8)"),
    (dict(eps=float("nan")), "eps is NaN or negative"),
    (dict(ref_type=5), "unknown type code"),
    (dict(delta_type=1, ref_type=1, out_type=2), "out_type 2 is neither fp32 nor the operands' common type 1"),
    (dict(delta_type=1, ref_type=2, out_type=1), "out_type 1 is neither fp32 nor the operands' common type 0"),
    (dict(valid_ratios=4096, levels=9, ref_input=4096), "9 levels (1 .. 8)"),
    (dict(valid_ratios=4096, levels=4, ref_input=4096, num_segments=2), "scale and embed take one segment, not 2"),
    (dict(valid_ratios=4096, levels=4), "ref_input null or misaligned", "forward"),
    (dict(valid_ratios=4096, levels=4, ref_input=4096, embed=4096), "embed needs dim_t", "forward"),
    (dict(valid_ratios=4096, levels=4, ref_input=4096, embed=4100, dim_t=4096), "embed needs dim_t, both 16-byte aligned", "forward"),
    (dict(embed=4096), "need valid_ratios"),
    (dict(levels=2), "need valid_ratios"),
    (dict(seg__rows0=0), "bad sizes (segment 0: rows0=0 rows1=2)"),
    (dict(seg__rows0=1 << 20, seg__rows1=1 << 10), "too large (segment 0"),
    (dict(seg__ref=0), "null pointer (ref of segment 0)"),
    (dict(seg__delta=0), "null pointer (delta of segment 0)"),
    (dict(seg__new_ref=0), "null pointer (new_ref of segment 0)"),
    (dict(seg__ref=4098), "ref of segment 0 must be aligned"),
    (dict(seg__delta_stride=(-8, 4)), "delta of segment 0 must be aligned to its element, with non-negative strides"),
]


@pytest.mark.parametrize("refusal", REFUSALS, ids=[r[1][:40] for r in REFUSALS])
def test_the_library_refuses_with_the_reason(refusal):
    """(a block that is not refused would be launched with its fake pointers: every entry is refused by the functions it names,
    on the host, before anything else happens)"""
    from semi_detr_amd import _lib
    lib = _lib.lib()
    kw, reason = refusal[:2]
    p = _block(**kw)
    fns = (lib.semidetr_ref_points_forward,) + ((lib.semidetr_ref_points_backward,) if len(refusal) == 2 else ())
    for fn in fns:
        rc = fn(None, ctypes.byref(p))
        assert rc != 0 and reason in lib.semidetr_last_error().decode(), (rc, lib.semidetr_last_error())
    assert lib.semidetr_ref_points_forward(None, None) == -1 and b"null pointer (parameter block)" in lib.semidetr_last_error()


def test_the_backward_refuses_a_launch_without_a_gradient():
    from semi_detr_amd import _lib
    lib = _lib.lib()
    assert lib.semidetr_ref_points_backward(None, ctypes.byref(_block(seg__g_new=0))) != 0
    assert b"no upstream gradient for segment 0" in lib.semidetr_last_error()
    assert lib.semidetr_ref_points_backward(None, ctypes.byref(_block(seg__g_ref=0, seg__g_delta=0))) != 0
    assert b"no gradient wanted from segment 0" in lib.semidetr_last_error()


def test_the_mirror_refuses_what_it_does_not_cover():
    import semi_detr_amd as s
    from semi_detr_amd import ref_points
    with pytest.raises(ValueError, match=r"Unknown pos_tensor shape\(-1\):3"):
        s.gen_sineembed_for_position(torch.zeros(2, 2, 3))
    dec = T.Decoder(num_layers=1)
    args = (torch.zeros(3, 1, 256), torch.zeros(5, 1, 256))
    for attr, value, reason in [("deformable_decoder", False, "deformable_decoder=False"),
                                ("query_pos_sine_scale", T.MLP(256, 256, 256, 2), "query_pos_sine_scale"),
                                ("ref_anchor_head", T.MLP(256, 256, 2, 2), "modulate_hw_attn"),
                                ("dec_layer_dropout_prob", [0.1], "dec_layer_dropout_prob"), ("rm_detach", ["dec"], "rm_detach")]:
        old = getattr(dec, attr)
        setattr(dec, attr, value)
        with pytest.raises(NotImplementedError, match=reason):
            s.decoder_forward(dec, *args, refpoints_unsigmoid=torch.zeros(3, 1, 4), valid_ratios=torch.ones(1, 4, 2))
        setattr(dec, attr, old)
    ref, vr = torch.rand(3, 2, 4), torch.ones(2, 4, 2)
    with pytest.raises(NotImplementedError, match=r"9 levels \(1 \.\. 8\)"):
        s.reference_inputs(ref, torch.ones(2, 9, 2))
    with pytest.raises(NotImplementedError, match="valid_ratios requires grad"):
        s.reference_inputs(ref, vr.clone().requires_grad_(True))
    with pytest.raises(NotImplementedError, match="valid_ratios is torch.float16"):
        s.reference_inputs(ref, vr.half())
    with pytest.raises(NotImplementedError, match=r"\(rows0, rows1, 2 or 4\) is built"):
        s.refine_boxes(torch.rand(3, 2, 3), torch.rand(3, 2, 3))
    with pytest.raises(NotImplementedError, match="torch.float64"):
        s.refine_boxes(ref.double(), ref.double())
    with pytest.raises(NotImplementedError, match=r"9 layers \(1 \.\. 8 segments\)"):
        s.box_outputs([torch.nn.Identity()] * 9, [ref] * 9, [ref] * 10)
    with pytest.raises(RuntimeError, match="must live on the GPU"):
        s.refine_boxes(ref, ref)
    assert ref_points.out_dtype(ref_points.REFINE, torch.float16, torch.float32) == torch.float32
    assert ref_points.out_dtype(ref_points.REFINE, torch.float16, torch.bfloat16) == torch.float32
    assert ref_points.out_dtype(ref_points.REFINE, torch.bfloat16, torch.bfloat16) == torch.bfloat16
    assert ref_points.out_dtype(ref_points.SIGMOID, None, torch.float16) == torch.float16
