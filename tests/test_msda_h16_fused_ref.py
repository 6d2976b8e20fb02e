"""CPU: the surface of the fused prologue / epilogue on a 16-bit value map and its yardstick (tests/msda_h16_fused_ref.py,
tests/msda_h16_fused_cases.py).

  * include/semidetr_hip.h declares the two entry points, `_lib.SIGNATURES` mirrors them, both libraries export them, the ABI version
    is still 7, the compiled front end has the three new functions; the host-side argument errors need no GPU;
  * `MSDeformAttn.fuse_prologue_16bit` is a plain attribute: off by default, not in the state_dict, kept by deepcopy / pickle,
    defaulted for a module pickled before it existed;
  * the yardstick is admissible: an honest fp32 prologue + the C oracle's fp32 op + an fp32 epilogue on the up-cast operands, each
    16-bit result rounded once, lies within the bound on every case; fewer than 2 % of grad_offsets are excluded by the reference's
    kink rule; and on every fp16 case |ref| + B32 of every rounded result stays below 65504, so overflow never excuses a kernel;
  * and sharp: offsets x scale rounded to 16 bits before the add (torch's autocast sequence), softmax weights rounded to 16 bits,
    grad_logits without the sum_j a_j g_j term, a 16-bit gradient rounded twice through the other 16-bit type -- each leaves the
    bound on every case it applies to.
"""
import copy
import ctypes
import os
import pickle
import re

import numpy as np
import pytest

import msda_h16_fused_cases as C
import msda_h16_fused_ref as F
import msda_h16_ref as H
import msda_ref64 as R
import oracle

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("semidetr_msda_fused_forward_h16", "semidetr_msda_fused_backward_h16")
H16_COMBOS = [c for c in C.COMBOS if c[1] == "h16"]


def test_fused_h16_surface_from_header_to_front_end():
    import semi_detr_amd
    import MultiScaleDeformableAttention as MSDA      # registered by the package import
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "semidetr_hip.h")).read(), flags=re.S)
    assert re.search(r"#define\s+SEMIDETR_ABI_VERSION\s+7\b", header)
    for name in NEW_SYMBOLS:
        assert re.search(r"^int\s+%s\s*\(" % name, header, flags=re.M), name
        assert name in semi_detr_amd._lib.SIGNATURES
    fwd, bwd = (semi_detr_amd._lib.SIGNATURES[n][1] for n in NEW_SYMBOLS)
    assert len(fwd) == 19 and len(bwd) == 23 and fwd[9] is ctypes.c_int and bwd[10] is ctypes.c_int      # prologue_type
    csrc = os.path.join(ROOT, "semi-detr_amd", "csrc")
    for so in ("libsemidetr_hip.so", "libsemidetr_hip_exp.so"):
        handle = ctypes.CDLL(os.path.join(csrc, so))
        for name in NEW_SYMBOLS:
            assert hasattr(handle, name), f"{name} missing from {so}"
        assert handle.semidetr_abi_version() == 7
    ext = semi_detr_amd.MultiScaleDeformableAttention._msda_ext
    for fn in ("ms_deform_attn_h16_fused_forward", "ms_deform_attn_h16_fused_backward", "fused_h16_supported"):
        assert callable(getattr(ext, fn)) and getattr(MSDA, fn) is getattr(ext, fn)
    assert semi_detr_amd.MSDeformAttnMixedFusedFunction is semi_detr_amd.ops.functions.MSDeformAttnMixedFusedFunction


def test_fused_h16_host_side_argument_errors_need_no_gpu():
    import semi_detr_amd
    L = semi_detr_amd._lib
    lib = L.lib()
    F32, FP16, BF16 = (L.ROW_TYPES["SEMIDETR_ROW_" + n] for n in ("F32", "FP16", "BF16"))
    p = ctypes.c_void_p(4096)      # never dereferenced: every check below fails on the host before a launch
    dims = (2, 100, 8, 32, 4, 10, 4)      # batch, spatial_size, num_heads, channels, num_levels, num_query, num_point

    def fwd(dtype=0, value=p, ref=p, ref_dim=2, off=p, logits=p, ptype=FP16, dims=dims, out=p):
        return lib.semidetr_msda_fused_forward_h16(None, dtype, value, p, p, ref, ref_dim, off, logits, ptype, None, *dims, out)

    def bwd(dtype=0, ptype=FP16, dims=dims, ws=p, goff=p):
        return lib.semidetr_msda_fused_backward_h16(None, dtype, p, p, p, p, p, 2, p, p, ptype, None, *dims, ws, p, goff, p)

    assert fwd(value=None) == -1 and b"null pointer" in lib.semidetr_last_error()
    assert fwd(ref=None) == -1 and b"null pointer" in lib.semidetr_last_error()
    assert fwd(dtype=2) == -1 and b"dtype" in lib.semidetr_last_error()
    # prologue_type: fp32 or the 16-bit type of dtype; the other 16-bit type and any other code are refused
    for dtype, ptype in ((0, BF16), (1, FP16), (0, 3), (1, -1)):
        assert fwd(dtype=dtype, ptype=ptype) == -1 and b"prologue_type" in lib.semidetr_last_error(), (dtype, ptype)
        assert bwd(dtype=dtype, ptype=ptype) == -1 and b"prologue_type" in lib.semidetr_last_error(), (dtype, ptype)
    assert fwd(ref_dim=3) == -1 and b"ref_dim" in lib.semidetr_last_error()
    # there is no generic fused kernel: channels != 32, more than 32 heads, more than 64 samples per row, a misaligned operand
    for bad in ((2, 100, 8, 16, 4, 10, 4), (2, 100, 33, 32, 4, 10, 4)):
        assert fwd(dims=bad) == -1 and b"no generic fused kernel" in lib.semidetr_last_error(), bad
    assert fwd(dims=(2, 100, 8, 32, 5, 10, 13)) == -1 and b"64 samples" in lib.semidetr_last_error()
    for kw in (dict(off=ctypes.c_void_p(4100)), dict(logits=ctypes.c_void_p(4098)), dict(value=ctypes.c_void_p(4100)),
               dict(out=ctypes.c_void_p(4100)), dict(ref=ctypes.c_void_p(4100))):
        assert fwd(**kw) == -1 and b"aligned" in lib.semidetr_last_error(), kw
    assert fwd(dims=(2, 100, 0, 32, 4, 10, 4)) == -1 and b"positive" in lib.semidetr_last_error()
    assert fwd(dims=(1, 1 << 30, 8, 32, 1, 1, 1)) == -2
    assert bwd(ws=None) == -1 and b"null pointer" in lib.semidetr_last_error()
    assert bwd(goff=ctypes.c_void_p(4100)) == -1 and b"aligned" in lib.semidetr_last_error()
    for ok_pair in ((0, F32), (1, F32), (0, FP16), (1, BF16)):      # accepted pairings get past the type check (and fail later)
        assert fwd(dtype=ok_pair[0], ptype=ok_pair[1], out=ctypes.c_void_p(4100)) == -1 and b"aligned" in lib.semidetr_last_error()


def test_fused_h16_front_end_refuses_cpu_tensors():
    import torch
    import semi_detr_amd      # noqa: F401  (registers MultiScaleDeformableAttention)
    import MultiScaleDeformableAttention as MSDA
    v = torch.zeros(1, 4, 2, 32, dtype=torch.bfloat16)
    sh, ls = torch.tensor([[2, 2]]), torch.tensor([0])
    ref, off, lg = torch.zeros(1, 1, 1, 2), torch.zeros(1, 1, 2, 1, 1, 2, dtype=torch.bfloat16), torch.zeros(1, 1, 2, 1, dtype=torch.bfloat16)
    with pytest.raises(RuntimeError, match="Not implemented on the CPU"):
        MSDA.ms_deform_attn_h16_fused_forward(v, sh, ls, ref, off, lg)
    with pytest.raises(RuntimeError, match="Not implemented on the CPU"):
        MSDA.ms_deform_attn_h16_fused_backward(v, sh, ls, ref, off, lg, torch.zeros(1, 1, 64, dtype=torch.bfloat16))
    assert MSDA.fused_h16_supported(v, ref, off, lg) is False      # a CPU tensor: not the op's


def test_module_keeps_fuse_prologue_16bit_out_of_the_state_dict():
    import semi_detr_amd
    m = semi_detr_amd.MSDeformAttn(64, 2, 2, 2)
    assert m.fuse_prologue_16bit is False and not any("fuse_prologue_16bit" in k for k in m.state_dict())
    m.fuse_prologue_16bit = True
    assert copy.deepcopy(m).fuse_prologue_16bit is True and pickle.loads(pickle.dumps(m)).fuse_prologue_16bit is True
    old = copy.deepcopy(m)
    del old.__dict__["fuse_prologue_16bit"]                 # a module pickled before the attribute existed
    assert pickle.loads(pickle.dumps(old)).fuse_prologue_16bit is False
    assert not any("fuse_prologue_16bit" in k for k in old.state_dict())


# ---- the yardstick is admissible

def _scale32(c):
    """d loc / d offset per coordinate in fp32, broadcastable to the offsets: (1 / W, 1 / H), or 0.5 / P x the box's (w, h)."""
    f = np.float32
    shp = np.asarray(c["shapes"])
    P = c["off"].shape[4]
    if c["ref"].shape[-1] == 2:
        return (f(1) / np.stack([shp[:, 1], shp[:, 0]], -1).astype(f))[None, None, None, :, None, :]
    return (f(0.5) / f(P)) * np.asarray(c["ref"], f)[:, :, None, :, None, 2:]


def _fp32_model(c, backward):
    """The contract restated in honest fp32 arithmetic: softmax and locations in float32 (numpy), the op by the C oracle's fp32
    path on the masked value map, the epilogue in float32.  Nothing is rounded to 16 bits here."""
    f = np.float32
    off, lg, ref = np.asarray(c["off"], f), np.asarray(c["logits"], f), np.asarray(c["ref"], f)
    N, Lq, M, L, P, _ = off.shape
    e = np.exp(lg - lg.max(-1, keepdims=True), dtype=f)
    a = (e / e.sum(-1, keepdims=True, dtype=f)).astype(f)
    scale = _scale32(c).astype(f)
    loc = (ref[:, :, None, :, None, :2] + off * scale).astype(f)
    value = np.array(c["value"], f)
    if c["mask"] is not None:
        value[c["mask"]] = 0
    attn = a.reshape(N, Lq, M, L, P)
    res = dict(out=oracle.msda_forward(value, c["shapes"], loc, attn))
    if backward:
        gv, gl, ga = oracle.msda_backward(value, c["shapes"], loc, attn, np.asarray(c["gout"], f))
        if c["mask"] is not None:
            gv = np.where(c["mask"][:, :, None, None], f(0), gv)
        g = ga.reshape(a.shape).astype(f)
        dot = (a * g).sum(-1, keepdims=True, dtype=f)
        res.update(grad_value=gv, grad_offsets=(gl * scale).astype(f), grad_logits=(a * (g - dot)).astype(f))
    return res


def _rounded_once(res, dtype, prologue_type):
    return {k: (H.round16(v, dtype) if k in F.rounded_keys(prologue_type) else v) for k, v in res.items()}


@pytest.mark.parametrize("dtype,prologue_type", C.COMBOS)
@pytest.mark.parametrize("name", list(C.CASES))
def test_fp32_model_rounded_once_is_within_the_bound(name, dtype, prologue_type):
    c, ref = C.inputs(name, dtype, prologue_type), C.reference(name, dtype, prologue_type)
    got = _rounded_once(_fp32_model(c, C.CASES[name]["backward"]), dtype, prologue_type)
    worst = {k: float(ref[k].ratio(v).max()) for k, v in got.items()}
    print(name, dtype, prologue_type, {k: "%.3f" % w for k, w in worst.items()})
    for k, v in got.items():
        F.check("fp32 model " + name, k, v, ref[k])
    if c["mask"] is not None and "grad_value" in got:
        assert not ref["grad_value"].val[c["mask"]].any() and not got["grad_value"][c["mask"]].any()


@pytest.mark.parametrize("dtype,prologue_type", C.COMBOS)
@pytest.mark.parametrize("name", [n for n, s in C.CASES.items() if s["backward"]])
def test_few_offset_gradients_are_excluded(name, dtype, prologue_type):
    share = float(C.reference(name, dtype, prologue_type)["grad_offsets"].skip.mean())
    assert share < 0.02, (name, share)


@pytest.mark.parametrize("name", list(C.CASES))
def test_fp16_cases_stay_inside_the_finite_range(name):
    """The reference alone must leave room: max(|ref| + B32) < 65504 for every rounded result."""
    ref = C.reference(name, "fp16", "h16")
    for key in F.rounded_keys("h16"):
        if key in ref:
            reach = float(ref[key].reach().max())
            assert reach < H.MAX16["fp16"], (name, key, reach)


# ---- ... and sharp.  Mutants are stated on the fp64 reference's own terms (only the named shortcut is taken) and their 16-bit
# results are rounded once at the end like an honest kernel's.

def _out_with(c, dtype, loc=None, attn=None):
    pro = R.prologue(c["ref"], c["off"], c["logits"], c["shapes"], c["off"].shape[4])
    r = R.msda(np.asarray(c["value"], np.float64), c["shapes"], pro["loc"] if loc is None else loc(pro),
               pro["attn"] if attn is None else attn(pro), mask=c["mask"])
    return dict(out=H.round16(r["out"].val, dtype))


def _autocast_locations(c, dtype):
    """torch's autocast sequence: offsets / normalizer formed (and rounded) in 16 bits, then added to the fp32 reference points"""
    def loc(pro):
        ref = np.asarray(c["ref"], np.float64)[:, :, None, :, None, :2]
        return ref + H.round16(np.asarray(c["off"], np.float64) * pro["scale"], dtype).astype(np.float64)
    return _out_with(c, dtype, loc=loc)


def _weights_rounded(c, dtype):
    return _out_with(c, dtype, attn=lambda pro: H.round16(pro["attn"], dtype).astype(np.float64))


def _grad_logits_without_dot(c, dtype, ref):
    a = ref["prologue"]["attn"]
    return dict(grad_logits=H.round16((a * ref["grad_attn"].val).reshape(ref["grad_logits"].val.shape), dtype))


def _gradients_rounded_twice(c, dtype, ref):
    other = "bf16" if dtype == "fp16" else "fp16"
    return {k: H.round16(H.round16(ref[k].val, other), dtype) for k in ("grad_value", "grad_offsets", "grad_logits")}


FORWARD_MUTANTS = {"offsets_x_scale_rounded_to_16_bits": _autocast_locations, "softmax_weights_rounded_to_16_bits": _weights_rounded}
BACKWARD_MUTANTS = {"grad_logits_without_the_dot": _grad_logits_without_dot, "gradient_rounded_twice": _gradients_rounded_twice}


@pytest.mark.parametrize("dtype,prologue_type", H16_COMBOS)
@pytest.mark.parametrize("name", list(C.CASES))
@pytest.mark.parametrize("mutant", sorted(FORWARD_MUTANTS))
def test_forward_mutants_leave_the_bound(mutant, name, dtype, prologue_type):
    c, ref = C.inputs(name, dtype, prologue_type), C.reference(name, dtype, prologue_type)
    worst = {k: float(ref[k].ratio(v).max()) for k, v in FORWARD_MUTANTS[mutant](c, dtype).items()}
    print(mutant, name, dtype, {k: "%.3g" % v for k, v in worst.items()})
    assert max(worst.values()) > 1.0, (mutant, name, dtype, worst)


@pytest.mark.parametrize("dtype,prologue_type", H16_COMBOS)
@pytest.mark.parametrize("name", [n for n, s in C.CASES.items() if s["backward"]])
@pytest.mark.parametrize("mutant", sorted(BACKWARD_MUTANTS))
def test_backward_mutants_leave_the_bound(mutant, name, dtype, prologue_type):
    c, ref = C.inputs(name, dtype, prologue_type), C.reference(name, dtype, prologue_type)
    worst = {k: float(ref[k].ratio(v).max()) for k, v in BACKWARD_MUTANTS[mutant](c, dtype, ref).items()}
    print(mutant, name, dtype, {k: "%.3g" % v for k, v in worst.items()})
    assert max(worst.values()) > 1.0, (mutant, name, dtype, worst)
