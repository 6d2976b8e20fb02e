"""CPU: the mixed-precision MSDA op's surface and its yardstick (tests/msda_h16_ref.py, tests/msda_h16_cases.py).

  * include/semidetr_hip.h declares the four new entry points, both libraries export them, the ABI version is still 7 and the
    compiled front end has the three new functions;
  * the yardstick is admissible: honest fp32 arithmetic (the C oracle's f32 path) on the up-cast inputs, rounded once, lies
    within the bound on every case and both 16-bit types;
  * and sharp: partial sums rounded to 16 bits after every sample, grad_value rounded per contribution, locations or attention
    rounded to 16 bits, the smallest-weight sample dropped -- each breaks it on at least one case;
  * fp16 range: on every case |ref| + B32 of `out` and `grad_value` stays below 65504, so overflow can never excuse a kernel.
"""
import ctypes
import os
import re

import numpy as np
import pytest

import msda_h16_cases as C
import msda_h16_ref as H
import msda_ref64 as R
import oracle

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("semidetr_msda_forward_h16", "semidetr_msda_backward_h16_workspace_bytes", "semidetr_msda_backward_h16",
               "semidetr_msda_h16_last_kernels")


def test_h16_surface_from_header_to_front_end():
    import semi_detr_amd
    import MultiScaleDeformableAttention as MSDA      # registered by the package import
    header = open(os.path.join(ROOT, "include", "semidetr_hip.h")).read()
    header = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    assert re.search(r"#define\s+SEMIDETR_H16_FP16\s+0\b", header) and re.search(r"#define\s+SEMIDETR_H16_BF16\s+1\b", header)
    csrc = os.path.join(ROOT, "semi-detr_amd", "csrc")
    for so in ("libsemidetr_hip.so", "libsemidetr_hip_exp.so"):
        handle = ctypes.CDLL(os.path.join(csrc, so))
        for name in NEW_SYMBOLS:
            assert hasattr(handle, name), f"{name} missing from {so}"
        assert handle.semidetr_abi_version() == 7
    lib = semi_detr_amd._lib.lib()
    assert lib.semidetr_msda_backward_h16_workspace_bytes(2, 3, 5, 7) == 4 * 2 * 3 * 5 * 7
    assert lib.semidetr_msda_backward_h16_workspace_bytes(2, 0, 5, 7) == 0
    assert isinstance(lib.semidetr_msda_h16_last_kernels(), bytes)
    ext = semi_detr_amd.MultiScaleDeformableAttention._msda_ext
    for fn in ("ms_deform_attn_h16_forward", "ms_deform_attn_h16_backward", "h16_supported"):
        assert callable(getattr(ext, fn)) and getattr(MSDA, fn) is getattr(ext, fn)
    assert ext.abi_version() == 7
    assert semi_detr_amd.MSDeformAttnMixedFunction is semi_detr_amd.ops.functions.MSDeformAttnMixedFunction


def test_h16_host_side_argument_errors_need_no_gpu():
    import semi_detr_amd
    lib = semi_detr_amd._lib.lib()
    p = ctypes.c_void_p(4096)      # never dereferenced: every check below fails on the host before a launch
    assert lib.semidetr_msda_forward_h16(None, 0, None, p, p, p, p, 1, 1, 1, 1, 1, 1, 1, p) == -1
    assert b"null pointer" in lib.semidetr_last_error()
    assert lib.semidetr_msda_forward_h16(None, 2, p, p, p, p, p, 1, 1, 1, 1, 1, 1, 1, p) == -1
    assert b"dtype" in lib.semidetr_last_error()
    assert lib.semidetr_msda_forward_h16(None, 1, p, p, p, p, p, 1, 1, 0, 1, 1, 1, 1, p) == -1
    assert b"positive" in lib.semidetr_last_error()
    assert lib.semidetr_msda_forward_h16(None, 0, p, p, p, p, p, 1, 1 << 30, 8, 32, 1, 1, 1, p) == -2
    assert lib.semidetr_msda_forward_h16(None, 0, p, p, p, p, p, 1, 1, 1, 1, 1, 1, 1, None) == -1
    assert lib.semidetr_msda_backward_h16(None, 1, p, p, p, p, p, p, 1, 1, 1, 1, 1, 1, 1, None, p, p, p) == -1
    assert b"null pointer" in lib.semidetr_last_error()
    assert lib.semidetr_msda_backward_h16(None, 7, p, p, p, p, p, p, 1, 1, 1, 1, 1, 1, 1, p, p, p, p) == -1


def test_h16_front_end_refuses_cpu_tensors():
    import torch
    import semi_detr_amd      # noqa: F401  (registers MultiScaleDeformableAttention)
    import MultiScaleDeformableAttention as MSDA
    v = torch.zeros(1, 4, 2, 2, dtype=torch.bfloat16)
    sh, ls = torch.tensor([[2, 2]]), torch.tensor([0])
    loc, attn = torch.zeros(1, 1, 2, 1, 1, 2), torch.zeros(1, 1, 2, 1, 1)
    with pytest.raises(RuntimeError, match="Not implemented on the CPU"):
        MSDA.ms_deform_attn_h16_forward(v, sh, ls, loc, attn, 64)
    with pytest.raises(RuntimeError, match="Not implemented on the CPU"):
        MSDA.ms_deform_attn_h16_backward(v, sh, ls, loc, attn, torch.zeros(1, 1, 4, dtype=torch.bfloat16), 64)
    assert MSDA.h16_supported(v, loc, attn) is False      # a CPU tensor: not the op's


def test_module_keeps_native_16bit_out_of_the_state_dict():
    import copy
    import pickle
    import semi_detr_amd
    m = semi_detr_amd.MSDeformAttn(64, 2, 2, 2)
    assert m.native_16bit is True and not any("native_16bit" in k for k in m.state_dict())
    m.native_16bit = False
    assert copy.deepcopy(m).native_16bit is False and pickle.loads(pickle.dumps(m)).native_16bit is False
    old = copy.deepcopy(m)
    del old.__dict__["native_16bit"]                        # a module pickled before the attribute existed
    assert pickle.loads(pickle.dumps(old)).native_16bit is True


# ---- the yardstick is admissible

@pytest.mark.parametrize("dtype", C.DTYPES)
@pytest.mark.parametrize("name", sorted(C.CASES))
def test_fp32_oracle_rounded_once_is_within_the_bound(name, dtype):
    c, ref = C.inputs(name, dtype), C.reference(name, dtype)
    out = H.round16(oracle.msda_forward(c["value"], c["shapes"], c["loc"], c["attn"]), dtype)
    worst = [H.check("oracle32 " + name, "out", out, ref["out"])]
    if name == C.ALL_OFFMAP:
        assert not ref["out"].val.any() and not out.any()
    if C.CASES[name]["backward"]:
        gv, gl, ga = oracle.msda_backward(c["value"], c["shapes"], c["loc"], c["attn"], c["gout"])
        worst += [H.check("oracle32 " + name, "grad_value", H.round16(gv, dtype), ref["grad_value"]),
                  H.check("oracle32 " + name, "grad_loc", gl, ref["grad_loc"]),
                  H.check("oracle32 " + name, "grad_attn", ga, ref["grad_attn"])]
    print(name, dtype, ["%.3f" % w for w in worst])


@pytest.mark.parametrize("name", sorted(C.CASES))
def test_fp16_cases_stay_inside_the_finite_range(name):
    """The reference alone must leave room: max(|ref| + B32) < 65504 for both rounded results."""
    ref = C.reference(name, "fp16")
    for key in H.ROUNDED:
        if key in ref:
            reach = float(ref[key].reach().max())
            assert reach < H.MAX16["fp16"], (name, key, reach)


# ---- ... and sharp.  Mutants are stated on the fp64 reference's own terms (what is summed is exact; only the named shortcut is
# taken) and their 16-bit results are rounded once at the end like an honest kernel's.

MUTANT_CASES = ("dec_offmap", "dec_anywhere", "enc_pyr4")


def _samples(c):
    """Per-sample terms of `out` in fp64: (N, Lq, M, L * P, D) = a_s * sum_k c_k v_k, and the attention (N, Lq, M, L * P)."""
    shapes, starts = R._level_table(c["shapes"])
    value = np.asarray(c["value"], np.float64)
    N, S, M, D = value.shape
    loc = np.asarray(c["loc"], np.float64)
    attn = np.asarray(c["attn"], np.float64)
    terms = []
    for n in range(N):
        vflat = np.concatenate([value[n].reshape(S * M, D), np.zeros((1, D))])
        rows, ok, cw = R._geometry(loc[n], shapes[:, 0], shapes[:, 1], starts, M)[:3]
        rows = np.where(ok, rows, S * M)
        terms.append(attn[n][..., None] * np.einsum("...k,...kd->...d", cw, vflat[rows]))
    t = np.stack(terms)
    return t.reshape(*t.shape[:3], -1, D), attn.reshape(*attn.shape[:3], -1)


def _out_partial_sums_rounded(c, dtype):
    terms, _ = _samples(c)
    acc = np.zeros(terms.shape[:3] + terms.shape[4:], np.float32)
    for s in range(terms.shape[3]):
        acc = H.round16(acc.astype(np.float64) + terms[:, :, :, s], dtype)
    return acc.reshape(acc.shape[0], acc.shape[1], -1)


def _grad_value_rounded_per_contribution(c, dtype):
    """grad_value accumulated IN the 16-bit type: the running sum of a row is rounded after every contribution (what a packed
    16-bit atomic does), contributions taken in (query, head, sample, corner) order."""
    shapes, starts = R._level_table(c["shapes"])
    value = np.asarray(c["value"], np.float64)
    N, S, M, D = value.shape
    loc, attn = np.asarray(c["loc"], np.float64), np.asarray(c["attn"], np.float64)
    gout = np.asarray(c["gout"], np.float64).reshape(N, -1, M, D)
    res = np.zeros((N, S * M + 1, D), np.float32)
    for n in range(N):
        rows, ok, cw = R._geometry(loc[n], shapes[:, 0], shapes[:, 1], starts, M)[:3]
        w = (attn[n][..., None] * cw)[ok]                                        # (K,)
        r = rows[ok]
        g = np.broadcast_to(gout[n][:, :, None, None, None, :], ok.shape + (D,))[ok]      # (K, D)
        order = np.argsort(r, kind="stable")
        r, contrib = r[order], (w[:, None] * g)[order]
        first = np.concatenate([[True], r[1:] != r[:-1]])
        rank = np.arange(len(r)) - np.maximum.accumulate(np.where(first, np.arange(len(r)), 0))
        for k in range(int(rank.max()) + 1):
            sel = rank == k
            res[n, r[sel]] = H.round16(res[n, r[sel]].astype(np.float64) + contrib[sel], dtype)
    return res[:, :S * M].reshape(N, S, M, D)


def _drop_smallest(a, c):
    flat = np.abs(a).reshape(*a.shape[:3], -1)
    drop = np.zeros(flat.shape, bool)
    np.put_along_axis(drop, np.argmin(flat, -1)[..., None], True, -1)
    return a, np.where(drop.reshape(a.shape)[..., None], 0.0, c)


def _restated(c, dtype, **change):
    """out and grad_value of the op with one input changed, in fp64, rounded once."""
    r = R.msda(np.asarray(c["value"], np.float64), c["shapes"], change.get("loc", c["loc"]), change.get("attn", c["attn"]),
               np.asarray(c["gout"], np.float64), weights_hook=change.get("hook"))
    return {k: H.round16(r[k].val, dtype) for k in H.ROUNDED}


MUTANTS = {
    "partial_sums_rounded_per_sample": lambda c, dt: dict(out=_out_partial_sums_rounded(c, dt)),
    "grad_value_rounded_per_contribution": lambda c, dt: dict(grad_value=_grad_value_rounded_per_contribution(c, dt)),
    "locations_rounded_to_16_bits": lambda c, dt: _restated(c, dt, loc=H.round16(c["loc"], dt)),
    "attention_rounded_to_16_bits": lambda c, dt: _restated(c, dt, attn=H.round16(c["attn"], dt)),
    "smallest_weight_sample_dropped": lambda c, dt: _restated(c, dt, hook=_drop_smallest),
}


@pytest.mark.parametrize("dtype", C.DTYPES)
@pytest.mark.parametrize("mutant", sorted(MUTANTS))
def test_mutants_break_the_bound(mutant, dtype):
    worst = {}
    for name in MUTANT_CASES:
        c, ref = C.inputs(name, dtype), C.reference(name, dtype)
        for key, got in MUTANTS[mutant](c, dtype).items():
            worst[name, key] = float(ref[key].ratio(got).max())
        if max(worst.values()) > 1.0:
            break
    print(mutant, dtype, {k: "%.3g" % v for k, v in worst.items()})
    assert max(worst.values()) > 1.0, (mutant, dtype, worst)
