"""CPU: the float64 statement tests/input_proj_ref64.py judged from three sides -- its values against torch's own float64
``F.group_norm`` + flatten / transpose / cat and autograd; torch's fp32 CPU ops admissible on every case of
tests/input_proj_cases.py, so the bounds are not too tight; nine mutations of the formulas rejected, so they are not too loose
-- and the host surface of ``semi_detr_amd.input_proj`` that needs no GPU."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch
from torch import nn
from torch.nn import functional as F

import input_proj_cases as C
import input_proj_ref64 as R


def torch_cpu(case, dtype):
    """the reference's op sequence on the CPU in ``dtype`` -> dict of numpy outputs (mean and rstd from native_group_norm)"""
    xs = [torch.from_numpy(np.array(x)).to(dtype).requires_grad_(True) for x in case["xs"]]
    ws = [torch.from_numpy(np.array(w)).to(dtype).requires_grad_(True) for w in case["weights"]]
    bs = [torch.from_numpy(np.array(b)).to(dtype).requires_grad_(True) for b in case["biases"]]
    eps = float(np.float32(case["eps"]))
    srcs = [F.group_norm(x, 32, w, b, eps) for x, w, b in zip(xs, ws, bs)]
    tokens = torch.cat([s.flatten(2).transpose(1, 2) for s in srcs], 1)
    stats = [torch.native_group_norm(x.detach(), w.detach(), b.detach(), x.shape[0], 256, x.shape[2] * x.shape[3], 32, eps)[1:]
             for x, w, b in zip(xs, ws, bs)]
    got = {"tokens": tokens.detach().numpy(), "mean": torch.stack([s[0] for s in stats], 1).numpy(),
           "rstd": torch.stack([s[1] for s in stats], 1).numpy()}
    outs, grads = [], []
    if case["gy"] is not None:
        outs.append(tokens)
        grads.append(torch.from_numpy(np.array(case["gy"])).to(dtype))
    if case["pos"] is not None:
        q = tokens + torch.from_numpy(np.array(case["pos"])).to(dtype)
        got["q"] = q.detach().numpy()
        if case["gq"] is not None:
            outs.append(q)
            grads.append(torch.from_numpy(np.array(case["gq"])).to(dtype))
    torch.autograd.backward(outs, grads)
    for l, x in enumerate(xs):
        got[f"dx{l}"] = x.grad.numpy()
    got["dweight"], got["dbias"] = np.stack([w.grad.numpy() for w in ws]), np.stack([b.grad.numpy() for b in bs])
    return got


@pytest.mark.parametrize("name", C.names())
def test_statement_equals_torch_float64(name):
    """Both sides evaluate the same real-valued formulas in float64 (the statement's chunked variance is algebraically the plain
    one).  A float64 sum of ``count`` terms is off by at most count * 2^-53 * sum |terms| whatever its order, and
    ``R.float64_rounding`` carries exactly that -- u = 2^-53, every sum as deep as it has terms -- through the statement's own
    tree, element by element: each element's bound comes from its own group's sum |terms| and its own rstd, so an ordinary
    group is held to about 1e-13 and only the group at mean 4096 gets the bound its conditioning asks for.  Either side may be
    off from the real-number result by that much, hence |statement - torch| <= 2 * err; an element without a finite bound
    would make the comparison empty, so there must be none."""
    case, ref = C.cases()[name], C.reference(name)
    got = torch_cpu(case, torch.float64)
    f64 = R.float64_rounding(case)
    for k, v in got.items():
        value, err = f64[k]
        assert np.array_equal(value, ref[k][0]) and np.isfinite(err).all(), (name, k)
        diff = np.abs(v.reshape(value.shape) - value)
        ok = diff <= 2 * err
        assert ok.all(), (name, k, float(diff[~ok].max()), float(err[~ok].min()), int((~ok).sum()))
        print(f"  {name}: {k} max diff {diff.max():.2e}, median bound {2 * np.median(err):.2e}, max bound {2 * err.max():.2e}")
    # not a case-wide figure: the longest group has 16 920 terms of size O(1), so an ordinary token is held to ~1e-11
    assert 2 * np.median(f64["tokens"][1]) < 1e-10


@pytest.mark.parametrize("name", C.names())
def test_torch_fp32_cpu_is_admissible(name):
    case = C.cases()[name]
    rep = R.check_gn_tokens(case, torch_cpu(case, torch.float32), name, C.reference(name))
    print(R.table(name, rep))


@pytest.mark.parametrize("name", C.names())
def test_fp32_evaluation_of_the_statement_is_admissible(name):
    case = C.cases()[name]
    rep = R.check_gn_tokens(case, R.eval_f32(case), name, C.reference(name))
    assert max(rep.values()) <= 1.0


def test_special_groups_have_a_statement():
    for name in ("pyr4_odd", "aligned_vec"):
        ref, case = C.reference(name), C.cases()[name]
        hw = case["shapes"][0][0] * case["shapes"][0][1]
        assert ref["mean"][0][0, 0, 0] == 1.375 and abs(ref["mean"][0][0, 0, 1] - 4096.0) < 1e-2
        assert np.isfinite(ref["rstd"][1][0, 0, :2]).all(), "the constant and the cancellation group have a bound on rstd"
        assert np.all(ref["tokens"][0][0, :hw, 0:8] == case["biases"][0][0:8].astype(np.float64))
    assert R.GROUP_DEPTH == 19 and R.BWD_GROUP_DEPTH == 38 and R.SLOT_DEPTH == 35


# mutant -> (case on which it must be rejected, the output that gives it away)
MUTANT_CASES = {"unbiased_variance": ("pyr4_odd", "rstd"), "eps_outside_sqrt": ("pyr4_odd", "rstd"),
                "one_pass_variance": ("pyr4_odd", "rstd"), "level_params_swapped": ("pyr4_odd", "tokens"),
                "group_of_4_channels": ("aligned_vec", "tokens"), "rows_in_nchw_order": ("one_9x33", "tokens"),
                "gq_dropped": ("pyr4_odd", "dx0"), "dweight_without_xhat": ("levels8", "dweight"),
                "mean_over_hw_only": ("aligned_vec", "tokens")}


@pytest.mark.parametrize("mutant", R.MUTANTS)
def test_mutants_are_rejected(mutant):
    assert set(MUTANT_CASES) == set(R.MUTANTS) and len(R.MUTANTS) == 9
    name, output = MUTANT_CASES[mutant]
    case = C.cases()[name]
    got = R.eval_f32(case, mutant=mutant)
    with pytest.raises(R.Inadmissible, match=output):
        R.check_gn_tokens(case, {output: got[output]}, name, C.reference(name))
    with pytest.raises(R.Inadmissible):
        R.check_gn_tokens(case, got, name, C.reference(name))


def test_one_pass_variance_is_rejected_on_the_cancellation_group_itself():
    for name in ("pyr4_odd", "aligned_vec"):
        case, ref = C.cases()[name], C.reference(name)
        got = R.eval_f32(case, mutant="one_pass_variance")
        only = ref["rstd"][0].copy()
        only[0, 0, 1] = got["rstd"][0, 0, 1]
        with pytest.raises(R.Inadmissible, match=r"rstd\[0, 0, 1\]"):
            R.within("rstd", only, ref["rstd"])


# ------------------------------------------------------------------------------------------------------------------
# host surface without a GPU
# ------------------------------------------------------------------------------------------------------------------
def test_constants_of_the_mirror_the_statement_and_the_header_agree():
    from semi_detr_amd import _lib, input_proj
    assert (input_proj.CHUNK, input_proj.TILE, input_proj.UNIT) == (R.CHUNK, R.TILE, R.UNIT)
    assert C.RAGGED_HW * 8 > 2 * input_proj.CHUNK and C.RAGGED_HW > 3 * input_proj.TILE and C.RAGGED_HW % input_proj.TILE
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "semidetr_hip.h")).read()
    assert int(re.search(r"#define\s+SEMIDETR_GN_MAX_LEVELS\s+(\d+)", header).group(1)) == _lib.GN_MAX_LEVELS == input_proj.MAX_LEVELS
    for n in ("semidetr_gn_tokens_workspace_bytes", "semidetr_gn_tokens_forward", "semidetr_gn_tokens_backward"):
        assert hasattr(_lib.lib(), n) and n in _lib.SIGNATURES


def test_spatial_shapes_and_level_start_index():
    from semi_detr_amd import input_proj
    shapes, starts = input_proj.pyramid_index([(5, 7), (3, 4), (2, 2), (1, 1)], "cpu")
    assert shapes.dtype == torch.long and shapes.tolist() == [[5, 7], [3, 4], [2, 2], [1, 1]]
    assert starts.dtype == torch.long and starts.tolist() == [0, 35, 47, 51]
    x = torch.zeros(1, 256, 4, 6)
    view = input_proj.nchw_view(torch.arange(2 * 30 * 256.).reshape(2, 30, 256), 3, (4, 6))
    assert view.shape == (2, 256, 4, 6) and view[1, 7, 2, 5] == (30 + 3 + 2 * 6 + 5) * 256 + 7 and x.shape[1:] == view.shape[1:]


def test_refusal_reasons_need_no_gpu():
    import semi_detr_amd as s
    x = torch.zeros(2, 256, 3, 4)
    for norm, reason in ((nn.GroupNorm(16, 256), "16 groups"), (nn.GroupNorm(32, 128), "128 channels"),
                         (nn.GroupNorm(32, 256, affine=False), "affine"), (nn.LayerNorm(256), "not nn.GroupNorm")):
        with pytest.raises(NotImplementedError, match=reason):
            s.group_norm_to_tokens([x], [norm])
    with pytest.raises(NotImplementedError, match="eps"):
        s.group_norm_to_tokens([x, x], [nn.GroupNorm(32, 256), nn.GroupNorm(32, 256, eps=1e-6)])
    with pytest.raises(ValueError, match="2 levels, 1 norms"):
        s.group_norm_to_tokens([x, x], [nn.GroupNorm(32, 256)])
    with pytest.raises(RuntimeError, match="must live on the GPU"):
        s.group_norm_to_tokens([x], [nn.GroupNorm(32, 256)])
    with pytest.raises(NotImplementedError, match="9 levels"):
        s.group_norm_to_tokens([x] * 9, [nn.GroupNorm(32, 256)] * 9)


def _host_block(**kw):
    """a block whose pointers all aim at one aligned host buffer: good enough for the checks that precede every launch"""
    from semi_detr_amd import _lib
    buf = (ctypes.c_float * 4096)()
    base = (ctypes.addressof(buf) + 15) & ~15
    p = _lib.GnTokens()
    p.batch, p.levels, p.channels, p.groups, p.eps, p.tokens_per_image = 1, 2, 256, 32, 1e-5, 3
    for l, (hw, start) in enumerate(((2, 0), (1, 2))):
        p.hw[l], p.start[l], p.x_batch_stride[l] = hw, start, 0
        for n in ("x", "weight", "bias", "grad_x"):
            getattr(p, n)[l] = base
    for n in ("tokens", "mean", "rstd", "gy"):
        setattr(p, n, base)
    p.gy_stride[0], p.gy_stride[1] = 768, 256
    for k, v in kw.items():
        if k.endswith("_stride"):
            getattr(p, k)[0], getattr(p, k)[1] = v
        elif isinstance(v, tuple):
            getattr(p, k)[v[0]] = v[1]
        else:
            setattr(p, k, v)
    return p, buf, base


def test_argument_errors_need_no_gpu():
    from semi_detr_amd import _lib
    lib = _lib.lib()

    def err(fn, text, rc=-1, work=1 << 20, **kw):
        p, buf, base = _host_block(**kw)
        got = fn(None, ctypes.byref(p), base, work)
        assert got == rc and text in lib.semidetr_last_error(), (got, lib.semidetr_last_error())

    fwd, bwd = lib.semidetr_gn_tokens_forward, lib.semidetr_gn_tokens_backward
    assert fwd(None, None, None, 0) == -1 and b"null pointer" in lib.semidetr_last_error()
    err(fwd, b"128 channels", channels=128)
    err(fwd, b"16 groups", groups=16)
    err(fwd, b"9 levels", levels=9)
    err(fwd, b"0 levels", levels=0)
    err(fwd, b"q and pos", q=1 << 12)
    err(fwd, b"q and pos", pos=1 << 12)
    err(fwd, b"unknown type code", x_type=3)
    err(fwd, b"neither fp32 nor x_type", out_type=1)
    err(fwd, b"overlap", start=(1, 1))
    err(fwd, b"pass tokens_per_image", tokens_per_image=2)
    err(fwd, b"bad sizes", hw=(0, 0))
    err(fwd, b"workspace", work=8)
    err(bwd, b"gy and gq", gy=None)
    err(bwd, b"grad_x", grad_x=(1, None))
    err(bwd, b"rows of gy", gy_stride=(770, 256))
    err(fwd, b"too large", rc=-2, batch=1 << 12, tokens_per_image=1 << 12)
    p, _, _ = _host_block()
    assert lib.semidetr_gn_tokens_workspace_bytes(ctypes.byref(p), 0) == 2 * 32 * 8        # one chunk per group, (sum, M2)
    assert lib.semidetr_gn_tokens_workspace_bytes(ctypes.byref(p), 1) == 2 * 576 * 4       # one unit per level
    p.channels = 128
    assert lib.semidetr_gn_tokens_workspace_bytes(ctypes.byref(p), 0) == 0 and lib.semidetr_gn_tokens_workspace_bytes(None, 0) == 0
