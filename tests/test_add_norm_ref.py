"""CPU: the float64 statement tests/add_norm_ref64.py judged from both sides -- torch's own fp32 CPU ops
(``F.layer_norm(x + residual) (+ pos)`` and autograd) are admissible on every case of tests/add_norm_cases.py, so the bounds are
not too tight; eight mutations of the formulas are rejected, so they are not too loose -- and the host surface of
``semi_detr_amd.add_norm`` that needs no GPU."""
import ctypes

import numpy as np
import pytest
import torch
from torch import nn
from torch.nn import functional as F

import add_norm_cases as C
import add_norm_ref64 as R


def torch_cpu(case):
    t = {k: None if case[k] is None else torch.from_numpy(np.array(case[k])) for k in ("x", "residual", "pos", "weight", "bias", "gy", "gq")}
    leaves = [t[k].requires_grad_(True) for k in ("x", "residual", "pos", "weight", "bias") if t[k] is not None]
    s = t["x"] if t["residual"] is None else t["x"] + t["residual"]
    y = F.layer_norm(s, (256,), t["weight"], t["bias"], float(np.float32(case["eps"])))
    got = {"y": y.detach().numpy()}
    outs, grads = [], []
    if t["gy"] is not None:
        outs.append(y)
        grads.append(t["gy"])
    if t["pos"] is not None:
        q = y + t["pos"]
        got["q"] = q.detach().numpy()
        if t["gq"] is not None:
            outs.append(q)
            grads.append(t["gq"])
    torch.autograd.backward(outs, grads)
    got["dx"], got["dweight"], got["dbias"] = t["x"].grad.numpy(), t["weight"].grad.numpy(), t["bias"].grad.numpy()
    extra = {"dresidual": None if t["residual"] is None else t["residual"].grad.numpy(),
             "dpos": None if t["pos"] is None or t["pos"].grad is None else t["pos"].grad.numpy()}
    return got, extra


@pytest.mark.parametrize("name", C.names())
def test_torch_fp32_cpu_is_admissible(name):
    case = C.cases()[name]
    got, extra = torch_cpu(case)
    rep = R.check_add_norm(case, got, name, C.reference(name))
    print(R.table(name, rep))
    if extra["dresidual"] is not None:
        assert np.array_equal(extra["dresidual"], got["dx"])
    if extra["dpos"] is not None:
        assert np.array_equal(extra["dpos"], case["gq"])


@pytest.mark.parametrize("name", C.names())
def test_fp32_evaluation_of_the_statement_is_admissible(name):
    case = C.cases()[name]
    rep = R.check_add_norm(case, R.eval_f32(case), name, C.reference(name))
    assert max(rep.values()) <= 1.0


def test_equal_values_row_has_no_spread_in_the_statement():
    ref = C.reference("r3_special_rows")
    case = C.cases()["r3_special_rows"]
    assert np.all(ref["y"][0][0] == case["bias"].astype(np.float64))
    assert ref["mean"][0][0] == 0.75 and abs(ref["mean"][0][1] - 4096.0) < 1e-2


# mutant -> (case on which it must be rejected, the output that gives it away)
MUTANT_CASES = {"unbiased_variance": ("r2051_contiguous", "rstd"), "eps_outside_sqrt": ("r3_special_rows", "rstd"),
                "residual_dropped": ("r65_contiguous", "y"), "pos_before_norm": ("r65_transposed", "y"),
                "one_pass_variance": ("r3_special_rows", "rstd"), "gq_dropped": ("r2051_contiguous", "dx"),
                "dweight_without_xhat": ("r65_contiguous", "dweight"), "mean_g_not_gw": ("r65_contiguous", "dx")}


@pytest.mark.parametrize("mutant", R.MUTANTS)
def test_mutants_are_rejected(mutant):
    assert set(MUTANT_CASES) == set(R.MUTANTS) and len(R.MUTANTS) >= 8
    name, output = MUTANT_CASES[mutant]
    case = C.cases()[name]
    got = R.eval_f32(case, mutant=mutant)
    with pytest.raises(R.Inadmissible, match=output):
        R.check_add_norm(case, {output: got[output]}, name, C.reference(name))
    with pytest.raises(R.Inadmissible):
        R.check_add_norm(case, got, name, C.reference(name))


def test_one_pass_variance_is_rejected_on_the_cancellation_row_itself():
    case = C.cases()["r3_special_rows"]
    got = R.eval_f32(case, mutant="one_pass_variance")
    ref = C.reference("r3_special_rows")
    assert np.isfinite(ref["rstd"][1][1]) and np.isfinite(ref["y"][1][1]).all()        # the statement speaks about that row
    only_row_1 = np.concatenate([ref["rstd"][0][:1], got["rstd"][1:2], ref["rstd"][0][2:]])
    with pytest.raises(R.Inadmissible, match=r"rstd\[1\]"):
        R.within("rstd", only_row_1, ref["rstd"])


# ------------------------------------------------------------------------------------------------------------------
# host surface without a GPU
# ------------------------------------------------------------------------------------------------------------------
SYMBOLS = ("semidetr_add_norm_workspace_bytes", "semidetr_add_norm_forward_f32", "semidetr_add_norm_backward_f32")


def test_library_exports_the_three_symbols_and_signatures_match_the_header():
    import semi_detr_amd
    lib = semi_detr_amd._lib.lib()
    for n in SYMBOLS:                            # their types and the block's layout: tests/test_cabi_mirror.py
        assert hasattr(lib, n) and n in semi_detr_amd._lib.SIGNATURES
    assert lib.semidetr_abi_version() == 7
    assert lib.semidetr_add_norm_workspace_bytes(0) == 0 and lib.semidetr_add_norm_workspace_bytes(2 ** 31) == 0
    assert lib.semidetr_add_norm_workspace_bytes(64) == 2048 and lib.semidetr_add_norm_workspace_bytes(2051) == 33 * 2048


def test_argument_errors_need_no_gpu():
    import semi_detr_amd
    from semi_detr_amd.add_norm import _Params
    lib = semi_detr_amd._lib.lib()
    buf = (ctypes.c_float * 2048)()
    base = (ctypes.addressof(buf) + 15) & ~15

    def block(**kw):
        p = _Params()
        p.rows0, p.rows1, p.dim, p.eps = 1, 2, 256, 1e-5
        for n in ("x", "weight", "bias", "y", "mean", "rstd", "grad_x", "gy"):
            setattr(p, n, base)
        p.x_stride[0], p.x_stride[1], p.gy_stride[0], p.gy_stride[1] = 512, 256, 512, 256
        for k, v in kw.items():
            if k.endswith("_stride"):
                getattr(p, k)[0], getattr(p, k)[1] = v
            else:
                setattr(p, k, v)
        return ctypes.byref(p)

    def err(rc, text):
        assert rc == -1 and text in lib.semidetr_last_error(), (rc, lib.semidetr_last_error())

    err(lib.semidetr_add_norm_forward_f32(None, None, None, 0), b"null pointer")
    err(lib.semidetr_add_norm_forward_f32(None, block(x=None), None, 0), b"null pointer")
    err(lib.semidetr_add_norm_forward_f32(None, block(dim=128), None, 0), b"row width 128")
    err(lib.semidetr_add_norm_forward_f32(None, block(x=base + 4), None, 0), b"16-byte aligned")
    err(lib.semidetr_add_norm_forward_f32(None, block(x_stride=(258, 256)), None, 0), b"16-byte aligned")
    err(lib.semidetr_add_norm_forward_f32(None, block(pos=base), None, 0), b"q and pos")
    err(lib.semidetr_add_norm_backward_f32(None, block(gy=None), None, 0), b"gy and gq")
    err(lib.semidetr_add_norm_backward_f32(None, block(grad_weight=base), base, 2047), b"workspace")
    assert lib.semidetr_add_norm_forward_f32(None, block(rows0=1 << 16, rows1=1 << 15), None, 0) == -2


def test_cpu_tensors_other_widths_and_mismatched_shapes_raise():
    import semi_detr_amd as s
    w, b = torch.ones(256), torch.zeros(256)
    x = torch.zeros(2, 3, 256)
    with pytest.raises(RuntimeError, match="must live on the GPU"):
        s.add_layer_norm(x, x, w, b)
    with pytest.raises(NotImplementedError, match="row width 128"):
        s.add_layer_norm(torch.zeros(2, 3, 128), None, torch.ones(128), torch.zeros(128))
    with pytest.raises(ValueError, match="residual is"):
        s.add_layer_norm(x, torch.zeros(3, 2, 256), w, b)
    with pytest.raises(ValueError, match="pos is"):
        s.add_layer_norm(x, x, w, b, pos=torch.zeros(1, 3, 256))
    with pytest.raises(NotImplementedError):
        s.LayerNorm(128)
    with pytest.raises(NotImplementedError):
        s.LayerNorm(256, elementwise_affine=False)


def test_layer_norm_adopt_keeps_parameters_and_state_dict_keys():
    import semi_detr_amd as s
    ref = nn.LayerNorm(256, eps=1e-6)
    new = s.LayerNorm.adopt(ref)
    assert new.weight is ref.weight and new.bias is ref.bias and new.eps == 1e-6
    assert new.elementwise_affine is True and new.normalized_shape == (256,)
    assert list(new.state_dict()) == list(ref.state_dict()) == ["weight", "bias"]
    fresh = s.LayerNorm(256)
    with torch.no_grad():
        ref.weight.normal_()
    assert fresh.load_state_dict(ref.state_dict(), strict=True).missing_keys == []
    assert torch.equal(fresh.weight, ref.weight)
    with pytest.raises(NotImplementedError):
        s.LayerNorm.adopt(nn.LayerNorm(128))


def test_convert_layer_norms_skips_other_widths_and_non_affine_norms():
    import semi_detr_amd as s
    m = nn.ModuleDict(dict(a=nn.LayerNorm(256), b=nn.LayerNorm(128), c=nn.LayerNorm(256, elementwise_affine=False),
                           d=nn.Sequential(nn.Linear(256, 256), nn.LayerNorm(256)), e=nn.LayerNorm((4, 256))))
    wa, wd = m["a"].weight, m["d"][1].weight
    keys = list(m.state_dict())
    assert s.convert_layer_norms(m) == 2
    assert type(m["a"]) is s.LayerNorm and type(m["d"][1]) is s.LayerNorm and m["a"].weight is wa and m["d"][1].weight is wd
    assert all(type(m[k]) is nn.LayerNorm for k in "bce")
    assert list(m.state_dict()) == keys
    assert s.convert_layer_norms(m) == 0


def test_bind_layer_epilogues_skips_everything_without_detr_od():
    from semi_detr_amd import registry
    try:
        import detr_od  # noqa: F401
        pytest.skip("detr_od is importable here")
    except ImportError:
        pass
    for _ in range(2):
        done, skipped = registry.bind_layer_epilogues()
        assert done == [] and len(skipped) == 7
        assert "DINOTransformerEncoder.forward" in skipped and "DINOTransformerDecoderLayer.forward_sa" in skipped
