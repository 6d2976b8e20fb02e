"""GPU: the fused prologue / epilogue on a 16-bit value map (semidetr_msda_fused_forward_h16 / _backward_h16) from the compiled front
end up to MSDeformAttn.fuse_prologue_16bit.

Every case of tests/msda_h16_fused_cases.py, for fp16 and bf16 with 16-bit offsets / logits and for bf16 with fp32 ones, against the
fp64 fused reference on the exactly up-cast operands with the bound of tests/msda_h16_fused_ref.py (msda_ref64.fused's fp32 bounds +
the one rounding of each 16-bit result; no per-test factor); the kernel instance each case names; dtypes; exact zeros of grad_value at
padded pixels; mask None against an all-False mask; the front end's argument errors; and the module's opt-in route under autocast
(bf16, fp16) and as a .half() module, with the helpers of tests/test_gpu_msda_h16.py.

Run with -s to see the worst err / bound of every result.
"""
from unittest import mock

import numpy as np
import pytest
import torch

import msda_h16_cases as C16
import msda_h16_fused_cases as C
import msda_h16_fused_ref as F
import msda_h16_ref as H
import test_gpu_msda_h16 as T
from test_gpu_msda_bounds import DINO

pytestmark = pytest.mark.gpu

GRADS = ("grad_value", "grad_offsets", "grad_logits")


def _operands(c, dtype, prologue_type):
    """the case's tensors on the device in their contract dtypes: (value, shapes, starts, ref, off, logits), mask, grad_out"""
    tsh, tls = T._level_tensors(c["shapes"])
    pt = dtype if prologue_type == "h16" else None
    mask = None if c["mask"] is None else torch.from_numpy(np.array(c["mask"])).cuda()
    args = (T._dev(c["value"], dtype), tsh, tls, T._dev(np.ascontiguousarray(c["ref"])), T._dev(c["off"], pt), T._dev(c["logits"], pt))
    return args, mask, T._dev(c["gout"], dtype)


@pytest.mark.parametrize("dtype,prologue_type", C.COMBOS)
@pytest.mark.parametrize("name", list(C.CASES))
def test_case_within_bound(name, dtype, prologue_type):
    MSDA = T._msda()
    s, c = C.CASES[name], C.inputs(name, dtype, prologue_type)
    args, mask, gout = _operands(c, dtype, prologue_type)
    out = MSDA.ms_deform_attn_h16_fused_forward(*args, mask)
    routes = [T._last()]
    got = dict(out=out)
    if s["backward"]:
        got.update(zip(GRADS, MSDA.ms_deform_attn_h16_fused_backward(*args, gout, mask)))
        routes.append(T._last())
    torch.cuda.synchronize()
    assert routes[0] == s["fwd"], (name, "forward", routes[0], s["fwd"])
    t16 = H.torch_dtype(dtype)
    tp = t16 if prologue_type == "h16" else torch.float32
    assert out.dtype == t16 and out.shape == (s["N"], args[4].shape[1], s["M"] * s["D"])
    if s["backward"]:
        assert routes[1] == s["bwd"], (name, "backward", routes[1], s["bwd"])
        assert got["grad_value"].dtype == t16 and got["grad_value"].shape == args[0].shape
        assert got["grad_offsets"].dtype == tp and got["grad_offsets"].shape == args[4].shape
        assert got["grad_logits"].dtype == tp and got["grad_logits"].shape == args[5].shape
        if c["mask"] is not None:
            assert not got["grad_value"].float().cpu().numpy()[c["mask"]].any(), "padded pixels must receive exactly zero gradient"
    ref = C.reference(name, dtype, prologue_type)
    worst = {}
    for k, t in got.items():      # (every figure is printed before the first assertion can fail)
        r = ref[k].ratio(t.float().cpu().numpy())
        worst[k] = float(r.max())
    print(f"\n{name} {dtype} prologue {prologue_type}: routes {routes}; worst err/bound " + ", ".join(f"{k} {v:.3f}" for k, v in worst.items()))
    for k, t in got.items():
        F.check(f"{name} {dtype}/{prologue_type} [{' / '.join(routes)}]", k, t.float().cpu().numpy(), ref[k])


def test_no_mask_equals_an_all_false_mask():
    """Bit for bit where the result is a function of the arguments: out, grad_offsets, grad_logits.  grad_value is summed with
    fp32 atomics whose order differs from launch to launch, with or without a mask: both runs are judged by the bound instead."""
    MSDA = T._msda()
    dtype, pt = "bf16", "h16"
    c = C.inputs(C.UNMASKED, dtype, pt)
    assert c["mask"] is None
    args, _, gout = _operands(c, dtype, pt)
    none = torch.zeros(args[0].shape[:2], dtype=torch.bool, device="cuda")
    a = [MSDA.ms_deform_attn_h16_fused_forward(*args, None)] + list(MSDA.ms_deform_attn_h16_fused_backward(*args, gout, None))
    b = [MSDA.ms_deform_attn_h16_fused_forward(*args, none)] + list(MSDA.ms_deform_attn_h16_fused_backward(*args, gout, none))
    torch.cuda.synchronize()
    for i in (0, 2, 3):
        assert torch.equal(a[i], b[i]), i
    ref = C.reference(C.UNMASKED, dtype, pt)
    for run in (a, b):
        F.check("mask None / all False", "grad_value", run[1].float().cpu().numpy(), ref["grad_value"])


def test_front_end_errors():
    MSDA = T._msda()
    c = C.inputs("dec_points_m3", "fp16", "h16")
    (v, tsh, tls, ref, off, lg), _, g = _operands(c, "fp16", "h16")
    assert MSDA.fused_h16_supported(v, ref, off, lg) and MSDA.fused_h16_supported(v, ref.half(), off, lg)
    assert MSDA.fused_h16_supported(v, ref, off.float(), lg.float())
    # the other 16-bit type, or offsets and logits of two types
    for o, l in ((off.to(torch.bfloat16), lg.to(torch.bfloat16)), (off.float(), lg)):
        assert not MSDA.fused_h16_supported(v, ref, o, l)
        with pytest.raises(RuntimeError, match="both be Float or both be value's dtype"):
            MSDA.ms_deform_attn_h16_fused_forward(v, tsh, tls, ref, o, l)
        with pytest.raises(RuntimeError, match="both be Float or both be value's dtype"):
            MSDA.ms_deform_attn_h16_fused_backward(v, tsh, tls, ref, o, l, g)
    # channels != 32: there is no generic fused kernel
    v16 = v.view(v.shape[0], v.shape[1], v.shape[2] * 2, 16)
    assert not MSDA.fused_h16_supported(v16, ref, off, lg)
    with pytest.raises(RuntimeError, match="32 channels per head"):
        MSDA.ms_deform_attn_h16_fused_forward(v16, tsh, tls, ref, off.repeat(1, 1, 2, 1, 1, 1), lg.repeat(1, 1, 2, 1))
    # offsets off the 8-byte grid
    off2 = T._off_grid(off)
    assert not MSDA.fused_h16_supported(v, ref, off2, lg)
    with pytest.raises(RuntimeError, match="8-byte aligned"):
        MSDA.ms_deform_attn_h16_fused_forward(v, tsh, tls, ref, off2, lg)
    with pytest.raises(RuntimeError, match="Not implemented on the CPU"):
        MSDA.ms_deform_attn_h16_fused_forward(v.cpu(), tsh, tls, ref, off, lg)
    with pytest.raises(RuntimeError, match="sampling_offsets must be on the same device as value|sampling_offsets must be a CUDA tensor"):
        MSDA.ms_deform_attn_h16_fused_forward(v, tsh, tls, ref, off.cpu(), lg)
    with pytest.raises(RuntimeError, match="value must be Half or BFloat16"):
        MSDA.ms_deform_attn_h16_fused_forward(v.float(), tsh, tls, ref, off.float(), lg.float())
    with pytest.raises(RuntimeError, match="must share one dtype"):
        MSDA.ms_deform_attn_h16_fused_backward(v, tsh, tls, ref, off, lg, g.to(torch.bfloat16))
    with pytest.raises(RuntimeError, match="must equal value.size"):
        MSDA.ms_deform_attn_h16_fused_forward(v[:, :-1].contiguous(), tsh, tls, ref, off, lg)
    assert not MSDA.fused_h16_supported(v.float(), ref, off.float(), lg.float()) and not MSDA.fused_h16_supported(v.cpu(), ref, off, lg)


def test_mixed_fused_function_gradients_and_saved_tensors():
    """MSDeformAttnMixedFusedFunction: the 16-bit value and the raw operands are saved, gradients have the operands' dtypes, none
    flows to the reference points or the index tensors."""
    import semi_detr_amd as sda
    dtype, pt = "bf16", "h16"
    c = C.inputs("dec_boxes", dtype, pt)
    (v, tsh, tls, ref, off, lg), _, g = _operands(c, dtype, pt)
    v, off, lg = v.requires_grad_(True), off.requires_grad_(True), lg.requires_grad_(True)
    ref = ref.requires_grad_(True)
    out = sda.MSDeformAttnMixedFusedFunction.apply(v, tsh, tls, ref, off, lg)
    saved = out.grad_fn.saved_tensors
    assert out.dtype == torch.bfloat16 and [t.dtype for t in (saved[0], saved[4], saved[5])] == [torch.bfloat16] * 3
    out.backward(g)
    assert v.grad.dtype == off.grad.dtype == lg.grad.dtype == torch.bfloat16 and ref.grad is None
    want = C.reference("dec_boxes", dtype, pt)
    for k, t in (("out", out), ("grad_value", v.grad), ("grad_offsets", off.grad), ("grad_logits", lg.grad)):
        F.check("MSDeformAttnMixedFusedFunction", k, t.detach().float().cpu().numpy(), want[k])


# ---- MSDeformAttn(256, 4, 8, 4) with fuse_prologue_16bit, DINO pyramid, N = 2 (helpers of tests/test_gpu_msda_h16.py) ----------

def _ctx(variant):
    return {"autocast_bf16": lambda: torch.autocast("cuda", dtype=torch.bfloat16),
            "autocast_fp16": lambda: torch.autocast("cuda", dtype=torch.float16),
            "half_module": lambda: torch.autocast("cuda", enabled=False)}[variant]()


def _dt(variant):
    return "bf16" if variant == "autocast_bf16" else "fp16"


def _linear_outputs(m, variant, call):
    """What the module's Linear layers hand the op (restated): value, offsets, logits in the variant's 16-bit type, and the
    reference points as the caller passes them."""
    query, ref, src, tsh, tls, mask = call
    if variant == "half_module":
        query, ref, src = query.half(), ref.half(), src.half()
    with torch.no_grad(), _ctx(variant):
        N, Lq, _ = query.shape
        M, L, P = m.n_heads, m.n_levels, m.n_points
        value = m.value_proj(src).view(N, src.shape[1], M, m.d_model // M)
        offsets = m.sampling_offsets(query).view(N, Lq, M, L, P, 2)
        logits = m.attention_weights(query).view(N, Lq, M, L * P)
    return value.contiguous(), tsh, tls, ref.contiguous(), offsets.contiguous(), logits.contiguous()


def _reference_of(args, mask, gout, variant):
    value, _, _, ref, off, lg = args
    f = lambda t: t.float().cpu().numpy()      # noqa: E731  (exact up-casts)
    return F.reference(f(value), np.asarray(DINO, np.int64), f(ref), f(off), f(lg), None if gout is None else f(gout),
                       None if mask is None else mask.cpu().numpy(), _dt(variant), "h16")


@pytest.mark.parametrize("variant", T.VARIANTS)
def test_module_no_grad_encoder_call_takes_the_fused_16bit_forward(variant):
    from semi_detr_amd.ops.modules import ms_deform_attn as mod
    MSDA = T._msda()
    m, call = T._module(variant), T._module_call("encoder")
    m.fuse_prologue_16bit = True
    query, ref, src, tsh, tls, mask = call
    assert mask is not None and bool(mask.any())
    if variant == "half_module":
        query, ref, src = query.half(), ref.half(), src.half()
    seen = []
    hook = m.output_proj.register_forward_pre_hook(lambda mod_, inp: seen.append(inp[0].detach().clone()))
    with mock.patch.object(mod, "MSDeformAttnMixedFusedFunction", wraps=mod.MSDeformAttnMixedFusedFunction) as spy, \
            mock.patch.object(mod, "MSDeformAttnMixedFunction", wraps=mod.MSDeformAttnMixedFunction) as other:
        with torch.no_grad(), _ctx(variant):
            out = m(query, ref, src, tsh, tls, mask)
    hook.remove()
    assert spy.apply.call_count == 1 and other.apply.call_count == 0
    assert T._last() == C.FWD4, T._last()
    args = _linear_outputs(m, variant, call)
    want = MSDA.ms_deform_attn_h16_fused_forward(*args, mask)
    t16 = H.torch_dtype(_dt(variant))
    assert seen[0].dtype == t16 and out.dtype == t16 and torch.equal(seen[0], want) and torch.isfinite(out.float()).all()
    F.check(f"module encoder no_grad {variant}", "out", seen[0].float().cpu().numpy(), _reference_of(args, mask, None, variant)["out"])


@pytest.mark.parametrize("variant", T.VARIANTS)
def test_module_decoder_training_call_takes_the_fused_16bit_route(variant):
    """2 x 50 decoder queries, forward and backward through MSDeformAttnMixedFusedFunction.  The comparison with the fp64 reference
    is made at the op boundary: what output_proj receives, and the gradients that reach the three Linear layers' outputs, against
    msda_h16_fused_ref on the very tensors the Linear layers produced and the grad_out the op received.  (The default route's
    query.grad / input_flatten.grad belong to another reference -- its offsets / normalizer product is formed in 16 bits -- so the
    two routes are not compared with each other beyond being finite and of the same dtypes.)"""
    m, call = T._module(variant), T._module_call("decoder")
    m.fuse_prologue_16bit = True
    t16 = H.torch_dtype(_dt(variant))
    grads = {}

    def keep(key):      # -> a tensor hook that records the gradient reaching that tensor
        return lambda g: grads.__setitem__(key, g.detach().clone())

    def watch_output(key):
        return lambda mod_, inp, out: out.register_hook(keep(key)) and None

    hooks = [lin.register_forward_hook(watch_output(k)) for k, lin in (("grad_value", m.value_proj), ("grad_offsets", m.sampling_offsets),
                                                                         ("grad_logits", m.attention_weights))]
    hooks.append(m.output_proj.register_forward_pre_hook(lambda mod_, inp: inp[0].register_hook(keep("gout")) and None))
    seen = []
    out, gq, gs, op = T._run_module(m, variant, call, seen)
    for h in hooks:
        h.remove()
    assert op == "MixedFused", op
    assert T._last() == C.FWD4, T._last()      # (the backward runs on autograd's thread; the last-kernels string is per thread)
    assert out.dtype == t16 and out.shape == call[0].shape and torch.isfinite(out.float()).all()
    in_dtype = torch.float16 if variant == "half_module" else torch.float32
    assert gq.dtype == in_dtype and gs.dtype == in_dtype and torch.isfinite(gq.float()).all() and torch.isfinite(gs.float()).all()
    assert gq.float().abs().max() > 0 and gs.float().abs().max() > 0
    for name, p in m.named_parameters():
        assert p.grad is not None and p.grad.dtype == p.dtype and torch.isfinite(p.grad.float()).all(), name
    assert len(seen) == 1 and seen[0].dtype == t16 and all(grads[k].dtype == t16 for k in GRADS + ("gout",))
    args = _linear_outputs(m, variant, call)
    ref = _reference_of(args, None, grads["gout"], variant)
    F.check(f"module decoder {variant}", "out", seen[0].float().cpu().numpy(), ref["out"])
    for k in GRADS:
        F.check(f"module decoder {variant}", k, grads[k].float().cpu().numpy().reshape(ref[k].val.shape), ref[k])
    # the default route on the same call: finite gradients of the same dtypes
    m.fuse_prologue_16bit = False
    out0, gq0, gs0, op0 = T._run_module(m, variant, call)
    assert op0 == "Mixed" and gq0.dtype == gq.dtype and gs0.dtype == gs.dtype
    assert torch.isfinite(gq0.float()).all() and torch.isfinite(gs0.float()).all()


@pytest.mark.parametrize("variant", T.VARIANTS)
def test_module_encoder_training_call_stays_on_the_upcast_route(variant):
    import semi_detr_amd as sda
    sda._lib.set_forward_policy("patch")
    try:
        m, call = T._module(variant), T._module_call("encoder")
        m.fuse_prologue_16bit = True
        before = T._last()
        assert T._run_module(m, variant, call)[3] == "" and T._last() == before
    finally:
        sda._lib.set_forward_policy("adaptive")


@pytest.mark.parametrize("variant", T.VARIANTS)
def test_module_default_route_is_unchanged(variant):
    """fuse_prologue_16bit at its default: the ops and kernels of the route as it was (tests/test_gpu_msda_h16.py)."""
    m = T._module(variant)
    assert m.fuse_prologue_16bit is False
    assert T._run_module(m, variant, T._module_call("decoder"))[3] == "Mixed" and T._last() == C16.FWD4
    query, ref, src, tsh, tls, mask = T._module_call("encoder")
    if variant == "half_module":
        query, ref, src = query.half(), ref.half(), src.half()
    with torch.no_grad(), _ctx(variant):
        m(query, ref, src, tsh, tls, mask)
    assert T._last() == C16.FWD4, T._last()
    # a module whose reference points require a gradient keeps the default route too (the fused op returns none)
    m.fuse_prologue_16bit = True
    q, r, s, tsh, tls, mask = T._module_call("decoder")
    if variant == "half_module":
        q, r, s = q.half(), r.half(), s.half()
    with _ctx(variant):
        out = m(q.requires_grad_(True), r.requires_grad_(True), s, tsh, tls, mask)
    assert T._op_of(out) == "Mixed"
