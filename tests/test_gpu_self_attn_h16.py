"""GPU: the self-attention's ``operand`` arithmetic (``ArithH16`` of csrc/self_attn.hip: fp16 / bf16 on the 16-bit MFMA) against
tests/self_attn_h16_ref64.py: every element of ``out``, ``lse``, ``dq``, ``dk`` and ``dv`` of every case of
tests/self_attn_cases.py through the C ABI, into NaN-filled buffers, in the case's own layout; gradient subsets, run-to-run
bits, rows at 8 bytes, the memory the route holds, and the module against ``nn.MultiheadAttention`` under the same autocast."""
import copy

import numpy as np
import pytest
import torch

import self_attn_cases as C
import self_attn_h16_ref64 as R16
from msda_h16_ref import torch_dtype
from self_attn_abi import run_abi

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
WORST = {}                                   # (quantity, dtype) -> worst error / bound over the cases, printed by the last test


def _bits(t):
    return t.numpy().tobytes()


@pytest.mark.parametrize("dt", R16.DTYPES)
@pytest.mark.parametrize("name", C.names())
def test_case_through_the_c_abi_within_bounds(name, dt):
    p = C.cases()[name]
    got = run_abi(p, dt)
    ref = R16.reference(name, dt)
    rep = R16.judge({n: t.numpy() for n, t in got.items()}, ref)
    print(R16.table(f"{name} {dt}", rep))
    for n, v in rep.items():
        WORST[n, dt] = max(WORST.get((n, dt), 0.0), v)
    R16.check({n: t.numpy() for n, t in got.items()}, ref, f"{name} {dt}")
    if name == "blocked_row":                # NaN exactly where torch has it, nothing left from the fill
        o = got["out"].numpy()
        assert np.isnan(o[40]).all() and not np.isnan(np.delete(o, 40, axis=0)).any()
        assert not torch.isnan(got["lse"]).any()
    else:
        assert not any(torch.isnan(t).any() for t in got.values()), "a NaN of the fill is left"


@pytest.mark.parametrize("dt", R16.DTYPES)
def test_gradient_subsets_are_bitwise_the_full_call_and_leave_the_rest_untouched(dt):
    for name in ("dn_edges_in_tiles", "lq_ne_lk"):          # packed and separate
        p = C.cases()[name]
        full = run_abi(p, dt)
        for want in ("q", "kv", "v"):
            got = run_abi(p, dt, want=want)
            for n in "qkv":
                if n in want:
                    assert _bits(got["d" + n]) == _bits(full["d" + n]), (name, want, n)
                else:
                    assert torch.isnan(got["d" + n]).all(), (name, want, n, "an unasked buffer was written")


@pytest.mark.parametrize("name", ["dn_skipped_tiles", "L257_B3_masked", "lq_ne_lk"])
def test_two_runs_agree_bitwise(name):
    for dt in R16.DTYPES:
        a, b = run_abi(C.cases()[name], dt), run_abi(C.cases()[name], dt)
        assert all(_bits(a[n]) == _bits(b[n]) for n in a), (name, dt)


@pytest.mark.parametrize("dt", R16.DTYPES)
def test_rows_eight_bytes_into_a_sixteen_byte_line_are_read_in_place(dt):
    p = C.cases()["L65_B1"]
    a, b = run_abi(p, dt, layout="separate"), run_abi(p, dt, layout="separate", shift8=True)
    assert all(_bits(a[n]) == _bits(b[n]) for n in a)
    from semi_detr_amd import _lib
    t = torch.zeros(4, 2, 260, dtype=torch_dtype(dt), device=DEV)[..., 4:]
    assert _lib.rows_native(t).data_ptr() == t.data_ptr()    # the Python route hands such a slice over as it is


def _leaves(p, dt, dtype=None):
    r16 = R16.rounded(p, dt)
    dtype = dtype or torch_dtype(dt)
    return [torch.from_numpy(r16[n]).to(DEV).to(dtype).requires_grad_(n != "gout") for n in ("q", "k", "v", "gout")]


def test_the_operand_route_holds_no_fp32_copy():
    import semi_detr_amd as s
    name = "L257_B3_masked"
    p = C.cases()[name]
    mask = torch.from_numpy(p["mask"]).to(DEV)
    (Lq, B, E), H = p["q"].shape, p["heads"]
    up = lambda n: -(-n // 512) * 512      # noqa: E731  (the caching allocator's block granularity)
    work = s._lib.lib().semidetr_self_attn_workspace_bytes(B, H, Lq, Lq)
    allowed = up(Lq * B * E * 2) + up(B * H * Lq * 4) + up(work) + 3 * up(Lq * B * E * 2)     # out, lse, workspace, dq dk dv

    def peak(arithmetic):
        q, k, v, g = _leaves(p, "bf16")
        torch.cuda.synchronize()
        base = torch.cuda.memory_allocated()
        torch.cuda.reset_peak_memory_stats()
        out = s.masked_attention(q, k, v, H, attn_mask=mask, arithmetic=arithmetic)
        grads = torch.autograd.grad(out, (q, k, v), g)
        torch.cuda.synchronize()
        assert out.dtype == torch.bfloat16 and all(t.dtype == torch.bfloat16 for t in grads)
        return torch.cuda.max_memory_allocated() - base
    operand, fp32 = peak("operand"), peak("fp32")
    print(f"peak bytes above the operands at {name}: operand {operand}, fp32 {fp32}, allowed {allowed}")
    assert operand <= allowed
    assert fp32 > allowed, "the measurement does not see the fp32 route's copies"


@pytest.mark.parametrize("dt", R16.DTYPES)
@pytest.mark.parametrize("name", ["dn_edges_in_tiles", "L129_B3_masked"])
def test_masked_attention_operand_route_within_bounds(name, dt):
    """Through autograd: the packed ``[q | k]`` function of the module and the separate one of ``masked_attention``."""
    import semi_detr_amd as s
    p, ref = C.cases()[name], R16.reference(name, dt)
    mask = torch.from_numpy(p["mask"]).to(DEV)
    q, k, v, g = _leaves(p, dt)
    out = s.masked_attention(q, k, v, p["heads"], attn_mask=mask, scale=p["scale"], arithmetic="operand")
    assert out.dtype == q.dtype
    out.backward(g)
    assert all(t.grad.dtype == t.dtype for t in (q, k, v))
    got = dict(out=out.detach(), dq=q.grad, dk=k.grad, dv=v.grad)
    R16.check({n: t.float().cpu().numpy() for n, t in got.items()}, ref, f"{name} {dt} separate")
    E = q.shape[2]
    qk = torch.cat([q.detach(), k.detach()], dim=2).requires_grad_(True)
    v2 = v.detach().clone().requires_grad_(True)
    out2 = s.self_attn.MaskedAttentionH16Function.apply(qk, v2, None, mask.view(torch.uint8), p["heads"], 32 ** -0.5, True)
    out2.backward(g)
    assert qk.grad.dtype == qk.dtype and qk.grad.shape == qk.shape
    assert torch.equal(out2, out) and torch.equal(qk.grad[..., :E], q.grad) and torch.equal(qk.grad[..., E:], k.grad)
    assert torch.equal(v2.grad, v.grad)
    # fp32 operands take the fp32 kernels whatever the argument says
    qf, kf, vf, gf = _leaves(p, dt, torch.float32)
    a = s.masked_attention(qf, kf, vf, p["heads"], attn_mask=mask, arithmetic="operand")
    b = s.masked_attention(qf, kf, vf, p["heads"], attn_mask=mask, arithmetic="fp32")
    assert a.dtype == torch.float32 and torch.equal(a, b)


REGIMES = {"autocast_fp16": (torch.float16, True), "autocast_bf16": (torch.bfloat16, True),
           "half_module": (torch.float16, False), "bfloat16_module": (torch.bfloat16, False)}


@pytest.mark.parametrize("regime", list(REGIMES))
def test_converted_module_is_no_further_from_float64_than_torch_under_the_same_regime(regime):
    """``convert_self_attention(m, arithmetic="operand")`` against the float64 module on the same weights and inputs at
    L257_B3_masked: dtypes are those of ``nn.MultiheadAttention``; the RMS error of the output and of every input / parameter
    gradient is no larger than that of ``nn.MultiheadAttention`` in the same regime, with no margin: the core adds only the
    roundings torch's route has too (P, the results) and omits torch's rounding of the scores and of the bmm outputs."""
    import semi_detr_amd as s
    dt16, autocast = REGIMES[regime]
    p = C.cases()["L257_B3_masked"]
    torch.manual_seed(0)
    E, H = p["q"].shape[2], p["heads"]
    base = torch.nn.MultiheadAttention(E, H, dropout=0.0).to(DEV)
    with torch.no_grad():
        base.in_proj_bias.normal_(0.0, 0.1)
        base.out_proj.bias.normal_(0.0, 0.1)
    if not autocast:
        base = base.to(dt16)
    io = dt16 if not autocast else torch.float32
    query, value = (torch.from_numpy(p[n]).to(DEV).to(io) for n in ("q", "v"))
    g = torch.from_numpy(p["gout"]).to(DEV).to(dt16)         # what every arm receives, the float64 one included
    mask = torch.from_numpy(p["mask"]).to(DEV)

    class Wrap(torch.nn.Module):
        def __init__(self, mha):
            super().__init__()
            self.self_attn = mha

    def run(wrap, dtype, cast):
        x, y = (t.detach().to(dtype, copy=True).requires_grad_(True) for t in (query, value))      # fresh leaves for every arm
        with torch.autocast("cuda", dtype=dt16, enabled=cast):
            out = wrap.self_attn(x, x, y, attn_mask=mask)[0]
        out.backward(g.to(out.dtype))
        res = [out.detach(), x.grad, y.grad] + [t.grad for t in wrap.parameters()]
        return res
    exact = run(Wrap(copy.deepcopy(base).double()), torch.float64, False)
    theirs = run(Wrap(copy.deepcopy(base)), io, autocast)
    mine = Wrap(copy.deepcopy(base))
    assert s.convert_self_attention(mine, arithmetic="operand") == 1 and mine.self_attn.arithmetic == "operand"
    ours = run(mine, io, autocast)
    names = ["out", "g_query", "g_value"] + [n for n, _ in mine.named_parameters()]
    bad = []
    for what, x, a, b in zip(names, exact, theirs, ours):
        assert b.dtype == a.dtype and b.shape == a.shape, (what, b.dtype, a.dtype)
        rms = lambda t: float((t.double() - x).pow(2).mean().sqrt())      # noqa: E731
        print(f"{regime:16s} {what:28s} rms |torch - fp64| = {rms(a):.4g}   rms |operand - fp64| = {rms(b):.4g}")
        if not rms(b) <= rms(a):
            bad.append((what, rms(b), rms(a)))
    assert not bad, f"{regime}: further from float64 than nn.MultiheadAttention: {bad}"


def test_full_size_once_in_bf16():
    p = C.full_size()
    ref = R16.ref64_h16(p, "bf16")
    got = run_abi(p, "bf16")
    rep = R16.check({n: t.numpy() for n, t in got.items()}, ref, "full size bf16")
    print(R16.table("L1100 pad200 B2 bf16", rep))


def test_print_the_worst_ratios():
    """The worst error / bound per quantity and dtype over the C-ABI cases above (profiles/self_attn_h16_probe.txt records it)."""
    for dt in R16.DTYPES:
        print(R16.table(f"worst over the cases, {dt}", {n: v for (n, d), v in sorted(WORST.items()) if d == dt}))
