"""GPU: semi_detr_amd.masked_attention / MultiheadAttention (csrc/self_attn.hip) against the float64 statement
tests/self_attn_ref64.py: every element of ``out``, ``dQ``, ``dK`` and ``dV`` through ``check_self_attn`` on the cases of
tests/self_attn_cases.py, on the decoder's own size and on the fixture recorded from the reference.  Before each call NaN-filled
buffers of the results' sizes are freed into the caching allocator, so an element a kernel does not write shows.

The module is judged stage by stage, each stage against float64 on the operands that stage actually received: the projections
(GEMMs) within gamma_{E+2} of their operand magnitudes, the core within ``check_self_attn``.  That the stages are the module is
itself checked: the module's results equal the staged chain's bit for bit."""
import os

import numpy as np
import pytest
import torch

import self_attn_cases as C
import self_attn_ref64 as R

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"


def _poison(*shapes):
    junk = [torch.full(s, float("nan"), dtype=torch.float32, device=DEV) for s in shapes for _ in range(2)]
    del junk


def _operands(p):
    """leaves that receive the gradients and the (q, k, v) handed to the op; -> (q, k, v, gradients())"""
    q, k, v = (torch.from_numpy(p[n]).to(DEV) for n in "qkv")
    if p["layout"] == "packed" and q.shape == k.shape:
        E = q.shape[2]
        buf = torch.cat([q, k, v], dim=2).requires_grad_(True)
        return buf[..., :E], buf[..., E:2 * E], buf[..., 2 * E:], \
            lambda: [buf.grad[..., i * E:(i + 1) * E].cpu().numpy() for i in range(3)]
    q, k, v = (t.requires_grad_(True) for t in (q, k, v))
    return q, k, v, lambda: [t.grad.cpu().numpy() for t in (q, k, v)]


def run(p):
    import semi_detr_amd as s
    q, k, v, grads = _operands(p)
    mask = None if p["mask"] is None else torch.from_numpy(p["mask"]).to(DEV)
    _poison(tuple(q.shape), tuple(k.shape))
    out = s.masked_attention(q, k, v, p["heads"], attn_mask=mask, scale=p["scale"])
    assert out.shape == q.shape and out.dtype == torch.float32 and out.is_contiguous()
    got = {"out": out.detach().cpu().numpy()}
    if not p["forward_only"]:
        _poison(tuple(q.shape), tuple(k.shape), tuple(k.shape))
        out.backward(torch.from_numpy(p["gout"]).to(DEV))
        got["dq"], got["dk"], got["dv"] = grads()
    return got


@pytest.mark.parametrize("name", C.names())
def test_case_within_bounds_and_backward_reproducible(name):
    p = C.cases()[name]
    got = run(p)
    rep = R.judge_self_attn(p, got, C.reference(name))
    print(R.table(name, rep))
    R.check_self_attn(p, got, name, C.reference(name))
    again = run(p)
    assert all(got[n].tobytes() == again[n].tobytes() for n in got), "not bit-identical from run to run"


def test_blocked_row_is_nan_in_that_row_only_and_backward_stays_finite_elsewhere():
    p = C.cases()["blocked_row"]
    got = run(p)
    assert np.isnan(got["out"][40]).all() and not np.isnan(np.delete(got["out"], 40, axis=0)).any()
    # the backward of this case is outside the contract: it only has to run and write its buffers
    q, k, v, grads = _operands(dict(p, layout="separate"))
    import semi_detr_amd as s
    out = s.masked_attention(q, k, v, p["heads"], attn_mask=torch.from_numpy(p["mask"]).to(DEV))
    out.backward(torch.from_numpy(p["gout"]).to(DEV))
    torch.cuda.synchronize()
    assert all(g.shape == t.shape for g, t in zip(grads(), (q, k, v)))


def test_only_the_requested_gradients_are_computed():
    import semi_detr_amd as s
    p = C.cases()["dn_edges_in_tiles"]
    ref = C.reference("dn_edges_in_tiles")
    mask = torch.from_numpy(p["mask"]).to(DEV)
    for wanted in ("q", "k", "v", "qv"):
        t = {n: torch.from_numpy(p[n]).to(DEV).requires_grad_(n in wanted) for n in "qkv"}
        _poison(tuple(t["q"].shape))
        out = s.masked_attention(t["q"], t["k"], t["v"], p["heads"], attn_mask=mask)
        out.backward(torch.from_numpy(p["gout"]).to(DEV))
        got = {"d" + n: t[n].grad.cpu().numpy() for n in wanted}
        assert all(t[n].grad is None for n in "qkv" if n not in wanted)
        R.check_self_attn(p, got, "wanted " + wanted, ref)


def test_full_size_decoder_case():
    p = C.full_size()
    ref = R.ref64(p)
    got = run(p)
    rep = R.check_self_attn(p, got, "full size", ref)
    print(R.table("L1100 pad200 B2", rep))


def test_refusals_on_the_gpu():
    import semi_detr_amd as s
    q = torch.zeros(8, 1, 256, device=DEV)
    with pytest.raises(NotImplementedError, match="float masks"):
        s.masked_attention(q, q, q, 8, attn_mask=torch.zeros(8, 8, device=DEV))
    with pytest.raises(NotImplementedError, match="per-head"):
        s.masked_attention(q, q, q, 8, attn_mask=torch.zeros(8, 8, 8, dtype=torch.bool, device=DEV))
    with pytest.raises(NotImplementedError, match="head dimension"):
        s.masked_attention(q, q, q, 4)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        s.masked_attention(q.cpu(), q.cpu(), q.cpu(), 8)
    # the library itself refuses another head dimension with its usual status and message
    import ctypes
    from semi_detr_amd import _lib, self_attn
    pr = self_attn._params(q, q, q, None, 4, 0.125)
    with pytest.raises(RuntimeError, match="head dimension 64"):
        _lib.call("semidetr_self_attn_forward_f32", q.device, ctypes.byref(pr), q, 0)


# ---------------------------------------------------------------------------------------------------------------------------
# the module, stage by stage
# ---------------------------------------------------------------------------------------------------------------------------
def _gemm_check(got, x, w, b, what):
    """got = x @ w.T + b computed in fp32 from exactly these fp32 operands: within gamma_{K+2} (|x| @ |w|.T + |b|)"""
    x, w = x.double().cpu().numpy(), w.double().cpu().numpy()
    b = np.zeros(w.shape[0]) if b is None else b.double().cpu().numpy()
    want = x @ w.T + b
    bound = R.gamma(x.shape[-1] + 2) * (np.abs(x) @ np.abs(w).T + np.abs(b)) + R.TINY
    ratio = float((np.abs(got.double().cpu().numpy() - want) / bound).max())
    print(f"{what:28s} gemm error / bound = {ratio:.3f}")
    assert ratio <= 1.0, (what, ratio)


def _module_from(case):
    import semi_detr_amd as s
    E, H = case["in_proj_weight"].shape[1], int(case["heads"])
    m = s.MultiheadAttention(E, H)
    sd = {n: torch.from_numpy(case[n].astype(np.float32)) for n in ("in_proj_weight", "in_proj_bias")}
    sd["out_proj.weight"], sd["out_proj.bias"] = (torch.from_numpy(case[n].astype(np.float32)) for n in ("out_w", "out_b"))
    m.load_state_dict(sd, strict=True)
    return m.to(DEV)


@pytest.fixture(scope="module")
def golden():
    from conftest import Golden
    return Golden("self_attn.npz")


@pytest.mark.parametrize("name", ["plain", "dn_mask", "two_images"])
def test_module_against_the_recorded_reference_stage_by_stage(golden, name):
    import semi_detr_amd as s
    c = golden[name]
    m = _module_from(c)
    E, H = m.embed_dim, m.num_heads
    tgt, pos = (torch.from_numpy(c[n].astype(np.float32)).to(DEV) for n in ("tgt", "pos"))
    mask = torch.from_numpy(c["mask"].astype(bool)).to(DEV) if "mask" in c else None
    g_up = torch.from_numpy(c["g_tgt2"].astype(np.float32)).to(DEV)
    query = (tgt + pos).requires_grad_(True)
    value = tgt.clone().requires_grad_(True)
    y, w = m(query, query, value, attn_mask=mask)
    assert w is None
    y.backward(g_up)
    mod = [y.detach(), query.grad, value.grad] + [p.grad.clone() for p in m.parameters()]
    # the same chain by hand, with the core's operands and gradients kept
    m.zero_grad()
    q2, v2 = query.detach().clone().requires_grad_(True), value.detach().clone().requires_grad_(True)
    W, b = m.in_proj_weight, m.in_proj_bias
    qk = torch.nn.functional.linear(q2, W[:2 * E], b[:2 * E])
    vv = torch.nn.functional.linear(v2, W[2 * E:], b[2 * E:])
    qk.retain_grad(), vv.retain_grad()
    core = s.MaskedAttentionFunction.apply(qk, vv, None, None if mask is None else mask.view(torch.uint8), H, 32 ** -0.5, True)
    core.retain_grad()
    y2 = m.out_proj(core)
    y2.backward(g_up)
    staged = [y2.detach(), q2.grad, v2.grad] + [p.grad for p in m.parameters()]
    assert all(torch.equal(a, b_) for a, b_ in zip(mod, staged)), "the module is not the staged chain"
    # every stage against float64 on the operands it received
    _gemm_check(qk.detach(), query.detach(), W[:2 * E].detach(), b[:2 * E].detach(), name + " in_proj qk")
    _gemm_check(vv.detach(), value.detach(), W[2 * E:].detach(), b[2 * E:].detach(), name + " in_proj v")
    _gemm_check(y2.detach(), core.detach(), m.out_proj.weight.detach(), m.out_proj.bias.detach(), name + " out_proj")
    _gemm_check(core.grad, g_up, m.out_proj.weight.detach().t(), None, name + " out_proj backward")
    _gemm_check(q2.grad, qk.grad, W[:2 * E].detach().t(), None, name + " in_proj qk backward")
    _gemm_check(v2.grad, vv.grad, W[2 * E:].detach().t(), None, name + " in_proj v backward")
    problem = dict(q=qk.detach()[..., :E].cpu().numpy(), k=qk.detach()[..., E:].cpu().numpy(), v=vv.detach().cpu().numpy(),
                   heads=H, mask=None if mask is None else mask.cpu().numpy(), scale=None, gout=core.grad.cpu().numpy())
    got = dict(out=core.detach().cpu().numpy(), dq=qk.grad[..., :E].cpu().numpy(), dk=qk.grad[..., E:].cpu().numpy(),
               dv=vv.grad.cpu().numpy())
    print(R.table(name + " core", R.check_self_attn(problem, got, name)))
    # and the whole against the reference's recorded float64 output: the stages' bounds leave out how the core carries the
    # projections' rounding on, so this end-to-end comparison is a plain sanity limit of 1e-4 relative to the output's scale
    assert np.abs(y.detach().cpu().numpy() - c["tgt2"]).max() <= 1e-4 * max(1.0, np.abs(c["tgt2"]).max())


class _Layer(torch.nn.Module):
    """What DINOTransformerDecoderLayer holds for forward_sa (transformer.py:765, 793-816)."""

    def __init__(self, E, H):
        super().__init__()
        self.self_attn = torch.nn.MultiheadAttention(E, H, dropout=0.0)
        self.dropout2 = torch.nn.Dropout(0.0)
        self.norm2 = torch.nn.LayerNorm(E)

    def forward(self, tgt, pos, mask):
        q = k = tgt + pos
        tgt2 = self.self_attn(q, k, tgt, attn_mask=mask)[0]
        return self.norm2(tgt + self.dropout2(tgt2))


def test_converted_decoder_layer_gives_the_same_parameter_gradients():
    """After convert_self_attention the layer computes what it computed with torch's module.  Both are fp32 evaluations of one
    chain (E = 256 GEMMs, softmax over at most 70 keys, LayerNorm) that differ in the order of their sums, so their rounding
    errors against the float64 evaluation of the same layer have the same distribution; the largest error over a tensor of
    hundreds of elements or more then differs by a small factor between the two.  Limit per tensor: the mirror's largest
    distance to float64 is at most 4 times that of torch's fp32 path (the reference's own error)."""
    import copy

    import semi_detr_amd as s
    torch.manual_seed(0)
    E, H, L, B = 256, 8, 70, 2
    layer = _Layer(E, H).to(DEV)
    tgt, pos = torch.randn(L, B, E, device=DEV), torch.randn(L, B, E, device=DEV)
    mask = torch.from_numpy(C.dn_mask(3, 4, 46)).to(DEV)
    g = torch.from_numpy(R.grad_pattern((L, B, E), 3)).to(DEV)
    params = dict(layer.named_parameters())

    def run_layer(m, dt):
        m.zero_grad()
        t = tgt.to(dt).clone().requires_grad_(True)
        out = m(t, pos.to(dt), mask)
        out.backward(g.to(dt))
        return [out.detach().double(), t.grad.double()] + [p.grad.double() for p in m.parameters()]
    exact = run_layer(copy.deepcopy(layer).double(), torch.float64)
    before = run_layer(layer, torch.float32)
    assert s.convert_self_attention(layer) == 1 and isinstance(layer.self_attn, s.MultiheadAttention)
    assert dict(layer.named_parameters()).keys() == params.keys()
    assert all(a is b for a, b in zip(layer.parameters(), params.values()))
    after = run_layer(layer, torch.float32)
    for what, x, a, b in zip(["out", "g_tgt"] + list(params), exact, before, after):
        ref_err, err = float((a - x).abs().max()), float((b - x).abs().max())
        print(f"{what:28s} |torch fp32 - fp64| = {ref_err:.3g}  |mirror - fp64| = {err:.3g}")
        assert err <= 4.0 * ref_err, (what, err, ref_err)
