"""GPU: semi_detr_amd.add_layer_norm / LayerNorm / the layer-level forwards (csrc/add_norm.hip) against the float64 statement
tests/add_norm_ref64.py: every element of ``y``, ``q``, ``mean``, ``rstd``, ``dx``, ``dweight`` and ``dbias`` through
``check_add_norm`` on the cases of tests/add_norm_cases.py.  Before each call NaN-filled buffers of the results' sizes are freed
into the caching allocator, so an element a kernel does not write shows.

The layer-level checks run the SAME modules (tests/add_norm_torch_restated.py: shared ``nn.Linear`` GEMMs, the attention
branches a fixed linear map) once through their own stock-torch forward and once through ``add_norm``'s forwards, and judge both
against the restatement in float64.  Across two layers the per-epilogue bounds of add_norm_ref64 do not compose into anything
useful (each LayerNorm divides by a data-dependent sigma), so the scale is the error of the fp32 restatement itself:
``max |hip - f64| <= FACTOR * max |fp32 restatement - f64|`` per tensor.  FACTOR = 4: the two fp32 sides share every GEMM and
differ in the order of 256-term sums of the same depth (8), so their errors are draws from the same distribution and the maxima
of two such draws over thousands of elements differ by well under 2; the second factor of 2 is head-room for the tensors of
256 elements (the norms' gradients), where the maximum of a single draw is itself uncertain by that much.  A wrong term (a
dropped residual or pos, a wrong mean, a query taken from the wrong layer) is off by 1e-2 or more against errors of 1e-6.
"""
import numpy as np
import pytest
import torch

import add_norm_cases as C
import add_norm_ref64 as R
import add_norm_torch_restated as T

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FACTOR = 4.0


def _poison(*shapes):
    junk = [torch.full(s, float("nan"), dtype=torch.float32, device=DEV) for s in shapes for _ in range(2)]
    del junk


def _layout(a, layout):
    """the logical (r0, r1, 256) array on the GPU in the case's memory layout"""
    if a is None:
        return None
    t = torch.from_numpy(np.array(a)).to(DEV)
    if layout == "transposed":
        return t.transpose(0, 1).contiguous().transpose(0, 1)
    if layout == "offset":
        buf = torch.full((t.shape[0], t.shape[1] + 2, t.shape[2]), float("nan"), device=DEV)
        buf[:, 1:-1] = t
        return buf[:, 1:-1]
    return t


def run(case):
    import semi_detr_amd as s
    from semi_detr_amd.add_norm import add_layer_norm_forward
    lay = case["layout"]
    x, res, pos, gy, gq = (_layout(case[k], lay) for k in ("x", "residual", "pos", "gy", "gq"))
    if lay != "contiguous" and x.shape[0] > 1 and x.shape[1] > 1:
        assert not x.is_contiguous()
    w, b = (torch.from_numpy(np.array(case[k])).to(DEV).requires_grad_(True) for k in ("weight", "bias"))
    shape = tuple(x.shape)
    _poison(shape, shape)
    y0, q0, mean, rstd = add_layer_norm_forward(x, res, w, b, case["eps"], pos)
    got = {"y": y0.cpu().numpy(), "mean": mean.cpu().numpy(), "rstd": rstd.cpu().numpy()}
    if pos is not None:
        got["q"] = q0.cpu().numpy()
    leaves = [t.requires_grad_(True) for t in (x, res, pos) if t is not None]
    _poison(shape, shape)
    out = s.add_layer_norm(x, res, w, b, case["eps"], pos)
    y, q = out if pos is not None else (out, None)
    assert y.is_contiguous() and y.dtype == torch.float32 and torch.equal(y, y0) and (q is None or torch.equal(q, q0))
    outs, grads = ([y], [gy]) if gy is not None else ([], [])
    if gq is not None:
        outs.append(q)
        grads.append(gq)
    _poison(shape, (256,), (256,))
    torch.autograd.backward(outs, grads)
    got["dx"], got["dweight"], got["dbias"] = x.grad.cpu().numpy(), w.grad.cpu().numpy(), b.grad.cpu().numpy()
    if res is not None:
        assert torch.equal(res.grad, x.grad), "the gradient of residual is dx"
    if pos is not None:
        assert (pos.grad is None) if gq is None else torch.equal(pos.grad, gq), "the gradient of pos is gq itself"
    return got


@pytest.mark.parametrize("name", C.names())
def test_case_within_bounds(name):
    case = C.cases()[name]
    got = run(case)
    print(R.table(name, {k: R.ratio(v, C.reference(name)[k]) for k, v in got.items()}))
    R.check_add_norm(case, got, name, C.reference(name))


def test_two_runs_are_bitwise_equal():
    case = C.cases()["r2051_contiguous"]
    a, b = run(case), run(case)
    assert sorted(a) == ["dbias", "dweight", "dx", "mean", "q", "rstd", "y"]
    assert all(a[k].tobytes() == b[k].tobytes() for k in a), "not bit-identical from run to run"


@pytest.mark.parametrize("name", ["r3_special_rows", "r2051_contiguous", "r65_offset"])
def test_equal_values_row_gives_the_bias_bit_for_bit(name):
    case = C.cases()[name]
    got = run(case)
    assert got["y"].reshape(-1, 256)[0].tobytes() == case["bias"].tobytes()
    assert got["mean"][0] == (0.75 if case["residual"] is not None else 1.375)


def test_only_the_needed_parameter_sums_and_16_bit_inputs():
    import semi_detr_amd as s
    case = C.cases()["r65_contiguous"]
    ref = C.reference("r65_contiguous")
    x, res, gy = (torch.from_numpy(np.array(case[k])).to(DEV) for k in ("x", "residual", "gy"))
    w, b = (torch.from_numpy(np.array(case[k])).to(DEV) for k in ("weight", "bias"))
    x.requires_grad_(True)
    s.add_layer_norm(x, res, w, b, case["eps"]).backward(gy)              # one backward launch: no parameter gradient
    R.check_add_norm(case, {"dx": x.grad.cpu().numpy()}, "dx only", ref)
    w.requires_grad_(True)
    s.add_layer_norm(x.detach(), res, w, b, case["eps"]).backward(gy)     # dweight without dbias
    assert b.grad is None
    R.check_add_norm(case, {"dweight": w.grad.cpu().numpy()}, "dweight only", ref)
    # bf16 in -> fp32 arithmetic on the up-cast -> bf16 out: the fp32 result of the rounded inputs, rounded once
    xb, rb = x.detach().bfloat16(), res.bfloat16()
    yb = s.add_layer_norm(xb, rb, w.detach(), b, case["eps"])
    want = s.add_layer_norm(xb.float(), rb.float(), w.detach(), b, case["eps"]).bfloat16()
    assert yb.dtype == torch.bfloat16 and torch.equal(yb, want)
    empty = s.add_layer_norm(torch.empty(0, 4, 256, device=DEV), None, w.detach(), b, pos=torch.empty(0, 4, 256, device=DEV))
    assert empty[0].shape == (0, 4, 256) and empty[1].shape == (0, 4, 256)
    with pytest.raises(NotImplementedError, match="row width"):
        s.add_layer_norm(torch.zeros(2, 128, device=DEV), None, torch.ones(128, device=DEV), torch.zeros(128, device=DEV))


# ------------------------------------------------------------------------------------------------------------------
# layer level
# ------------------------------------------------------------------------------------------------------------------
def _judge(name, hip, rest32, ref64):
    """every tensor of ``hip`` against the float64 restatement, on the scale of the fp32 restatement's own error"""
    assert len(hip) == len(rest32) == len(ref64)
    worst = 0.0
    for i, (h, r, d) in enumerate(zip(hip, rest32, ref64)):
        if d is None:
            assert h is None and r is None, (name, i)
            continue
        scale = float((r.double() - d).abs().max())
        err = float((h.double() - d).abs().max())
        assert torch.isfinite(h).all() and scale > 0, (name, i)
        worst = max(worst, err / scale)
        assert err <= FACTOR * scale, f"{name}[{i}]: |hip - f64| = {err:.3e}, |fp32 restatement - f64| = {scale:.3e}"
    print(f"  {name}: {len(hip)} tensors, worst |hip - f64| / |fp32 restatement - f64| = {worst:.2f}")


def _grads(outs, wrt, seeds):
    return list(torch.autograd.grad(outs, wrt, seeds, allow_unused=True))


def _encoder_problem(dropout=0.0):
    g = torch.Generator().manual_seed(5)
    torch.manual_seed(5)                                             # the Linear layers draw from the global generator
    enc = T.Encoder(2, 512, dropout)
    T.randomize_norms(enc, g)
    tokens = 8 * 6 + 4 * 3                                           # a 2-level pyramid
    src, pos, seed = (torch.randn(2, tokens, 256, generator=g) for _ in range(3))
    shapes = torch.tensor([[8, 6], [4, 3]])
    return enc.to(DEV), src.to(DEV), pos.to(DEV), seed.to(DEV), shapes.to(DEV)


def _encoder_sides(enc, src, pos, seed, shapes, train=False):
    from semi_detr_amd import add_norm
    enc.train(train)
    args = (shapes, shapes.new_tensor([0, 48]), None, None)
    params = list(enc.parameters())
    sides = {}
    for side in ("rest", "hip", "f64"):
        m = T.in_float64(enc) if side == "f64" else enc
        cast = (lambda t: t.double()) if side == "f64" else (lambda t: t)
        s_, p_ = cast(src).requires_grad_(True), cast(pos).requires_grad_(True)
        torch.manual_seed(11)
        out = (add_norm.encoder_forward(m, s_, p_, *args) if side == "hip" else m(s_, p_, *args))[0]
        sides[side] = [out.detach()] + _grads([out], [s_, p_] + list(m.parameters()), [cast(seed)])
    assert len(sides["hip"]) == 3 + len(params)
    return sides


def test_encoder_forward_against_the_restatement():
    sides = _encoder_sides(*_encoder_problem())
    assert sides["hip"][2] is not None                               # pos receives the sum over both layers
    _judge("encoder", sides["hip"], sides["rest"], sides["f64"])


def _decoder_problem(dropout=0.0):
    g = torch.Generator().manual_seed(6)
    torch.manual_seed(6)
    dec = T.DecoderStack(2, 512, dropout)
    T.randomize_norms(dec, g)
    tgt, qpos = (torch.randn(7, 2, 256, generator=g) for _ in range(2))
    memory = torch.randn(60, 2, 256, generator=g)
    refp = torch.rand(7, 2, 4, generator=g)
    seeds = [torch.randn(7, 2, 256, generator=g) for _ in range(2)]
    return dec.to(DEV), [t.to(DEV) for t in (tgt, qpos, refp, memory)], [t.to(DEV) for t in seeds]


def _decoder_sides(dec, inputs, seeds, hip_forward, train=False, f64_of=None):
    dec.train(train)
    sides = {}
    for side in ("rest", "hip", "f64"):
        m = T.in_float64(f64_of if f64_of is not None else dec) if side == "f64" else dec
        m.train(train)
        cast = (lambda t: t.double()) if side == "f64" else (lambda t: t)
        tgt, qpos, refp, memory = (cast(t) for t in inputs)
        leaves = [t.requires_grad_(True) for t in (tgt, qpos, memory)]
        torch.manual_seed(12)
        outs = m(tgt, qpos, refp, memory, layer_forward=hip_forward if side == "hip" else None)
        sides[side] = [o.detach() for o in outs] + _grads(outs, leaves + list(m.parameters()), [cast(t) for t in seeds])
    return sides


def test_decoder_layer_forwards_against_the_restatement():
    from semi_detr_amd import add_norm
    dec, inputs, seeds = _decoder_problem()
    sides = _decoder_sides(dec, inputs, seeds, add_norm.decoder_layer_forward)
    _judge("decoder", sides["hip"], sides["rest"], sides["f64"])

    def staged(layer, tgt, tgt_query_pos, tgt_reference_points, memory):       # sa / ca / ffn called one by one
        tgt, query = add_norm.decoder_layer_forward_sa(layer, tgt, tgt_query_pos, want_query=True)
        tgt = add_norm.decoder_layer_forward_ca(layer, tgt, tgt_query_pos, tgt_reference_points=tgt_reference_points,
                                                memory=memory, query=query)
        return add_norm.decoder_layer_forward_ffn(layer, tgt)
    again = _decoder_sides(dec, inputs, seeds, staged)
    assert all(torch.equal(a, b) for a, b in zip(again["hip"], sides["hip"]))


def test_convert_layer_norms_on_a_decoder_stack():
    import semi_detr_amd as s
    dec, inputs, seeds = _decoder_problem()
    original = T.in_float64(dec)                                       # before the conversion: deepcopy keeps nn.LayerNorm
    params = list(dec.parameters())
    keys = list(dec.state_dict())
    rest = _decoder_sides(dec, inputs, seeds, None)["rest"]
    assert s.convert_layer_norms(dec) == 7                             # 3 per layer and the final norm
    assert all(a is b for a, b in zip(params, dec.parameters())) and list(dec.state_dict()) == keys
    assert type(dec.norm) is s.LayerNorm and type(dec.layers[1].norm3) is s.LayerNorm
    conv = _decoder_sides(dec, inputs, seeds, None, f64_of=original)
    _judge("converted decoder", conv["rest"], rest, conv["f64"])


def test_dropout_path():
    from semi_detr_amd import add_norm
    enc, src, pos, seed, shapes = _encoder_problem(dropout=0.1)
    plain = _encoder_sides(*_encoder_problem(dropout=0.0))["hip"]
    evaluated = _encoder_sides(enc, src, pos, seed, shapes, train=False)["hip"]
    assert all(torch.equal(a, b) for a, b in zip(plain, evaluated)), "p = 0.1 in eval mode is the p = 0 path"
    sides = _encoder_sides(enc, src, pos, seed, shapes, train=True)     # each side under torch.manual_seed(11): the same masks
    assert not torch.equal(sides["hip"][0], evaluated[0])
    # float64 draws other masks than fp32, so the fp32 restatement in training mode is the reference and the scale is the
    # eval-mode error of the same tensors (the same arithmetic with some branch elements zeroed and the rest times 1 / 0.9)
    ev = _encoder_sides(enc, src, pos, seed, shapes, train=False)
    for i, (h, r, e32, e64) in enumerate(zip(sides["hip"], sides["rest"], ev["rest"], ev["f64"])):
        scale = float((e32.double() - e64).abs().max())
        assert float((h - r).abs().max()) <= 2 * FACTOR * scale, i
    dec, inputs, seeds = _decoder_problem(dropout=0.1)
    sd = _decoder_sides(dec, inputs, seeds, add_norm.decoder_layer_forward, train=True)
    se = _decoder_sides(dec, inputs, seeds, add_norm.decoder_layer_forward, train=False)
    for i, (h, r, e32, e64) in enumerate(zip(sd["hip"], sd["rest"], se["rest"], se["f64"])):
        scale = float((e32.double() - e64).abs().max())
        assert float((h - r).abs().max()) <= 2 * FACTOR * scale, i
