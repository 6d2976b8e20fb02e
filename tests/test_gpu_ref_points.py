"""GPU: semi_detr_amd.ref_points (csrc/ref_points.hip) against the float64 statement tests/ref_points_ref64.py: every element
of ``new_ref``, ``ref_input``, the embedding, ``g_delta`` and ``g_ref`` of every case of tests/ref_points_cases.py through
``check``.  Before each call NaN-filled buffers of the results' sizes are freed into the caching allocator, so an element a
kernel does not write shows.  The statement's dim_t is the table the mirror hands the kernel.

``decoder_forward`` and ``box_outputs`` run the SAME modules (tests/ref_points_torch_restated.py) once through stock torch and
once through the mirror; both are judged against the restatement in float64 by the rule and FACTOR of
tests/test_gpu_add_norm.py: ``max |hip - f64| <= FACTOR * max |fp32 restatement - f64|`` per tensor.
"""
import copy

import numpy as np
import pytest
import torch

import add_norm_torch_restated as A
import ref_points_cases as C
import ref_points_ref64 as R
import ref_points_torch_restated as T
from test_gpu_add_norm import _judge

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _poison(*shapes):
    junk = [torch.full(s, float("nan"), dtype=torch.float32, device=DEV) for s in shapes for _ in range(2)]
    del junk


def _layout(a, dtype, layout):
    """the logical (rows0, rows1, width) array on the GPU in ``dtype`` and the case's memory layout"""
    t = torch.from_numpy(np.array(a)).to(DEV).to(C.TORCH[dtype])
    if layout == "transposed":                        # the head's rows: (bs, nq, width) memory seen as (nq, bs, width)
        t = t.transpose(0, 1).contiguous().transpose(0, 1)
        assert t.shape[0] == 1 or t.shape[1] == 1 or not t.is_contiguous()
        return t
    if layout == "slice":
        buf = torch.full((t.shape[0], t.shape[1] + 2, t.shape[2] + 3), float("nan"), dtype=t.dtype, device=DEV)
        buf[:, 1:-1, 1:1 + t.shape[2]] = t
        return buf[:, 1:-1, 1:1 + t.shape[2]]
    return t


def _np(t):
    return None if t is None else t.detach().float().cpu().numpy()


def run(case):
    """the case through RefPointsFunction and torch.autograd -> the dict ``R.check`` reads, and the raw result tensors"""
    from semi_detr_amd import ref_points as P
    mode, lay, width = case["mode"], case["layout"], case["width"]
    refs = [_layout(seg["ref"], case["ref_dtype"], lay).requires_grad_(True) for seg in case["segments"]]
    deltas = [_layout(seg["delta"], case["delta_dtype"], lay).requires_grad_(True) for seg in case["segments"]] if mode == C.REFINE \
        else None
    vr = None if case["vr"] is None else torch.from_numpy(case["vr"]).to(DEV)
    shapes = [tuple(r.shape) for r in refs]
    if vr is not None:
        nq, bs = shapes[0][:2]
        shapes += [(bs, nq, vr.shape[1], width), (nq, bs, 128 * width)]
    _poison(*shapes)
    outs = P._apply(mode, case["eps"], vr, vr is not None, False, False, deltas, refs, "test")
    news = list(outs[:len(refs)]) if mode != C.NONE else []
    got, raw = {}, list(outs)
    if news:
        assert all(y.dtype == C.TORCH[case["out_dtype"]] and y.is_contiguous() for y in news)
        got["new_ref"] = [_np(y) for y in news]
    seeds = [torch.from_numpy(seg["g_new"]).to(DEV).to(C.TORCH[case["out_dtype"]]) for seg in case["segments"]] if news else []
    if vr is not None:
        ref_input, embed = outs[len(news):]
        assert ref_input.is_contiguous() and ref_input.dtype == embed.dtype == torch.float32
        got["ref_input"], got["embed"] = _np(ref_input.transpose(0, 1)), _np(embed)
        seeds += [torch.from_numpy(case["g_ref_input"]).to(DEV).transpose(0, 1), torch.from_numpy(case["g_embed"]).to(DEV)]
    _poison(*[tuple(r.shape) for r in refs] * 2)
    torch.autograd.backward(list(outs), seeds)
    assert all(r.grad.dtype == r.dtype and r.grad.shape == r.shape for r in refs)
    got["g_ref"] = [_np(r.grad) for r in refs]
    if deltas is not None:
        assert all(d.grad.dtype == d.dtype for d in deltas)
        got["g_delta"] = [_np(d.grad) for d in deltas]
    raw += [r.grad for r in refs] + ([d.grad for d in deltas] if deltas is not None else [])
    return got, raw


def _statement_case(case):
    from semi_detr_amd import ref_points as P
    case = dict(case, dim_t=P.dim_t(DEV).cpu().numpy())
    if case["mode"] == C.NONE:                        # nothing seeds the points themselves here: their gradient comes from scale and embed
        case["segments"] = [dict(seg, g_new=None) for seg in case["segments"]]
    return case


@pytest.mark.parametrize("name", C.names())
def test_case_within_bounds(name):
    case = C.cases()[name]
    got, _ = run(case)
    ratios = R.check(_statement_case(case), got, name)
    print(R.table(name, ratios))
    assert ratios["open"] == 0


@pytest.mark.parametrize("name", ["sigmoid_q130_b3_l4_w4", "refine_q65_b3_l4_w4_slice", "refine_6_segments_w4_transposed",
                                  "none_q130_b3_l1_w2_one"])
def test_two_runs_are_bitwise_equal(name):
    case = C.cases()[name]
    (_, a), (_, b) = run(case), run(case)
    assert len(a) == len(b) and len(a) >= 2
    for x, y in zip(a, b):
        assert x.dtype == y.dtype and x.contiguous().view(torch.uint8).equal(y.contiguous().view(torch.uint8)), \
            "not bit-identical from run to run"


def test_the_table_is_the_references_expression():
    from semi_detr_amd import ref_points as P
    t = torch.arange(128, dtype=torch.float32, device=DEV)
    assert torch.equal(P.dim_t(DEV), 10000 ** (2 * (t // 2) / 128)) and P.dim_t(DEV) is P.dim_t(torch.device(DEV))


def test_public_functions():
    import semi_detr_amd as s
    g = torch.Generator().manual_seed(3)
    ref = torch.rand(65, 2, 4, generator=g).to(DEV)
    vr = (0.5 + 0.5 * torch.rand(2, 4, 2, generator=g)).to(DEV)
    ref_input, embed = s.reference_inputs(ref, vr)
    assert ref_input.shape == (65, 2, 4, 4) and ref_input.transpose(0, 1).is_contiguous() and embed.shape == (65, 2, 512)
    case = {"mode": C.NONE, "eps": C.EPS, "segments": [{"ref": ref.cpu().numpy()}], "out_dtype": "fp32", "ref_dtype": "fp32",
            "vr": vr.cpu().numpy()}
    R.check(_statement_case(case), {"ref_input": _np(ref_input), "embed": _np(embed)}, "reference_inputs")
    for width in (2, 4):
        pos = ref[..., :width].contiguous()
        alone = s.gen_sineembed_for_position(pos)
        assert alone.shape == (65, 2, 128 * width) and alone.dtype == torch.float32
        R.within(f"gen_sineembed_for_position width {width}", _np(alone), R.embed(R.exact(_np(pos)), _statement_case(case)["dim_t"]))
    with pytest.raises(ValueError, match=r"Unknown pos_tensor shape\(-1\):3"):
        s.gen_sineembed_for_position(ref[..., :3])
    delta = torch.randn(65, 2, 4, generator=g).to(DEV).requires_grad_(True)
    y = s.refine_boxes(delta, ref)
    case = {"mode": C.REFINE, "eps": C.EPS, "segments": [{"ref": _np(ref), "delta": _np(delta)}], "out_dtype": "fp32",
            "ref_dtype": "fp32", "vr": None}
    R.check(case, {"new_ref": [_np(y)]}, "refine_boxes")
    y.sum().backward()
    assert delta.grad is not None and ref.grad is None
    with pytest.raises(NotImplementedError, match=r"9 levels \(1 \.\. 8\)"):
        s.reference_inputs(ref, torch.ones(2, 9, 2, device=DEV))
    with pytest.raises(NotImplementedError, match="valid_ratios requires grad"):
        s.reference_inputs(ref, vr.clone().requires_grad_(True))


# ------------------------------------------------------------------------------------------------------------------
# module level
# ------------------------------------------------------------------------------------------------------------------
NQ, BS, LEVELS, S_MEM = 65, 2, 4, 37


def _decoder_inputs(seed=0):
    g = torch.Generator().manual_seed(seed)
    torch.manual_seed(seed)                           # the modules' own initialisation draws from the global generator
    dec, fc_reg = T.Decoder(num_layers=2, levels=LEVELS, query_dim=4), T.box_heads(2)
    A.randomize_norms(dec, g)
    x = {"tgt": torch.randn(NQ, BS, T.D, generator=g), "memory": torch.randn(S_MEM, BS, T.D, generator=g),
         "refpoints_unsigmoid": torch.randn(NQ, BS, 4, generator=g), "valid_ratios": 0.5 + 0.5 * torch.rand(BS, LEVELS, 2, generator=g)}
    return dec.to(DEV), fc_reg.to(DEV), {k: v.to(DEV) for k, v in x.items()}


def _run_decoder(forward, dec, fc_reg, x, dtype):
    dec, fc_reg = (copy.deepcopy(dec).to(dtype), copy.deepcopy(fc_reg).to(dtype)) if dtype != torch.float32 else (dec, fc_reg)
    dec.zero_grad(), fc_reg.zero_grad()
    tgt, unsig = (x[k].to(dtype).requires_grad_(True) for k in ("tgt", "refpoints_unsigmoid"))
    hs, refs = forward(dec, tgt, x["memory"].to(dtype), refpoints_unsigmoid=unsig, valid_ratios=x["valid_ratios"].to(dtype),
                       fc_reg=fc_reg)
    outs = list(hs) + list(refs)
    assert len(hs) == 2 and len(refs) == 3 and all(r.requires_grad for r in refs)
    seeds = [torch.randn(o.shape, generator=torch.Generator().manual_seed(11 + i)).to(DEV) for i, o in enumerate(outs)]
    wrt = [tgt, unsig] + list(dec.ref_point_head.parameters()) + list(fc_reg.parameters()) + \
        [dec.layers[0].cross_attn.lin_r.weight, dec.layers[1].cross_attn.lin_r.weight, dec.norm.weight]
    grads = torch.autograd.grad(outs, wrt, [s.to(dtype) for s in seeds], allow_unused=True)
    return [o.detach() for o in outs], list(grads)


def test_decoder_forward_against_the_restated_decoder():
    import semi_detr_amd as s
    dec, fc_reg, x = _decoder_inputs()
    stock = lambda d, *a, **k: d(*a, **k)                                   # noqa: E731
    seen = []
    hooks = [layer.cross_attn.register_forward_pre_hook(lambda m, args: seen.append(args[1])) for layer in dec.layers]
    out_hip, grad_hip = _run_decoder(s.decoder_forward, dec, fc_reg, x, torch.float32)
    for h in hooks:
        h.remove()
    assert len(seen) == 2 and all(r.shape == (BS, NQ, LEVELS, 4) and r.is_contiguous() for r in seen)
    assert seen[0].requires_grad and not seen[1].requires_grad, "the points of layers >= 1 are detached, those of layer 0 are not"
    out_32, grad_32 = _run_decoder(stock, dec, fc_reg, x, torch.float32)
    out_64, grad_64 = _run_decoder(stock, dec, fc_reg, x, torch.float64)
    assert all(g is not None for g in grad_64)
    _judge("decoder_forward outputs", out_hip, out_32, out_64)
    _judge("decoder_forward gradients", grad_hip, grad_32, grad_64)
    # without fc_reg the points never change: the same structure, one entry in the list of points
    hs, refs = s.decoder_forward(dec, x["tgt"], x["memory"], refpoints_unsigmoid=x["refpoints_unsigmoid"], valid_ratios=x["valid_ratios"])
    hs_t, refs_t = dec(x["tgt"], x["memory"], refpoints_unsigmoid=x["refpoints_unsigmoid"], valid_ratios=x["valid_ratios"])
    assert len(hs) == 2 and len(refs) == len(refs_t) == 1 and refs[0].shape == (BS, NQ, 4)
    assert float((hs[1] - hs_t[1]).detach().abs().max()) < 1e-3


def _head_inputs(layers=6, seed=5):
    g = torch.Generator().manual_seed(seed)
    torch.manual_seed(seed)
    fc_reg = T.box_heads(layers).to(DEV)
    hs = [torch.randn(BS, NQ, T.D, generator=g).to(DEV) for _ in range(layers)]
    reference = [torch.rand(NQ, BS, 4, generator=g).to(DEV) for _ in range(layers + 1)]
    return fc_reg, hs, reference


def _run_head(fn, fc_reg, hs, reference, dtype):
    fc_reg = copy.deepcopy(fc_reg).to(dtype) if dtype != torch.float32 else fc_reg
    fc_reg.zero_grad()
    hs = [h.to(dtype).requires_grad_(True) for h in hs]
    leaves = [r.to(dtype).requires_grad_(True) for r in reference]
    out = fn(fc_reg, hs, [r.transpose(0, 1) for r in leaves])               # the head gets (bs, nq, 4) transposes
    seed = torch.randn(out.shape, generator=torch.Generator().manual_seed(2)).to(DEV).to(dtype)
    grads = torch.autograd.grad([out], hs + leaves[:-1] + list(fc_reg.parameters()), [seed])
    return [out.detach()], list(grads)


def test_box_outputs_against_the_restated_head_loop():
    import semi_detr_amd as s
    fc_reg, hs, reference = _head_inputs()
    out_hip, grad_hip = _run_head(s.box_outputs, fc_reg, hs, reference, torch.float32)
    out_32, grad_32 = _run_head(T.box_outputs, fc_reg, hs, reference, torch.float32)
    out_64, grad_64 = _run_head(T.box_outputs, fc_reg, hs, reference, torch.float64)
    assert out_hip[0].shape == (6, BS, NQ, 4) and out_hip[0].is_contiguous()
    _judge("box_outputs", out_hip, out_32, out_64)
    _judge("box_outputs gradients (hs, reference[l], fc_reg)", grad_hip, grad_32, grad_64)
    # the same launch, element by element
    deltas = [f(h) for f, h in zip(fc_reg, hs)]
    case = {"mode": C.REFINE, "eps": C.EPS, "out_dtype": "fp32", "ref_dtype": "fp32", "vr": None,
            "segments": [{"ref": _np(r), "delta": _np(d.transpose(0, 1))} for r, d in zip(reference, deltas)]}
    R.check(case, {"new_ref": [_np(o.transpose(0, 1)) for o in out_hip[0]]}, "box_outputs")


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
def test_autocast_gives_the_restatements_dtypes(dtype):
    import semi_detr_amd as s
    dec, fc_reg, x = _decoder_inputs(1)
    kw = dict(refpoints_unsigmoid=x["refpoints_unsigmoid"], valid_ratios=x["valid_ratios"], fc_reg=fc_reg)
    head_fc, hs, reference = _head_inputs(3)
    head_refs = [r.transpose(0, 1) for r in reference]
    g = torch.Generator().manual_seed(4)
    delta16, ref16 = torch.randn(NQ, BS, 4, generator=g).to(DEV).to(dtype), torch.rand(NQ, BS, 4, generator=g).to(DEV).to(dtype)
    with torch.autocast("cuda", dtype=dtype):
        hs_t, refs_t = dec(x["tgt"], x["memory"], **kw)
        hs_h, refs_h = s.decoder_forward(dec, x["tgt"], x["memory"], **kw)
        assert [t.dtype for t in hs_h + refs_h] == [t.dtype for t in hs_t + refs_t]
        assert s.box_outputs(head_fc, hs, head_refs).dtype == T.box_outputs(head_fc, hs, head_refs).dtype == torch.float32
        # log is on autocast's fp32 list: 16-bit operands give fp32 points there, and their own dtype outside
        assert s.refine_boxes(delta16, ref16).dtype == T.refine(delta16, ref16).dtype == torch.float32
        assert s.refine_boxes(delta16, ref16.float()).dtype == T.refine(delta16, ref16.float()).dtype == torch.float32
        ri_h, em_h = s.reference_inputs(ref16, x["valid_ratios"])
        ri_t, em_t = T.reference_inputs(ref16, x["valid_ratios"])
        assert (ri_h.dtype, em_h.dtype) == (ri_t.dtype, em_t.dtype) == (torch.float32, torch.float32)
    assert s.refine_boxes(delta16, ref16).dtype == T.refine(delta16, ref16).dtype == dtype
    for a, b in zip(refs_h, refs_t):
        assert float((a.detach().float() - b.detach().float()).abs().max()) < 2e-2
