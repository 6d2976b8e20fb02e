"""GPU: the transformer mirrors -- ``add_norm``, ``self_attn``, ``query_select`` -- under ``torch.autocast`` (bf16, fp16) and as
``.half()`` modules, with operands of mixed dtypes (inputs: tests/mixed_precision_cases.py; the judges are checked on the CPU
by tests/test_mixed_precision_ref.py).

Dtypes are never written down here: what a result's dtype has to be is read from stock torch running the restated sequence
(``F.layer_norm(x + residual) + pos``, ``nn.MultiheadAttention``, tests/query_select_torch_restated.py,
tests/add_norm_torch_restated.py) in the same context on the same GPU.

Values: the arithmetic is fp32 on the exactly up-cast inputs and each result that leaves in a 16-bit type is rounded once.
Against the float64 statement of the up-cast problem an fp32 result stays within the derived bound B of add_norm_ref64 /
self_attn_ref64 / query_select_ref64 and a 16-bit result within B + u16 (|ref| + B) + s16 (tests/msda_h16_ref.py); no new factor.
The fp32 residual stream is the sharp case: its bound has no 16-bit term, so a ``y`` that passed through bf16 is off by up to 2^-9
relative against a bound near 1e-6.

Run with -s to see the worst err / bound of every result.
"""
import copy
import types

import numpy as np
import pytest
import torch
from torch import nn
from torch.nn import functional as F

import add_norm_torch_restated as T
import mixed_precision_cases as M
import query_select_ref64 as QR
import query_select_torch_restated as QT
import self_attn_cases as SC
import self_attn_ref64 as SR
from msda_h16_ref import torch_dtype
from test_gpu_add_norm import FACTOR
from test_gpu_self_attn import _poison
from test_query_select_ref import diff

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _np(t):
    return None if t is None else t.detach().float().cpu().numpy()


def _kind(t):
    """'f32' / 'h16' / None of a tensor (anything else is an error)"""
    if t is None:
        return None
    assert t.dtype in (torch.float32, torch.float16, torch.bfloat16), t.dtype
    return "f32" if t.dtype == torch.float32 else "h16"


def _place(a, kind, dt, layout="contiguous"):
    """a float32 array (holding 16-bit values exactly where ``kind`` is 'h16') on the GPU in its dtype and memory layout"""
    if a is None:
        return None
    t = torch.from_numpy(np.array(a)).to(DEV)
    if kind == "h16":
        t = t.to(torch_dtype(dt))
    return t.transpose(0, 1).contiguous().transpose(0, 1) if layout == "transposed" else t


# ------------------------------------------------------------------------------------------------------------------
# 1. add_layer_norm / LayerNorm: the dtype matrix
# ------------------------------------------------------------------------------------------------------------------
ADD_NORM = ("y", "q", "dx", "dx_res", "dpos", "dweight", "dbias")


def _add_norm_run(case, op, context):
    """forward + backward of ``op(x, residual, weight, bias, eps, pos) -> y | (y, q)`` on fresh leaves in the context ->
    {name: tensor or None} for ADD_NORM"""
    dt, k, lay = case["dtype16"], case["kinds"], case["layout"]
    x, res, pos = (_place(case[n], k[n], dt, lay) for n in ("x", "residual", "pos"))
    w, b = (_place(case[n], k[n], dt) for n in ("weight", "bias"))
    for t in (x, res, pos, w, b):
        if t is not None:
            t.requires_grad_(True)
    shape = tuple(x.shape)
    _poison(shape, shape)
    with M.autocast(context):
        out = op(x, res, w, b, case["eps"], pos)
    y, q = out if pos is not None else (out, None)
    seeds = [torch.from_numpy(np.array(case["gy"])).to(DEV).to(y.dtype)]
    if q is not None:
        seeds.append(torch.from_numpy(np.array(case["gq"])).to(DEV).to(q.dtype))
    _poison(shape, (256,), (256,))
    torch.autograd.backward([y] + ([q] if q is not None else []), seeds)
    return dict(y=y.detach(), q=None if q is None else q.detach(), dx=x.grad, dx_res=None if res is None else res.grad,
                dpos=None if pos is None else pos.grad, dweight=w.grad, dbias=b.grad, gq=seeds[-1] if q is not None else None)


def _stock_add_norm(x, res, w, b, eps, pos):
    y = F.layer_norm(x if res is None else x + res, (256,), w, b, eps)
    return y if pos is None else (y, y + pos)


@pytest.mark.parametrize("base,combo,context", M.add_norm_names(), ids=["/".join(n) for n in M.add_norm_names()])
def test_add_layer_norm_dtype_matrix(base, combo, context):
    import semi_detr_amd as s
    case = M.add_norm_case(base, combo, context)

    def mirror(x, res, w, b, eps, pos):
        if combo not in ("bare", "res16"):
            return s.add_layer_norm(x, res, w, b, eps, pos)
        # LayerNorm.forward, as an adopted enc_output_norm is called, on this run's leaves in the Parameters' place
        return s.LayerNorm.forward(types.SimpleNamespace(weight=w, bias=b, eps=eps), x, res, pos)
    stock = _add_norm_run(case, _stock_add_norm, context)
    got = _add_norm_run(case, mirror, context)
    # dtypes: stock torch's, which are the derived ones
    want = {n: _kind(stock[n]) for n in ADD_NORM}
    assert want == M.derived_dtypes(case), ("stock torch contradicts the derivation", want, M.derived_dtypes(case))
    for n in ADD_NORM:
        assert (got[n] is None) == (stock[n] is None) and (got[n] is None or got[n].dtype == stock[n].dtype), \
            f"{case['name']}: {n} is {None if got[n] is None else got[n].dtype}, stock torch gives " \
            f"{None if stock[n] is None else stock[n].dtype}"
    assert got["y"].is_contiguous() and (got["q"] is None or got["q"].is_contiguous())
    # the gradient of residual is dx in the residual's dtype, that of pos is gq in pos's dtype
    if got["dx_res"] is not None and got["dx_res"].dtype == torch.float32:
        assert torch.equal(got["dx"], got["dx_res"].to(got["dx"].dtype)), "x.grad is not residual.grad rounded once"
    elif got["dx_res"] is not None:
        assert torch.equal(got["dx"], got["dx_res"])
    if got["dpos"] is not None:
        assert torch.equal(got["dpos"], got["gq"].to(got["dpos"].dtype)), "the gradient of pos is gq in pos's dtype"
    # bitwise: the fp32 call on the up-cast tensors, each result converted once into its dtype
    up = dict(case, kinds={n: (None if v is None else "f32") for n, v in case["kinds"].items()})
    plain = _add_norm_run(up, lambda *a: s.add_layer_norm(*a), "half_module")          # autocast disabled, everything fp32
    assert all(plain[n] is None or plain[n].dtype == torch.float32 for n in ADD_NORM)
    for n in ADD_NORM:
        if got[n] is not None:
            assert torch.equal(got[n], plain[n].to(got[n].dtype)), f"{case['name']}: {n} is not the fp32 result rounded once"
    # values: every element within B, or B + u16 (|ref| + B) + s16 where it left in 16 bits
    judged = {n: _np(got[n]) for n in ("y", "q", "dx", "dx_res", "dweight", "dbias") if got[n] is not None}
    judged["kinds"] = {n: _kind(got[n]) for n in judged}
    rep = M.check_add_norm16(case, judged, M.add_norm_reference(base, combo, context))
    print("\n" + " ".join(f"{n}[{judged['kinds'][n]}]={v:.3g}" for n, v in rep.items()) + f"  {case['name']}")


# ------------------------------------------------------------------------------------------------------------------
# 2. masked_attention and MultiheadAttention
# ------------------------------------------------------------------------------------------------------------------
def _attn_run(p, dt):
    import semi_detr_amd as s
    t16 = torch_dtype(dt)
    q, k, v = (torch.from_numpy(np.array(p[n])).to(DEV).to(t16) for n in "qkv")
    if p["layout"] == "packed" and q.shape == k.shape:
        E = q.shape[2]
        buf = torch.cat([q, k, v], dim=2).requires_grad_(True)       # ONE 16-bit (L, B, 3E) buffer: rows_f32 has to copy
        q, k, v = buf[..., :E], buf[..., E:2 * E], buf[..., 2 * E:]
        grads = lambda: [buf.grad[..., i * E:(i + 1) * E] for i in range(3)]
    else:
        q, k, v = (t.requires_grad_(True) for t in (q, k, v))
        grads = lambda: [t.grad for t in (q, k, v)]
    mask = None if p["mask"] is None else torch.from_numpy(p["mask"]).to(DEV)
    _poison(tuple(q.shape), tuple(k.shape))
    out = s.masked_attention(q, k, v, p["heads"], attn_mask=mask, scale=p["scale"])
    assert out.shape == q.shape and out.dtype == t16 and out.is_contiguous()
    _poison(tuple(q.shape), tuple(k.shape), tuple(k.shape))
    out.backward(torch.from_numpy(np.array(p["gout"])).to(DEV).to(t16))
    g = grads()
    assert all(t.dtype == t16 for t in g), [t.dtype for t in g]
    return dict(out=_np(out), dq=_np(g[0]), dk=_np(g[1]), dv=_np(g[2]))


@pytest.mark.parametrize("dt", M.DTYPES)
@pytest.mark.parametrize("name", M.ATTN_CASES)
def test_masked_attention_on_16_bit_operands(name, dt):
    p, ref = M.attn_case(name, dt), M.attn_reference(name, dt)
    if dt == "fp16":          # the range condition, from the CPU's numbers: no result can leave the range of fp16
        assert all(v < M.MAX16["fp16"] for v in M.attn_reach(name, dt).values())
    got = _attn_run(p, dt)
    rep = SR.check_self_attn(p, got, f"{name} {dt}", ref, dtype16=dt)
    print("\n" + SR.table(f"{name} {dt}", rep))
    again = _attn_run(p, dt)
    assert all(got[n].tobytes() == again[n].tobytes() for n in got), "not bit-identical from run to run"
    assert all(np.isfinite(v).all() for v in got.values())


def _mha_problem():
    torch.manual_seed(0)
    E, H, L, B = 256, 8, 70, 2
    holder = nn.Module()
    holder.self_attn = nn.MultiheadAttention(E, H, dropout=0.0)
    holder.to(DEV)
    tgt, pos = torch.randn(L, B, E, device=DEV), torch.randn(L, B, E, device=DEV)
    mask = torch.from_numpy(SC.dn_mask(3, 4, 46)).to(DEV)
    g = torch.from_numpy(SR.grad_pattern((L, B, E), 3)).to(DEV)
    return holder, tgt, pos, mask, g


@pytest.mark.parametrize("context", ["autocast_bf16", "autocast_fp16"])
def test_converted_multihead_attention_under_autocast(context):
    """The inputs of test_converted_decoder_layer_gives_the_same_parameter_gradients (tests/test_gpu_self_attn.py) and its
    limit: per tensor |mirror - f64| <= 4 |stock - f64|.  Here both fp32-parameter sides run their GEMMs in 16 bits."""
    import semi_detr_amd as s
    holder, tgt, pos, mask, g = _mha_problem()
    g16 = g.to(torch_dtype(M.DTYPE16[context]))          # the seed both sides receive: the output is 16-bit under autocast
    mirror = copy.deepcopy(holder)
    assert s.convert_self_attention(mirror) == 1 and type(mirror.self_attn) is s.MultiheadAttention
    names = [n for n, _ in holder.named_parameters()]
    assert [n for n, _ in mirror.named_parameters()] == names

    def run(m, exact=False):
        cast = (lambda t: t.double()) if exact else (lambda t: t)
        query, value = cast(tgt + pos).requires_grad_(True), cast(tgt).clone().requires_grad_(True)
        with M.autocast("half_module" if exact else context):
            out = m.self_attn(query, query, value, attn_mask=mask)[0]
        out.backward(cast(g16).to(out.dtype))
        return [out.detach(), query.grad, value.grad] + [p.grad for p in m.parameters()]
    exact = run(copy.deepcopy(holder).double(), exact=True)
    stock, got = run(holder), run(mirror)
    assert stock[0].dtype == torch_dtype(M.DTYPE16[context]), "stock torch returns a 16-bit output under autocast"
    for what, x, a, b in zip(["out", "g_query", "g_value"] + names, exact, stock, got):
        assert b.dtype == a.dtype, f"{what}: {b.dtype}, stock torch gives {a.dtype}"
        ref_err, err = float((a.double() - x).abs().max()), float((b.double() - x).abs().max())
        print(f"{context} {what:28s} |stock autocast - fp64| = {ref_err:.3g}  |mirror - fp64| = {err:.3g}")
        assert torch.isfinite(b).all() and err <= 4.0 * ref_err, (what, err, ref_err)


# ------------------------------------------------------------------------------------------------------------------
# 3. query selection on 16-bit logits
# ------------------------------------------------------------------------------------------------------------------
def _report(what, err, bound):
    worst = float((err[bound > 0] / bound[bound > 0]).max(initial=0.0))
    print(f"[mixed select] {what}: worst err / bound = {worst:.3f}")
    assert (err <= bound).all(), (what, worst)


@pytest.mark.parametrize("operands", ["logits16", "all16"])
@pytest.mark.parametrize("dt", M.DTYPES)
def test_select_queries_on_16_bit_logits(dt, operands):
    """``logits16``: what autocast hands over (16-bit ``enc_outputs_class``, everything else fp32); ``all16``: every floating
    operand 16-bit.  The tokens are exactly the first k of (key descending, token ascending) on the up-cast keys.  ``refpoint``
    and ``tgt`` are gathers, hence bitwise copies; ``init_box_proposal`` and ``ref_enc`` are sigmoids of gathered rows
    (transformer.py:1398, 1334) and stay within query_select_ref64's bound, widened where torch returns them in 16 bits."""
    import semi_detr_amd as s
    c = M.select_case(dt)
    k, S = c["k"], c["keys"].shape[1]
    t16 = torch_dtype(dt)
    kind = "h16" if operands == "all16" else "f32"
    r16 = (lambda a: M.round16(a, dt)) if operands == "all16" else (lambda a: np.asarray(a, np.float32))
    prop_np = r16(c["p"]["prop"].astype(np.float32))                       # +inf where the token is padded or invalid
    with np.errstate(invalid="ignore"):
        coord_np = r16(c["reg"] + prop_np)
    om_np = r16(QR.masked_memory(c["memory"], c["p"]["valid"]))
    lg = _place(c["logits"], "h16", dt)
    prop = _place(prop_np, kind, dt)

    def leaves():
        return _place(coord_np, kind, dt).requires_grad_(True), _place(om_np, kind, dt).requires_grad_(True)
    g_tgt, g_enc, g_ref = QR.grad_pattern((M.SEL_N, k, M.SEL_D), 1), QR.grad_pattern((M.SEL_N, k, 4), 2), QR.grad_pattern((M.SEL_N, k, 4), 5)

    def run(select):
        coord, outmem = leaves()
        res = select(lg, coord, prop, outmem, k)
        _, ref, _, tgt, enc = res
        seeds = [torch.from_numpy(a).to(DEV).to(t.dtype) for a, t in ((g_tgt, tgt), (g_enc, enc), (g_ref, ref))]
        torch.autograd.backward([tgt, enc, ref], seeds)
        return [t.detach() for t in res] + [coord.grad, outmem.grad]
    stock = run(QT.select)
    got = run(s.select_queries)
    names = ["topk_proposals", "refpoint", "init_box_proposal", "tgt", "ref_enc", "grad coord", "grad output_memory"]
    for n, a, b in zip(names, stock, got):
        assert b.dtype == a.dtype and b.shape == a.shape, f"{n}: {b.dtype} {tuple(b.shape)}, stock torch gives {a.dtype} {tuple(a.shape)}"
    idx, ref, init, tgt, enc, gc, gm = got
    want = M.select_numpy(c["keys"], k)
    assert np.array_equal(idx.cpu().numpy(), want), "not the first k of (key descending, token ascending)"
    rows = np.arange(M.SEL_N)[:, None]
    assert _np(ref).tobytes() == coord_np[rows, want].tobytes() and _np(tgt).tobytes() == om_np[rows, want].tobytes()
    h16 = lambda t: dt if _kind(t) == "h16" else None                      # widen the bound of what left in 16 bits
    g = QR.gather(want, coord_np, prop_np.astype(np.float64), np.zeros_like(prop_np, np.float64), om_np)
    _report(f"{dt} {operands} ref_enc", diff(_np(enc), g["ref_enc"]), QR.widen16(g["ref_bound"], g["ref_enc"], h16(enc)))
    _report(f"{dt} {operands} init_box", diff(_np(init), g["init_box"]), QR.widen16(g["init_bound"], g["init_box"], h16(init)))
    gc64, bound, gm_want = QR.gather_backward(want, S, g["ref_enc"], g_ref, g_tgt, g_enc)
    assert _np(gm).tobytes() == gm_want.tobytes()                          # copies and zeros
    _report(f"{dt} {operands} grad coord", diff(_np(gc), gc64), QR.widen16(bound, gc64, h16(gc)))
    again = run(s.select_queries)
    assert all(torch.equal(a, b) for a, b in zip(got, again)), "not bit-identical from run to run"


@pytest.mark.parametrize("dt", M.DTYPES)
def test_gen_encoder_output_proposals_on_16_bit_memory(dt):
    import semi_detr_amd as s
    c = M.select_case(dt)
    t16 = torch_dtype(dt)
    mem_np = M.round16(c["memory"], dt)
    mask = torch.from_numpy(c["mask"]).to(DEV)
    g_np = QR.grad_pattern(mem_np.shape, 3)                                 # multiples of 1 / 8: exact in both 16-bit types

    def run(fn):
        mem = _place(mem_np, "h16", dt).requires_grad_(True)
        om, prop = fn(mem, mask, c["shapes"])
        om.backward(torch.from_numpy(g_np).to(DEV).to(om.dtype))
        return om.detach(), prop.detach(), mem.grad
    stock, got = run(QT.gen_proposals), run(s.gen_encoder_output_proposals)
    for n, a, b in zip(("output_memory", "output_proposals", "grad memory"), stock, got):
        assert b.dtype == a.dtype, f"{n}: {b.dtype}, stock torch gives {a.dtype}"
    om, prop, gmem = got
    assert om.dtype == t16 and prop.dtype == torch.float32 and gmem.dtype == t16
    valid = c["p"]["valid"]
    assert _np(om).tobytes() == QR.masked_memory(mem_np, valid).tobytes()
    assert _np(gmem).tobytes() == QR.masked_memory(g_np, valid).tobytes()
    p64 = prop.double().cpu().numpy()
    fin = np.isfinite(c["p"]["prop"])
    assert np.array_equal(np.isinf(p64) & (p64 > 0), ~fin)
    _report(f"{dt} proposals", np.abs(p64[fin] - c["p"]["prop"][fin]), c["p"]["bound"][fin])


# ------------------------------------------------------------------------------------------------------------------
# 4. the bound pieces in sequence under autocast
# ------------------------------------------------------------------------------------------------------------------
SHAPES = [(8, 6), (4, 3)]
K = 20


class _Chain(nn.Module):
    """Encoder, two-stage block and decoder of the restated modules (tests/add_norm_torch_restated.py) with a real
    ``nn.MultiheadAttention`` as the decoder layers' self-attention."""

    def __init__(self):
        super().__init__()
        self.enc = T.Encoder(2, 512)
        self.owner = nn.Module()                              # what two_stage_queries reads of DINOTransformer
        self.owner.enc_output, self.owner.enc_output_norm = nn.Linear(256, 256), nn.LayerNorm(256)
        self.owner.tgt_embed = nn.Embedding(K, 256)
        self.owner.num_queries, self.owner.embed_init_tgt, self.owner.two_stage_type = K, True, "standard"
        self.fc_enc_cls, self.fc_enc_reg = nn.Linear(256, 8), nn.Linear(256, 4)
        self.ref_point_head = nn.Linear(4, 256)               # the decoder's query_pos: a 16-bit GEMM output under autocast
        self.dec = T.DecoderStack(2, 512)
        for layer in self.dec.layers:
            layer.self_attn = nn.MultiheadAttention(256, 8, dropout=0.0)


def _select_given(idx, coord, anchors, memory):
    """query_select_torch_restated.select with the tokens given"""
    four = idx.unsqueeze(-1).repeat(1, 1, 4)
    boxes = torch.gather(coord, 1, four)
    return idx, boxes, torch.gather(anchors, 1, four).sigmoid(), \
        torch.gather(memory, 1, idx.unsqueeze(-1).repeat(1, 1, memory.shape[2])), boxes.sigmoid()


def _chain(m, mode, src, pos, pad, dn, idx=None):
    """One forward of the chain.  mode 'stock': every module's own forward and the restated selection (``idx``: the tokens are
    given instead); 'hip': encoder_forward, two_stage_queries, decoder_layer_forward.  -> dict of the tensors at the boundaries"""
    from semi_detr_amd import add_norm, query_select as Q
    shapes = torch.tensor(SHAPES, device=DEV)
    args = (shapes, shapes.new_tensor([0, SHAPES[0][0] * SHAPES[0][1]]), None, pad)
    rec = {}
    hooks = [m.owner.enc_output_norm.register_forward_hook(lambda mod, i, o: rec.__setitem__("output_memory", o)),
             m.fc_enc_cls.register_forward_hook(lambda mod, i, o: rec.__setitem__("logits", o))]
    try:
        if mode == "hip":
            memory = add_norm.encoder_forward(m.enc, src, pos, *args)[0]
            inner = Q.select_queries

            def recorder(*a):
                rec["select"] = inner(*a)
                return rec["select"]
            Q.select_queries = recorder
            try:
                refpoint, tgt, hs_enc, ref_enc, init = Q.two_stage_queries(m.owner, memory, pad, shapes, m.fc_enc_cls, m.fc_enc_reg,
                                                                           None, None)
            finally:
                Q.select_queries = inner
            hs_enc, ref_enc = hs_enc[0], ref_enc[0]
            assert hs_enc is rec["select"][3] or torch.equal(hs_enc, rec["select"][3])
        else:
            memory = m.enc(src, pos, *args)[0]
            om, prop = QT.gen_proposals(memory, pad, SHAPES)
            om = m.owner.enc_output_norm(m.owner.enc_output(om))
            coord = m.fc_enc_reg(om) + prop
            logits = m.fc_enc_cls(om)
            rec["select"] = QT.select(logits, coord, prop, om, K) if idx is None else _select_given(idx, coord, prop, om)
            _, undetached, init, hs_enc, ref_enc = rec["select"]
            refpoint = undetached.detach()
            tgt = m.owner.tgt_embed.weight[:K, None, :].repeat(1, src.shape[0], 1).transpose(0, 1)
        boxes = refpoint.sigmoid().transpose(0, 1)
        qpos = m.ref_point_head(boxes)
        tgt, mem_t = tgt.transpose(0, 1), memory.transpose(0, 1)
        layer_outs, inter = [], []
        for layer in m.dec.layers:
            kw = dict(tgt_query_pos=qpos, tgt_reference_points=boxes, memory=mem_t, self_attn_mask=dn)
            tgt = add_norm.decoder_layer_forward(layer, tgt, **kw) if mode == "hip" else layer(tgt, **kw)
            layer_outs.append(tgt)
            inter.append(m.dec.norm(tgt))
    finally:
        for h in hooks:
            h.remove()
    return dict(memory=memory, output_memory=rec["output_memory"], logits=rec["logits"], select=rec["select"],
                refpoint=refpoint, tgt=tgt, init=init, query_pos=qpos, layer_outs=layer_outs, inter=inter, hs_enc=hs_enc,
                ref_enc=ref_enc)


def _boundaries(r):
    named = [("memory", r["memory"]), ("output_memory", r["output_memory"]), ("logits", r["logits"]), ("query_pos", r["query_pos"]),
             ("refpoint_embed", r["refpoint"]), ("init_box_proposal", r["init"])]
    named += [(f"select[{i}]", t) for i, t in enumerate(r["select"])]
    named += [(f"layer[{i}]", t) for i, t in enumerate(r["layer_outs"])] + [(f"intermediate[{i}]", t) for i, t in enumerate(r["inter"])]
    return named


@pytest.mark.parametrize("context", ["autocast_bf16", "autocast_fp16"])
def test_encoder_two_stage_decoder_in_sequence_under_autocast(context):
    import semi_detr_amd as s
    g = torch.Generator().manual_seed(21)
    torch.manual_seed(21)
    model = _Chain()
    T.randomize_norms(model, g)
    model.to(DEV)
    S = sum(h * w for h, w in SHAPES)
    src, pos = (torch.randn(2, S, 256, generator=g).to(DEV) for _ in range(2))
    seeds = [torch.randn(K, 2, 256, generator=g).to(DEV) for _ in range(2)] + \
        [torch.randn(2, K, 256, generator=g).to(DEV), torch.randn(2, K, 4, generator=g).to(DEV)]
    pad = torch.from_numpy(M.band_mask(SHAPES, [(1.0, 1.0), (0.75, 0.67)])).to(DEV)
    dn = torch.from_numpy(SC.dn_mask(2, 2, K - 8)).to(DEV)
    hip_model = copy.deepcopy(model)
    assert s.convert_self_attention(hip_model) == 2 and s.convert_layer_norms(hip_model) == 4 + 1 + 6 + 1
    names = [n for n, _ in model.named_parameters()]
    assert [n for n, _ in hip_model.named_parameters()] == names

    def run(m, mode, exact=False, idx=None):
        cast = (lambda t: t.double()) if exact else (lambda t: t)
        s_, p_ = cast(src).clone().requires_grad_(True), cast(pos).clone().requires_grad_(True)
        with M.autocast("half_module" if exact else context):
            r = _chain(m, mode, s_, p_, pad, dn, idx)
        outs = r["inter"] + [r["hs_enc"], r["ref_enc"]]
        grads = torch.autograd.grad(outs, [s_, p_] + list(m.parameters()), [cast(t).to(o.dtype) for t, o in zip(seeds, outs)],
                                    allow_unused=True)
        return r, [r["memory"].detach()] + [o.detach() for o in outs] + list(grads)
    stock_r, stock = run(model, "stock")
    hip_r, hip = run(hip_model, "hip")                                      # it runs without raising
    # every boundary in stock torch's dtype
    for (n, a), (n2, b) in zip(_boundaries(stock_r), _boundaries(hip_r)):
        assert n == n2 and b.dtype == a.dtype and b.shape == a.shape, f"{n}: hip {b.dtype} {tuple(b.shape)}, stock {a.dtype} {tuple(a.shape)}"
    what = ["memory", "intermediate[0]", "intermediate[1]", "hs_enc", "ref_enc", "grad src", "grad pos"] + ["grad " + n for n in names]
    for n, a, b in zip(what, stock, hip):
        assert (a is None) == (b is None) and (a is None or a.dtype == b.dtype), f"{n}: hip {None if b is None else b.dtype}, " \
            f"stock {None if a is None else a.dtype}"
    # the hip side's selection, exactly, on the logits that side computed (the two sides' output_memory are the results of
    # two LayerNorm implementations, so their logits are close, not bitwise equal)
    keys = QR.keys_of(_np(hip_r["logits"]))
    hip_idx = hip_r["select"][0]
    assert np.array_equal(hip_idx.cpu().numpy(), QR.topk(keys, K))
    print(f"\n{context}: logits bitwise equal on both sides: {torch.equal(stock_r['logits'], hip_r['logits'])}; "
          f"same tokens: {torch.equal(stock_r['select'][0], hip_idx)}")
    # each side against the float64 chain that is handed that side's tokens
    model64 = copy.deepcopy(model).double()
    f64_stock = run(model64, "stock", exact=True, idx=stock_r["select"][0])[1]
    f64_hip = f64_stock if torch.equal(stock_r["select"][0], hip_idx) else run(model64, "stock", exact=True, idx=hip_idx)[1]
    assert len(hip) == len(stock) == len(f64_hip) == len(f64_stock) == len(what)
    worst = 0.0
    for n, h, r, dh, ds in zip(what, hip, stock, f64_hip, f64_stock):
        if dh is None:
            assert h is None and r is None and ds is None, n
            continue
        scale, err = float((r.double() - ds).abs().max()), float((h.double() - dh).abs().max())
        print(f"  {context} {n:44s} |hip - f64| = {err:.3e}  |stock - f64| = {scale:.3e}")
        assert torch.isfinite(h).all() and scale > 0, n
        worst = max(worst, err / scale)
        assert err <= FACTOR * scale, f"{n}: |hip - f64| = {err:.3e}, |stock autocast - f64| = {scale:.3e}"
    print(f"  chain {context}: {len(what)} tensors, worst |hip - f64| / |stock - f64| = {worst:.2f}")
