"""The detector's transformer as it is actually wired, with the real multi-scale deformable attention in every layer: the model,
inputs, the two drivers and the judges shared by tests/test_detector_chain_ref.py (CPU) and tests/test_gpu_detector_chain.py (GPU).

One model of the restated pieces: ``input_proj_torch_restated.build_input_proj`` (two backbone levels, two extra levels),
``add_norm_torch_restated.Encoder`` with the real ``get_reference_points`` (transformer.py:675-691), the two-stage block,
``ref_points_torch_restated.Decoder`` with ``nn.MultiheadAttention`` self-attention, ``box_heads`` and ``box_outputs``.  Every
encoder ``self_attn`` and decoder ``cross_attn`` is ``msda_torch_restated.MSDeformAttn``.

  * ``stock_forward``: every module's own forward (the baseline, and in float64 the reference);
  * ``hip_forward``: ``project_pyramid`` -> ``encoder_forward(query=)`` -> ``two_stage_queries`` -> ``ref_points.decoder_forward
    (fc_reg=)`` -> ``ref_points.box_outputs`` on ``hip_model`` (the attention modules replaced by ``semi_detr_amd.MSDeformAttn``,
    then ``convert_layer_norms`` and ``convert_self_attention``).

The rule is that of tests/test_gpu_add_norm.py, per tensor: ``max |side - f64| <= FACTOR * max |stock - f64|``, the float64 chain
handed the side's own selected tokens.

Bilinear kinks.  d out / d location jumps where a sample crosses a pixel-centre line, so a sample that two fp32 sides put on
different sides of a line breaks the rule for no fault.  In the ``init`` state (``sampling_offsets.weight = 0``, references
detached) the only results that see d out / d location are each attention's ``sampling_offsets.{weight, bias}.grad``.  ``taps``
hooks, per attention call, the reference points, the query, the offsets and the gradient of the offsets; ``kink_report`` judges
that gradient elementwise without the samples within 2 E px of a line (E: how far a side's pixel coordinates are from the
float64 chain's, plus 4 fp32 ulps of the level extent for the arithmetic inside a kernel), and the two parameter gradients
against the float64 Linear backward of the side's own hooked gradient.

Under autocast the same holds for a ReLU: ``relu_taps`` hooks the box heads' Linears in front of one and ``relu_report`` judges
them at the op boundary without the units whose argument a side puts on the other side of 0 than the float64 chain does.

``MUTANTS`` are deliberate handoff mistakes of the stock driver; the CPU test shows the rule rejects each.
"""
import contextlib
import copy

import numpy as np
import torch
from torch import nn

import add_norm_torch_restated as A
import input_proj_torch_restated as T
import msda_torch_restated as MT
import query_select_torch_restated as QT
import ref_points_torch_restated as RP
import self_attn_cases as SC
from mixed_precision_cases import band_mask
from msda_lattice_cases import MASK_FRACS, POW2

D, HEADS, LEVELS, POINTS = 256, 8, 4, 4
N, K = 2, 20
CHANNELS = (16, 24)                         # two backbone levels; levels 2 and 3 are the stride-2 convs of input_proj
PYRAMIDS = {"patch": [(12, 16), (6, 8), (3, 4), (2, 2)], "window": POW2}
POLICY = {"patch": "patch", "window": "window"}        # the encoder kernels are pinned: the adaptive choice depends on timing
STATES = ("init", "trained")
CONTEXTS = ("fp32_fused", "fp32_unfused", "autocast_bf16", "autocast_bf16_fused16", "autocast_fp16")
FRACTION = 5.0 / 32.0                       # of every sampling_offsets.bias: an odd multiple of 1 / 32 (lattice_margin)
MARGIN = 1.0 / 32.0
LEFT_OUT_CAP = 0.01
KEY_GAP = 1e-4                              # between the first K + 1 keys: 50 x the fp32 chain's error of the logits (2e-6)
MUTANTS = ("no_valid_ratio", "encoder_mask_dropped_layer1", "decoder_memory_mask_dropped", "layer0_without_pos",
           "stale_ref_input", "reference_not_detached", "level_start_shifted")


def is_autocast(context):
    return context.startswith("autocast")


def autocast(context, device):
    if not is_autocast(context):
        return contextlib.nullcontext() if torch.device(device).type == "cpu" else torch.autocast("cuda", enabled=False)
    return torch.autocast(torch.device(device).type, dtype=torch.float16 if context.endswith("fp16") else torch.bfloat16)


# ------------------------------------------------------------------------------------------------------------------ the model
def get_reference_points(spatial_shapes, valid_ratios, device):
    """transformer.py:675-691: a level's pixel centres over its valid extent, times every level's valid ratio -> (N, S, L, 2)"""
    per_level = []
    for lvl, (H, W) in enumerate(torch.as_tensor(spatial_shapes).tolist()):
        cy = (torch.arange(H, dtype=torch.float32, device=device) + 0.5)[:, None].expand(H, W).reshape(-1)
        cx = (torch.arange(W, dtype=torch.float32, device=device) + 0.5)[None, :].expand(H, W).reshape(-1)
        y = cy[None] / (valid_ratios[:, None, lvl, 1] * H)
        x = cx[None] / (valid_ratios[:, None, lvl, 0] * W)
        per_level.append(torch.stack((x, y), -1))
    return torch.cat(per_level, 1)[:, :, None] * valid_ratios[:, None]


def _unscaled_reference_points(spatial_shapes, valid_ratios, device):
    ones = torch.ones_like(valid_ratios)
    return get_reference_points(spatial_shapes, ones, device)


class ChainEncoder(A.Encoder):
    get_reference_points = staticmethod(get_reference_points)


class Detector(nn.Module):
    def __init__(self):
        super().__init__()
        self.input_proj = T.build_input_proj(CHANNELS, LEVELS)
        self.enc = ChainEncoder(2, 512)
        for layer in self.enc.layers:
            layer.self_attn = MT.MSDeformAttn(D, LEVELS, HEADS, POINTS)
        self.owner = nn.Module()                              # what two_stage_queries reads of DINOTransformer
        self.owner.enc_output, self.owner.enc_output_norm = nn.Linear(D, D), nn.LayerNorm(D)
        self.owner.tgt_embed = nn.Embedding(K, D)
        self.owner.num_queries, self.owner.embed_init_tgt, self.owner.two_stage_type = K, True, "standard"
        self.fc_enc_cls, self.fc_enc_reg = nn.Linear(D, 8), nn.Linear(D, 4)
        self.dec = RP.Decoder(2, LEVELS, 4, 512)
        for layer in self.dec.layers:
            layer.cross_attn = MT.MSDeformAttn(D, LEVELS, HEADS, POINTS)
            layer.self_attn = nn.MultiheadAttention(D, HEADS, dropout=0.0)
        self.fc_reg = RP.box_heads(2)


def attentions(model):
    """[(name, module)] of the deformable attentions in call order"""
    return [(f"enc.layers.{i}.self_attn", l.self_attn) for i, l in enumerate(model.enc.layers)] + \
        [(f"dec.layers.{i}.cross_attn", l.cross_attn) for i, l in enumerate(model.dec.layers)]


def build_model(state, seed=7):
    """``seed`` is committed with the conditions of tests/test_detector_chain_ref.py: a top-k whose keys are KEY_GAP apart"""
    assert state in STATES
    torch.manual_seed(seed)
    g = torch.Generator().manual_seed(seed + 1)
    model = Detector()
    A.randomize_norms(model, g)
    T.randomize_norms(model, g)
    with torch.no_grad():
        for _, att in attentions(model):
            so, aw = att.sampling_offsets, att.attention_weights
            so.weight.zero_()
            if state == "trained":
                so.weight.copy_(0.02 * torch.randn(so.weight.shape, generator=g))
            whole = torch.randint(-3, 3, so.bias.shape, generator=g)          # -3 .. 2: |b| <= 3, at most 7 significant bits
            so.bias.copy_(whole.float() + FRACTION)
            aw.weight.copy_(0.05 * torch.randn(aw.weight.shape, generator=g))
            aw.bias.copy_(0.3 * torch.randn(aw.bias.shape, generator=g))
            att.value_proj.bias.copy_(0.1 * torch.randn(D, generator=g))
            att.output_proj.bias.copy_(0.1 * torch.randn(D, generator=g))
    return model


def hip_model(model):
    """A deepcopy whose attentions are ``semi_detr_amd.MSDeformAttn`` with the same parameters, the LayerNorms and the decoder
    self-attentions converted"""
    import semi_detr_amd as s
    m = copy.deepcopy(model)
    names = [n for n, _ in m.named_parameters()]
    for holder, attr in [(l, "self_attn") for l in m.enc.layers] + [(l, "cross_attn") for l in m.dec.layers]:
        old = getattr(holder, attr)
        new = s.MSDeformAttn(D, LEVELS, HEADS, POINTS).to(old.value_proj.weight.device)
        new.load_state_dict(old.state_dict(), strict=True)
        setattr(holder, attr, new)
    assert s.convert_layer_norms(m) == 4 + 1 + 6 + 1 and s.convert_self_attention(m) == 2
    assert [n for n, _ in m.named_parameters()] == names
    return m


def set_context(hip, context):
    for _, att in attentions(hip):
        att.fuse_prologue = context != "fp32_unfused"
        att.native_16bit = True
        att.fuse_prologue_16bit = context == "autocast_bf16_fused16"


def inputs(pyramid, seed=9):
    """dict(feats: the two backbone maps, pos (N, S, 256), pad (N, S) bool, vr (N, L, 2) [w, h] from the mask, dn, seeds)"""
    shapes = PYRAMIDS[pyramid]
    g = torch.Generator().manual_seed(seed + len(pyramid))
    S = sum(h * w for h, w in shapes)
    feats = [torch.randn(N, c, h, w, generator=g) for c, (h, w) in zip(CHANNELS, shapes)]
    pos = torch.randn(N, S, D, generator=g)
    pad = torch.from_numpy(band_mask(shapes, MASK_FRACS))
    vr, start = [], 0
    for h, w in shapes:
        m = pad[:, start:start + h * w].view(N, h, w)
        vr.append(torch.stack([(~m[:, 0, :]).sum(1).float() / w, (~m[:, :, 0]).sum(1).float() / h], -1))
        start += h * w
    seeds = [torch.randn(N, K, D, generator=g), torch.randn(N, K, D, generator=g), torch.randn(2, N, K, 4, generator=g),
             torch.randn(N, K, D, generator=g), torch.randn(N, K, 4, generator=g)]
    return dict(feats=feats, pos=pos, pad=pad, vr=torch.stack(vr, 1), dn=torch.from_numpy(SC.dn_mask(2, 2, K - 8)), seeds=seeds,
                shapes=shapes)


# ------------------------------------------------------------------------------------------------------------------ the taps
class taps:
    """Context manager: per attention call of ``model`` -> ``self.calls[name]`` = dict(ref, query, off, shapes and, after a
    backward, g_off), all detached"""

    def __init__(self, model):
        self.model, self.calls, self._hooks = model, {}, []

    def __enter__(self):
        for name, att in attentions(self.model):
            rec = self.calls.setdefault(name, {})

            def pre(mod, args, rec=rec):
                rec["ref"], rec["shapes"] = args[1].detach(), args[3].tolist()

            def lin(mod, args, out, rec=rec):
                rec["query"], rec["off"] = args[0].detach(), out.detach()
                if out.requires_grad:
                    out.register_hook(lambda g, rec=rec: rec.__setitem__("g_off", g.detach()))
            self._hooks += [att.register_forward_pre_hook(pre), att.sampling_offsets.register_forward_hook(lin)]
        return self

    def __exit__(self, *exc):
        for h in self._hooks:
            h.remove()


RELU_LINEARS = tuple(f"fc_reg.{i}.layers.{j}" for i in range(2) for j in range(2))     # the box heads' Linears in front of a ReLU
FEW_ELEMENTS = ("fc_enc_reg",)              # a Linear whose bias.grad has 4 elements: tapped like the above, judged without exclusion


class relu_taps:
    """Context manager: per call of each of RELU_LINEARS -> ``self.calls[name]`` = [dict(x, z and, after a backward, g)]: the
    Linear's input, its output (the ReLU's argument) and the gradient of that output, detached"""

    def __init__(self, model):
        self.model, self.calls, self._hooks = model, {name: [] for name in RELU_LINEARS + FEW_ELEMENTS}, []

    def __enter__(self):
        for name in RELU_LINEARS + FEW_ELEMENTS:
            def hook(mod, args, out, calls=self.calls[name]):
                rec = dict(x=args[0].detach(), z=out.detach())
                if out.requires_grad:
                    out.register_hook(lambda g, rec=rec: rec.__setitem__("g", g.detach()))
                calls.append(rec)
            self._hooks.append(self.model.get_submodule(name).register_forward_hook(hook))
        return self

    def __exit__(self, *exc):
        for h in self._hooks:
            h.remove()


def pixel_locations(rec):
    """the samples of a tapped call in pixels of their level, float64: (N, Lq, M, L, P, 2) [x, y]"""
    ref, off = rec["ref"].double(), rec["off"].double()
    shapes = torch.tensor(rec["shapes"], device=ref.device)
    loc = MT.locations_of(ref, off.view(off.shape[0], off.shape[1], HEADS, LEVELS, POINTS, 2), shapes, POINTS)
    extent = torch.stack([shapes[:, 1], shapes[:, 0]], -1).double()
    return loc * extent[None, None, None, :, None, :] - 0.5


def line_distance(px):
    """distance of each sample to the nearest pixel-centre line, the smaller of x and y: (N, Lq, M, L, P)"""
    return (px - px.round()).abs().min(-1)[0]


def lattice_margin(f64_taps):
    """the smallest line distance of the encoder samples"""
    return min(float(line_distance(pixel_locations(rec)).min()) for name, rec in f64_taps.items() if name.startswith("enc"))


def location_error(side_rec, f64_rec):
    """E per level: max |side px - f64 px| + 4 fp32 ulps of the level extent -> (L,) float64"""
    d = (pixel_locations(side_rec) - pixel_locations(f64_rec)).abs().amax((0, 1, 2, 4, 5))
    ulp = torch.tensor([float(np.spacing(np.float32(max(hw)))) for hw in f64_rec["shapes"]], dtype=torch.float64, device=d.device)
    return d + 4 * ulp


def kept_samples(f64_rec, E):
    """the samples further than 2 E px from every line in the float64 chain: (N, Lq, M, L, P) bool"""
    return line_distance(pixel_locations(f64_rec)) > 2 * E[None, None, None, :, None]


# ------------------------------------------------------------------------------------------------------------------ the drivers
def _select_given(idx, coord, anchors, memory):
    """query_select_torch_restated.select with the tokens given"""
    four = idx.unsqueeze(-1).repeat(1, 1, 4)
    boxes = torch.gather(coord, 1, four)
    return idx, boxes, torch.gather(anchors, 1, four).sigmoid(), \
        torch.gather(memory, 1, idx.unsqueeze(-1).repeat(1, 1, memory.shape[2])), boxes.sigmoid()


def _decoder_mutant(dec, mutant, tgt, memory, dn, pad, refpoints_unsigmoid, starts, shapes, vr, fc_reg):
    """``RP.Decoder.forward`` with a handoff between the layers broken"""
    output, intermediate = tgt, []
    reference_points = refpoints_unsigmoid.sigmoid()
    ref_points = [reference_points]
    first_input = None
    for layer_id, layer in enumerate(dec.layers):
        ref_input, embed = RP.reference_inputs(reference_points, vr)
        if first_input is None:
            first_input = ref_input
        if mutant == "stale_ref_input":
            ref_input = first_input
        output = layer(tgt=output, tgt_query_pos=dec.ref_point_head(embed), tgt_query_sine_embed=embed,
                       tgt_reference_points=ref_input, memory=memory, memory_key_padding_mask=pad, memory_level_start_index=starts,
                       memory_spatial_shapes=shapes, self_attn_mask=dn)
        new = (fc_reg[layer_id](output) + RP.inverse_sigmoid(reference_points)).sigmoid()
        reference_points = new if mutant == "reference_not_detached" else new.detach()
        ref_points.append(new)
        intermediate.append(dec.norm(output))
    return [[t.transpose(0, 1) for t in intermediate], [t.transpose(0, 1) for t in ref_points]]


def stock_forward(m, feats, pos, pad, vr, dn, idx=None, mutant=None):
    """Every module's own forward.  ``idx``: the selected tokens are given.  -> dict of the boundary tensors"""
    assert mutant is None or mutant in MUTANTS, mutant
    tokens, q, shapes, starts = T.project(m.input_proj, feats, LEVELS, pos)
    if mutant == "level_start_shifted":
        starts = torch.cat([starts[:1], starts[:-1]])
    if mutant in ("no_valid_ratio", "encoder_mask_dropped_layer1", "layer0_without_pos"):
        ref = (_unscaled_reference_points if mutant == "no_valid_ratio" else get_reference_points)(shapes, vr, tokens.device)
        memory = tokens
        for i, layer in enumerate(m.enc.layers):
            memory = layer(memory, None if mutant == "layer0_without_pos" and i == 0 else pos, ref, shapes, starts,
                           None if mutant == "encoder_mask_dropped_layer1" and i == 1 else pad)
    else:
        memory = m.enc(tokens, pos, shapes, starts, vr, pad)[0]
    om, prop = QT.gen_proposals(memory, pad, shapes.tolist())
    om = m.owner.enc_output_norm(m.owner.enc_output(om))
    logits = m.fc_enc_cls(om)
    coord = m.fc_enc_reg(om) + prop
    sel = QT.select(logits, coord, prop, om, K) if idx is None else _select_given(idx, coord, prop, om)
    _, undetached, _, hs_enc, ref_enc = sel
    tgt = m.owner.tgt_embed.weight[:K, None, :].repeat(1, tokens.shape[0], 1)                       # (K, N, 256)
    dec_pad = None if mutant == "decoder_memory_mask_dropped" else pad
    if mutant in ("stale_ref_input", "reference_not_detached"):
        hs, reference = _decoder_mutant(m.dec, mutant, tgt, memory.transpose(0, 1), dn, dec_pad, undetached.detach().transpose(0, 1),
                                        starts, shapes, vr, m.fc_reg)
    else:
        hs, reference = m.dec(tgt, memory.transpose(0, 1), tgt_mask=dn, memory_key_padding_mask=dec_pad,
                              refpoints_unsigmoid=undetached.detach().transpose(0, 1), level_start_index=starts,
                              spatial_shapes=shapes, valid_ratios=vr, fc_reg=m.fc_reg)
    boxes = RP.box_outputs(m.fc_reg, hs, reference)
    return dict(tokens=tokens, q=q, memory=memory, output_memory=om, logits=logits, idx=sel[0], hs=hs, reference=reference,
                boxes=boxes, hs_enc=hs_enc, ref_enc=ref_enc)


def hip_forward(m, feats, pos, pad, vr, dn):
    """The mirrors, in the order the product calls them"""
    from semi_detr_amd import add_norm, input_proj, query_select as Q, ref_points
    rec = {}
    hooks = [m.owner.enc_output_norm.register_forward_hook(lambda mod, i, o: rec.__setitem__("output_memory", o)),
             m.fc_enc_cls.register_forward_hook(lambda mod, i, o: rec.__setitem__("logits", o))]
    inner = Q.select_queries

    def recorder(*a):
        rec["select"] = inner(*a)
        return rec["select"]
    Q.select_queries = recorder
    try:
        tokens, q, shapes, starts, _ = input_proj.project_pyramid(m.input_proj, feats, LEVELS, pos)
        memory = add_norm.encoder_forward(m.enc, tokens, pos, shapes, starts, vr, pad, query=q)[0]
        refpoint, tgt, hs_enc, ref_enc, _ = Q.two_stage_queries(m.owner, memory, pad, shapes, m.fc_enc_cls, m.fc_enc_reg, None, None)
        hs, reference = ref_points.decoder_forward(m.dec, tgt.transpose(0, 1), memory.transpose(0, 1), tgt_mask=dn,
                                                   memory_key_padding_mask=pad, refpoints_unsigmoid=refpoint.transpose(0, 1),
                                                   level_start_index=starts, spatial_shapes=shapes, valid_ratios=vr, fc_reg=m.fc_reg)
        boxes = ref_points.box_outputs(m.fc_reg, hs, reference)
    finally:
        Q.select_queries = inner
        for h in hooks:
            h.remove()
    return dict(tokens=tokens, q=q, memory=memory, output_memory=rec["output_memory"], logits=rec["logits"], idx=rec["select"][0],
                hs=hs, reference=reference, boxes=boxes, hs_enc=hs_enc[0], ref_enc=ref_enc[0])


def forward_tensors(r):
    """[(name, tensor)] of what is judged forward"""
    named = [(n, r[n]) for n in ("tokens", "q", "memory", "output_memory", "logits")]
    named += [(f"intermediate[{i}]", t) for i, t in enumerate(r["hs"])] + [(f"reference[{i}]", t) for i, t in enumerate(r["reference"])]
    return named + [("boxes", r["boxes"]), ("hs_enc", r["hs_enc"]), ("ref_enc", r["ref_enc"])]


def run_side(model, forward, inp, context="fp32_fused", device="cpu", exact=False, **kw):
    """Forward under the context, backward from the fixed seeds -> dict(fwd [(name, tensor)], grads [(name, tensor or None)],
    idx, taps {attention: dict}, params {name: the parameter's data} )"""
    cast = (lambda t: t.double()) if exact else (lambda t: t)
    feats = [cast(t.to(device)).clone().requires_grad_(True) for t in inp["feats"]]
    pos = cast(inp["pos"].to(device)).clone().requires_grad_(True)
    pad, vr, dn = inp["pad"].to(device), cast(inp["vr"].to(device)), inp["dn"].to(device)
    with taps(model) as tp, relu_taps(model) as rt:
        with autocast("fp32" if exact else context, device):
            r = forward(model, feats, pos, pad, vr, dn, **kw)
        outs = list(r["hs"]) + [r["boxes"], r["hs_enc"], r["ref_enc"]]
        names = [n for n, _ in model.named_parameters()]
        grads = torch.autograd.grad(outs, feats + [pos] + list(model.parameters()),
                                    [cast(s.to(device)).to(o.dtype) for s, o in zip(inp["seeds"], outs)], allow_unused=True)
    what = [f"grad feats[{i}]" for i in range(len(feats))] + ["grad pos"] + ["grad " + n for n in names]
    return dict(fwd=[(n, t.detach()) for n, t in forward_tensors(r)], grads=list(zip(what, grads)), idx=r["idx"], taps=tp.calls, relu=rt.calls,
                params=dict(zip(names, grads[len(feats) + 1:])))


# ------------------------------------------------------------------------------------------------------------------ the judges
def _err(a, b):
    return float((a.double() - b.double()).abs().max()) if a.numel() else 0.0


def reduction_floor(g, x=None):
    """One unit roundoff of the gradient's dtype times the largest sum of absolute terms of ``g.sum(0)`` (or of ``g.t() @ x``).
    A sum of n terms in any order is off by up to (n - 1) u sum |term|, so u sum |term| is an error no correct reduction can be
    held below.  It is the floor of the scale in the "| own gradient" rows: there both sides' errors are roundings of the
    SAME torch reduction on nearly equal operands (a few ulps each), and the larger of two such draws over a few hundred
    elements was seen at 4.7 times the smaller; a gradient that is wired wrongly is off by its own size."""
    g2 = g.double().abs().reshape(-1, g.shape[-1])
    terms = g2.sum(0) if x is None else g2.t() @ x.double().abs().reshape(-1, x.shape[-1])
    return float(torch.finfo(g.dtype).eps) * float(terms.max())


def rule_report(side, stock, f64_side, f64_stock, which="fwd", skip=()):
    """[(name, |side - f64|, |stock - f64|)] per tensor of ``which`` ('fwd' or 'grads'); asserts the ``None`` pattern and dtypes
    equal stock's.  ``skip``: names left to another judge."""
    rows = []
    for (n, h), (n2, r), (_, dh), (_, ds) in zip(side[which], stock[which], f64_side[which], f64_stock[which]):
        assert n == n2
        assert (h is None) == (r is None), f"{n}: side {None if h is None else h.dtype}, stock {None if r is None else r.dtype}"
        if r is None:
            assert dh is None and ds is None, n
            continue
        assert h.dtype == r.dtype and h.shape == r.shape, f"{n}: side {h.dtype} {tuple(h.shape)}, stock {r.dtype} {tuple(r.shape)}"
        assert torch.isfinite(h).all(), n
        if n not in skip:
            rows.append((n, _err(h, dh), _err(r, ds)))
    return rows


def broken(rows, factor):
    """the names of the tensors that break the rule"""
    return [n for n, err, scale in rows if not err <= factor * scale]


def offset_gradient_names(model, calls=""):
    return ["grad " + name + ".sampling_offsets." + p for name, _ in attentions(model) if name.startswith(calls)
            for p in ("weight", "bias")]


def same_cell(side_rec, f64_rec):
    """the samples a side puts into the bilinear cell the float64 chain puts them into: (N, Lq, M, L, P) bool"""
    return (pixel_locations(side_rec).floor() == pixel_locations(f64_rec).floor()).all(-1)


def kink_report(model, side, stock, f64_side, f64_stock, mode="margin", calls=""):
    """The ``init``-state judgement of d out / d offsets at the op boundary, per attention call whose name starts with ``calls``
    -> (rows, shares, left): rows as rule_report's, for the gradient of the Linear's output on the kept samples and for the two
    parameter gradients against the float64 Linear backward of the side's own hooked gradient; shares {call: (left out on the
    side, on stock)}; left {call: (E in px, worst error among the samples left out on the side, on stock)}.

    ``mode`` says which samples are left out.  'margin' (fp32): those within 2 E px of a line in the float64 chain.  'cell'
    (autocast, where the sides' reference boxes differ by 16-bit roundings upstream and E is a tenth of a pixel): those the
    side puts into another bilinear cell than its float64 chain does -- the samples that did cross a line."""
    assert mode in ("margin", "cell")
    rows, shares, worst_left = [], {}, {}
    for name, _ in attentions(model):
        if not name.startswith(calls):
            continue
        E = torch.maximum(location_error(side["taps"][name], f64_side["taps"][name]),
                          location_error(stock["taps"][name], f64_stock["taps"][name]))
        errs, left, flipped = [], [], [float(E.max())]
        for s, f in ((side, f64_side), (stock, f64_stock)):
            keep = kept_samples(f["taps"][name], E) if mode == "margin" else same_cell(s["taps"][name], f["taps"][name])
            left.append(1.0 - float(keep.double().mean()))
            g, g64 = s["taps"][name]["g_off"].double(), f["taps"][name]["g_off"]
            d = (g - g64).abs().view(keep.shape + (2,))
            errs.append(float((d * keep[..., None]).max()))
            flipped.append(float((d * ~keep[..., None]).max()))
        rows.append((f"{name}: grad offsets, kept samples", errs[0], errs[1]))
        shares[name], worst_left[name] = tuple(left), tuple(flipped)
        lin = [[], []]
        for k, s in enumerate((side, stock)):
            g = s["taps"][name]["g_off"].double().flatten(0, 1)
            x = s["taps"][name]["query"].double().flatten(0, 1)
            lin[k] = [_err(s["params"][name + ".sampling_offsets.weight"], g.t() @ x),
                      _err(s["params"][name + ".sampling_offsets.bias"], g.sum(0))]
        rec = side["taps"][name]
        rows.append((f"{name}: sampling_offsets.weight.grad | own gradient", lin[0][0],
                     max(lin[1][0], reduction_floor(rec["g_off"], rec["query"]))))
        rows.append((f"{name}: sampling_offsets.bias.grad | own gradient", lin[0][1], max(lin[1][1], reduction_floor(rec["g_off"]))))
    return rows, shares, worst_left


def relu_gradient_names():
    return ["grad " + name + "." + p for name in RELU_LINEARS for p in ("weight", "bias")]


def few_elements_report(side, stock, f64_side, f64_stock):
    """``fc_enc_reg.bias.grad`` at the op boundary.  It has 4 elements, each the sum of the 2 K selected rows of the gradient of
    ``enc_outputs_coord``: in fp32 both sides are within a few ulps of the float64 value and ``max |stock - f64|`` over 4
    numbers is anything between 0 and those few ulps, so the whole-tensor ratio says nothing (4.06 seen beside 1.1).  Judged
    instead: the gradient of the Linear's output, (N, S, 4), by the rule, and bias.grad against the float64 sum of the side's
    own hooked gradient -> rows as rule_report's."""
    rows = []
    for name in FEW_ELEMENTS:
        errs, lin = [], []
        for s, f in ((side, f64_side), (stock, f64_stock)):
            (rec,), (rec64,) = s["relu"][name], f["relu"][name]
            errs.append(_err(rec["g"], rec64["g"]))
            lin.append(_err(s["params"][name + ".bias"], rec["g"].double().reshape(-1, rec["g"].shape[-1]).sum(0)))
        rows.append((f"{name}: grad of the Linear's output", errs[0], errs[1]))
        rows.append((f"{name}: bias.grad | own gradient", lin[0], max(lin[1], reduction_floor(side["relu"][name][0]["g"]))))
    return rows


def relu_report(side, stock, f64_side, f64_stock):
    """The box heads' Linears in front of a ReLU at the op boundary (the ReLU's derivative jumps at 0 as the bilinear one does at
    a pixel-centre line: a unit whose argument a side puts on the other side of 0 than the float64 chain does is an error of
    the size of that unit's gradient) -> (rows, shares): rows as rule_report's, per Linear for the gradient of its output on
    the units that keep the float64 chain's sign, and for weight.grad / bias.grad against the float64 Linear backward of the
    side's own hooked gradients, summed over its calls; shares {Linear: (share of the units across 0 on the side, on stock)}."""
    rows, shares = [], {}
    for name in RELU_LINEARS:
        kept, crossed, lin = [], [], []
        for s, f in ((side, f64_side), (stock, f64_stock)):
            err, flips, units, gw, gb, fw, fb = 0.0, 0, 0, 0, 0, 0.0, 0.0
            for rec, rec64 in zip(s["relu"][name], f["relu"][name]):
                if "g" not in rec64:                   # a call nothing is differentiated through (the last layer's refinement)
                    assert "g" not in rec
                    continue
                flip = (rec["z"].double() > 0) != (rec64["z"] > 0)
                d = (rec["g"].double() - rec64["g"]).abs()
                err, flips, units = max(err, float((d * ~flip).max())), flips + int(flip.sum()), units + flip.numel()
                g, x = rec["g"].double().reshape(-1, rec["g"].shape[-1]), rec["x"].double().reshape(-1, rec["x"].shape[-1])
                gw, gb = gw + g.t() @ x, gb + g.sum(0)
                fw, fb = fw + reduction_floor(rec["g"], rec["x"]), fb + reduction_floor(rec["g"])
            kept.append(err)
            crossed.append(flips / units)
            lin.append((_err(s["params"][name + ".weight"], gw), _err(s["params"][name + ".bias"], gb), fw, fb))
        rows.append((f"{name}: grad of the ReLU's argument, units that keep their sign", kept[0], kept[1]))
        rows.append((f"{name}: weight.grad | own gradient", lin[0][0], max(lin[1][0], lin[0][2])))
        rows.append((f"{name}: bias.grad | own gradient", lin[0][1], max(lin[1][1], lin[0][3])))
        shares[name] = tuple(crossed)
    return rows, shares


def left_out_shares(side, f64_side):
    """{call: share of the samples within 2 E px of a line}, E from this side alone (the CPU condition on the committed seeds)"""
    return {name: 1.0 - float(kept_samples(f64_side["taps"][name], location_error(rec, f64_side["taps"][name])).double().mean())
            for name, rec in side["taps"].items()}


def topk_gap(logits):
    """the smallest difference between consecutive keys among the first K + 1 (key = max over the classes), per image"""
    keys = logits.double().max(-1)[0].sort(1, descending=True)[0][:, :K + 1]
    return float((keys[:, :-1] - keys[:, 1:]).min())


def in_float64(model):
    return copy.deepcopy(model).double()
