"""GPU: the detector chain with the real ``semi_detr_amd.MSDeformAttn`` in every layer, driven through the mirrors in the order
the product calls them (tests/detector_chain_cases.py; the judges are checked on the CPU by tests/test_detector_chain_ref.py).

    project_pyramid -> encoder_forward(query=) -> two_stage_queries -> ref_points.decoder_forward(fc_reg=) -> box_outputs

against stock torch running the restated modules in the same context, both against the float64 chain handed the side's own
selected tokens: per tensor ``max |hip - f64| <= FACTOR * max |stock - f64|`` (FACTOR of tests/test_gpu_add_norm.py).  Dtypes and
the ``None`` pattern of every boundary and gradient are stock torch's.

What the stand-in chains cannot see and this one does: the encoder's valid-ratio reference points and the padding mask inside the
fused kernels of every layer, ``q = tokens + pos`` handed from ``project_pyramid`` to layer 0, ``memory_key_padding_mask`` in the
decoder, the transposed ``ref_input`` of the reference-point op renewed and detached between the decoder layers, and the MSDA
routes (fused prologue, up-cast, 16-bit, fused 16-bit) beside the mixed add_norm and the 16-bit self-attention under autocast.

Gradients: ``init`` state in fp32 -- every gradient by the rule, the attentions' ``sampling_offsets`` gradients by
``kink_report`` (samples within 2 E px of a pixel-centre line left out, at most 1 % per call); ``trained`` -- dtype, ``None``
pattern and finiteness (a sample that crosses a line on one side only reaches the query through the offsets); the ratios of the
rule are printed there, not asserted.

``init`` under autocast -- every gradient by the rule as it stands, but for the ``sampling_offsets`` gradients of the two decoder
cross-attentions, which go to the op boundary.  The encoder's locations are the same numbers on both sides (constant reference
points, offsets = the exact bias), so both sides cross the same lines and the whole-tensor rule holds.  The decoder's reference
boxes come through 16-bit GEMMs (``fc_enc_reg``, ``fc_reg``) and differ from the float64 chain's by hundredths of a pixel, each
side puts OTHER samples across a line, one such sample is an error of the size of the gradient itself, and the maximum over a
tensor is whichever side drew the larger one (figures: profiles/detector_chain_probe.txt).  So for these four tensors the
gradient of the Linear's output is judged by the rule on the samples the side keeps in the float64 chain's bilinear cell, the
share left out may not exceed min(4 E, CROSSING_CAP) on either side, and the two parameter gradients are judged against the
float64 Linear backward of the side's own hooked gradient.  The whole-tensor ratios are printed, not asserted.

The same under autocast for the box heads' Linears in front of a ReLU (``fc_reg.*.layers.0 / .1``): the ReLU's derivative jumps
at 0, the 16-bit GEMM in front of it moves its argument by 1e-3, and a unit that one side puts across 0 is an error of the size
of that unit's gradient (``fc_reg.0.layers.0.bias.grad``, patch pyramid, fp16: hip 3 such units of 10240, stock 2, error 7.5e-3
on them against 7.5e-4 on every other unit of BOTH sides; whole-tensor ratio 4.64).  ``relu_report`` judges the gradient of
the ReLU's argument on the units that keep the float64 chain's sign, the share of the others against 1 %, and weight.grad /
bias.grad against the float64 Linear backward of the side's own hooked gradients.

In every ``init`` cell ``fc_enc_reg.bias.grad`` (4 elements) is judged by ``few_elements_report``: the gradient of the Linear's
output by the rule, the bias gradient against the float64 sum of the side's own hooked gradient.

Wherever a parameter gradient is judged against the float64 Linear backward of the side's own hooked gradient, both errors
are roundings of one torch reduction; the scale of those rows has the floor ``detector_chain_cases.reduction_floor``.

One yardstick for both sides.  ``max |stock - f64|`` is the scale of the rule, so it has to be the error of the SAME problem
computed with the SAME torch kernels as the hip side's:
  * torch's convolutions pick their algorithm per call unless told otherwise, and the algorithms differ in accuracy (fp16
    gradients of one stock side moved by 13 % between two calls): every side here runs with
    ``torch.backends.cudnn.deterministic = True`` and ``benchmark = False`` (``_pinned_algorithms``), which makes a side's
    forward repeat bit for bit.
  * 16-bit logits tie or nearly tie, so the two sides may return the selected tokens in another ORDER; the queries are
    positional (``tgt_embed``, the de-noising mask), so that is another problem with another error.  Each side's selection is
    judged exactly on its own logits; where the two lists differ the stock side is run again handed hip's tokens, and that run
    is the scale (the float64 chain is handed the same tokens).

Run with -s for the worst ratio of every tensor.
"""
import functools

import numpy as np
import pytest
import torch

import detector_chain_cases as C
import msda_h16_cases as C16
import msda_h16_fused_cases as F16
import query_select_ref64 as QR
import test_gpu_msda_bounds as B
from test_gpu_add_norm import FACTOR
from test_gpu_lib_call import Recorder

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
MATRIX = [(p, s, c) for p in C.PYRAMIDS for s in C.STATES for c in C.CONTEXTS]
MSDA_CALLS = ("ms_deform_attn_forward", "ms_deform_attn_backward", "ms_deform_attn_fused_forward", "ms_deform_attn_fused_backward",
              "ms_deform_attn_h16_forward", "ms_deform_attn_h16_backward", "ms_deform_attn_h16_fused_forward",
              "ms_deform_attn_h16_fused_backward")
CROSSING_CAP = 0.05            # of a call's samples in another cell than the float64 chain's: near three times the largest share seen (1.8 %)
STRIPS = (B.FWD_STRIP1, B.FWD_STRIP2, B.FWD_STRIP4)
ROW_BACKWARDS = (B.BWD_D32_8, B.BWD_D32_32, B.BWD_MERGED)
# what must have run inside the chain somewhere in the matrix: name -> (python entry of the op, kernels it may report)
ROUTES = {
    "fused masked patch forward": ("ms_deform_attn_fused_forward", (B.FWD_PATCH,)),
    "fused masked patch backward": ("ms_deform_attn_fused_backward", (B.BWD_PATCH,)),
    "fused masked window forward": ("ms_deform_attn_fused_forward", (B.FWD_WINDOW,)),
    "fused masked window backward": ("ms_deform_attn_fused_backward", (B.BWD_WINDOW,)),
    "fused decoder strip, boxes": ("ms_deform_attn_fused_forward", STRIPS),
    "fused decoder strip backward": ("ms_deform_attn_fused_backward", ROW_BACKWARDS),
    "16-bit forward": ("ms_deform_attn_h16_forward", (C16.FWD1, C16.FWD2, C16.FWD4)),
    "16-bit backward": ("ms_deform_attn_h16_backward", (C16.BWD,)),
    "fused 16-bit forward": ("ms_deform_attn_h16_fused_forward", (F16.FWD1, F16.FWD2, F16.FWD4)),
    "fused 16-bit backward": ("ms_deform_attn_h16_fused_backward", (F16.BWD,)),
}


class Names(Recorder):
    """tests/test_gpu_lib_call.py's recorder, keeping the name of every C-ABI call as well"""

    def __getattr__(self, name):
        fn = Recorder.__getattr__(self, name)

        def named(*args):
            self.__dict__.setdefault("names", []).append(name)
            return fn(*args)
        return named


class _Observed:
    """While active: every C-ABI call of the mirrors goes through ``Names``, and every MSDA op call leaves (python entry, the
    kernels it launched) in ``routes`` (read on the calling thread right after the call: the backward runs on autograd's)."""

    def __enter__(self):
        import MultiScaleDeformableAttention as MSDA
        import semi_detr_amd as s
        self._lib, self._msda = s._lib, MSDA
        self._handle = s._lib.lib()
        self.rec = Names(self._handle)
        self.routes, self._saved = [], {}
        for name in MSDA_CALLS:
            inner = self._saved[name] = getattr(MSDA, name)
            # (the 16-bit ops keep their own string: tests/test_gpu_msda_h16.py)
            last = self._handle.semidetr_msda_h16_last_kernels if "h16" in name else self._handle.semidetr_msda_last_kernels

            def spy(*a, _inner=inner, _name=name, _last=last):
                out = _inner(*a)
                self.routes.append((_name, _last().decode()))
                return out
            setattr(MSDA, name, spy)
        s._lib._lib = self.rec
        return self

    def __exit__(self, *exc):
        self._lib._lib = self._handle
        for name, inner in self._saved.items():
            setattr(self._msda, name, inner)


@pytest.fixture(autouse=True)
def _pinned_algorithms():
    """module docstring, "One yardstick for both sides" """
    saved = torch.backends.cudnn.deterministic, torch.backends.cudnn.benchmark
    torch.backends.cudnn.deterministic, torch.backends.cudnn.benchmark = True, False
    yield
    torch.backends.cudnn.deterministic, torch.backends.cudnn.benchmark = saved


@functools.lru_cache(maxsize=None)
def _problem(pyramid, state):
    model = C.build_model(state).to(DEV)
    return model, C.hip_model(model), C.in_float64(model), C.inputs(pyramid)


@functools.lru_cache(maxsize=None)
def _stock(pyramid, state, stock_context):
    """stock torch in the context: shared by the contexts that differ on the hip side only, never modified"""
    model, _, _, inp = _problem(pyramid, state)
    return C.run_side(model, C.stock_forward, inp, stock_context, DEV)


_f64_cache, _given_cache = {}, {}


def _stock_given(pyramid, state, stock_context, idx):
    """stock torch in the context handed the tokens ``idx`` (where the two sides' selections differ)"""
    key = (pyramid, state, stock_context, idx.cpu().numpy().tobytes())
    if key not in _given_cache:
        model, _, _, inp = _problem(pyramid, state)
        _given_cache[key] = C.run_side(model, C.stock_forward, inp, stock_context, DEV, idx=idx)
    return _given_cache[key]



def _f64(pyramid, state, idx):
    key = (pyramid, state, idx.cpu().numpy().tobytes())
    if key not in _f64_cache:
        _, _, model64, inp = _problem(pyramid, state)
        _f64_cache[key] = C.run_side(model64, C.stock_forward, inp, device=DEV, exact=True, idx=idx)
    return _f64_cache[key]


@functools.lru_cache(maxsize=None)
def _run(pyramid, state, context):
    """One cell of the matrix -> the figures; dtypes, the ``None`` pattern and finiteness are asserted here."""
    import semi_detr_amd as s
    model, hip, _, inp = _problem(pyramid, state)
    stock_context = {"fp32_fused": "fp32", "fp32_unfused": "fp32", "autocast_bf16_fused16": "autocast_bf16"}.get(context, context)
    stock = _stock(pyramid, state, stock_context)
    C.set_context(hip, context)
    s._lib.set_forward_policy(C.POLICY[pyramid])
    try:
        with _Observed() as seen:
            side = C.run_side(hip, C.hip_forward, inp, context, DEV)
            torch.cuda.synchronize()
    finally:
        s._lib.set_forward_policy("adaptive")
    # the selection, exactly, on the logits this side computed
    keys = QR.keys_of(dict(side["fwd"])["logits"].float().cpu().numpy())
    assert np.array_equal(side["idx"].cpu().numpy(), QR.topk(keys, C.K)), "not the first K of (key descending, token ascending)"
    # ... and stock's on its own: torch.topk's tokens are the first K by key (ties: any order)
    own = dict(stock["fwd"])["logits"].float().max(-1)[0]
    assert torch.equal(own.gather(1, stock["idx"]), own.sort(1, descending=True)[0][:, :C.K])
    same_tokens = torch.equal(side["idx"], stock["idx"])
    if not same_tokens:
        stock = _stock_given(pyramid, state, stock_context, side["idx"])
    f64_side = f64_stock = _f64(pyramid, state, side["idx"])
    rep = dict(fwd=C.rule_report(side, stock, f64_side, f64_stock, "fwd"), grads=[], kinks=[], shares={}, left={},
               routes=seen.routes, entries=set(seen.rec.__dict__.get("names", [])),
               same_tokens=same_tokens, whole=[], shown=[])
    # which sampling_offsets gradients go to the op boundary: all of them in fp32, the decoder's under autocast (module docstring)
    mode, calls = ("cell", "dec.") if C.is_autocast(context) else ("margin", "")
    judged_elsewhere = C.offset_gradient_names(model, calls) if state == "init" else ()
    if state == "init":
        judged_elsewhere = judged_elsewhere + ["grad " + n + ".bias" for n in C.FEW_ELEMENTS]      # C.few_elements_report
        if C.is_autocast(context):
            judged_elsewhere = judged_elsewhere + C.relu_gradient_names()
    grads = C.rule_report(side, stock, f64_side, f64_stock, "grads", skip=judged_elsewhere)
    if state == "init":
        rep["grads"], rep["mode"] = grads, mode
        rep["kinks"], rep["shares"], rep["left"] = C.kink_report(model, side, stock, f64_side, f64_stock, mode, calls)
        rep["kinks"] = rep["kinks"] + C.few_elements_report(side, stock, f64_side, f64_stock)
        if C.is_autocast(context):
            relu_rows, rep["relu_shares"] = C.relu_report(side, stock, f64_side, f64_stock)
            rep["kinks"] = rep["kinks"] + relu_rows
        rep["whole"] = [r for r in C.rule_report(side, stock, f64_side, f64_stock, "grads") if r[0] in judged_elsewhere]
    else:
        rep["shown"] = grads
    return rep


def _show(title, rows):
    worst = 0.0
    for n, err, scale in rows:
        ratio = err / scale if scale > 0 else (0.0 if err == 0 else float("inf"))
        worst = max(worst, ratio)
        print(f"  {title} {n:64s} |hip - f64| = {err:.3e}  |stock - f64| = {scale:.3e}  ratio {ratio:.2f}")
    return worst


@pytest.mark.parametrize("pyramid,state,context", MATRIX, ids=["/".join(c) for c in MATRIX])
def test_chain_against_stock_torch_and_float64(pyramid, state, context):
    rep = _run(pyramid, state, context)
    title = f"{pyramid}/{state}/{context}"
    print(f"\n{title}: same tokens on both sides: {rep['same_tokens']}; MSDA calls: " + "; ".join(f"{a} [{b}]" for a, b in rep["routes"]))
    worst = {k: _show(title, rep[k]) for k in ("fwd", "grads", "kinks")}
    whole = _show(title + " (not judged: the whole tensor, line crossings included)", rep["whole"])
    shown = _show(title + " (not judged: trained state)", rep["shown"])
    for name, (a, b) in rep["shares"].items():
        E, la, lb = rep["left"][name]
        print(f"  {title} {name}: E = {E:.2e} px; left out ({rep['mode']}) hip {a:.2e} / stock {b:.2e} of the samples; worst "
              f"|side - f64| among them hip {la:.3e} / stock {lb:.3e}")
    print(f"  {title}: worst |hip - f64| / |stock - f64|: forward {worst['fwd']:.2f}, gradients {worst['grads']:.2f}, "
          f"offset gradients at the op boundary {worst['kinks']:.2f} (whole tensors {whole:.2f}); trained-state gradients, not judged {shown:.2f}")
    for which in ("fwd", "grads", "kinks"):
        bad = C.broken(rep[which], FACTOR)
        assert not bad, [r for r in rep[which] if r[0] in bad]
    for name, (a, b) in rep.get("relu_shares", {}).items():
        print(f"  {title} {name}: ReLU arguments across 0 from the float64 chain's: hip {a:.2e} / stock {b:.2e} of the units")
        assert max(a, b) <= C.LEFT_OUT_CAP, (name, a, b)
    if rep.get("mode") == "margin":
        assert all(max(pair) <= C.LEFT_OUT_CAP for pair in rep["shares"].values()), rep["shares"]
    elif rep.get("mode") == "cell":
        # a sample can only change its cell from within E of a line: at most 2 E per coordinate of uniformly spread samples
        for name, pair in rep["shares"].items():
            assert max(pair) <= min(4.0 * rep["left"][name][0], CROSSING_CAP), (name, pair, rep["left"][name][0])
    # the mirrors ran their own entry points, forward and backward: a mirror that fell back to stock torch launches none
    norm = "mixed" if C.is_autocast(context) else "f32"
    want = ["semidetr_gn_tokens_forward", "semidetr_gn_tokens_backward", f"semidetr_add_norm_forward_{norm}",
            f"semidetr_add_norm_backward_{norm}", "semidetr_self_attn_forward", "semidetr_self_attn_backward",
            "semidetr_ref_points_forward", "semidetr_ref_points_backward", "semidetr_qsel_proposals_f32",
            "semidetr_qsel_proposals_backward_f32", "semidetr_qsel_topk_f32", "semidetr_qsel_gather_f32",
            "semidetr_qsel_gather_backward_f32"]
    missing = [w for w in want if not any(e.startswith(w) for e in rep["entries"])]
    assert not missing, (missing, sorted(rep["entries"]))
    # four attention modules, each called once forward and once backward
    assert len(rep["routes"]) == 8, rep["routes"]


def test_every_msda_route_ran_inside_the_chain():
    """over the whole matrix (cells already run are not run again)"""
    ran = [r for cell in MATRIX for r in _run(*cell)["routes"]]
    missing = [what for what, (entry, kernels) in ROUTES.items() if not any(e == entry and k in kernels for e, k in ran)]
    assert not missing, (missing, sorted(set(ran)))
