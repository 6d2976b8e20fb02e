"""Cases of the fused prologue / epilogue on a 16-bit value map, shared by tests/test_msda_h16_fused_ref.py (CPU) and
tests/test_gpu_msda_h16_fused.py (GPU).

Inputs come from test_gpu_msda_bounds.make_case with io="fused" (value signed and spread over five decades per head, grad_out ~
N(0, 1), logits ~ N(0, 2), padded pixels of value hold NaN: a kernel that loads a masked corner fails).  value and grad_out are
rounded to the 16-bit type first (torch, CPU) and so are offsets and logits when the prologue type is 16-bit; reference points stay
fp32.

The smallest shapes that reach every kernel instance: the three forward splits, both backward row counts, a workgroup tail, an odd
head count, rows with no sample on the map, 2-d points and 4-d boxes, L * P = 16 (softmax by lane shuffles) and 20 (softmax rows
in LDS), a band mask and a mask that is no band.
"""
import functools

import numpy as np

import msda_h16_fused_ref as F
import msda_h16_ref as H
from test_gpu_msda_bounds import DINO, PYR4, PYR5, _spec, make_case

FWD1, FWD2, FWD4 = "msda_fwd_h16_fused<1", "msda_fwd_h16_fused<2", "msda_fwd_h16_fused<4"
BWD = "msda_bwd_h16_fused+msda_h16_convert"

CASES = {
    # SPLIT 4, workgroup tail, 8-row backward, boxes
    "dec_boxes": _spec(DINO, 2, Lq=33, io="fused", ref_dim=4, spread=1.5, fwd=FWD4, bwd=BWD, seed=201),
    # odd head count, rows with no sample on the map
    "dec_points_m3": _spec(DINO, 1, Lq=33, M=3, io="fused", spread="offmap", fwd=FWD4, bwd=BWD, seed=202),
    # SPLIT 2, 32-row backward, band mask
    "enc_pyr4_band": _spec(PYR4, 2, io="fused", mask="band", spread=2.0, fwd=FWD2, bwd=BWD, seed=203),
    # L * P = 20, a mask that is no band
    "enc_pyr5_random": _spec(PYR5, 2, io="fused", mask="random", spread=6.0, fwd=FWD2, bwd=BWD, seed=204),
    # SPLIT 1 (forward only)
    "enc_pyr4_bs4": _spec(PYR4, 4, io="fused", mask="random", spread=2.0, fwd=FWD1, bwd=BWD, seed=205, backward=False),
}
UNMASKED = "dec_boxes"
# (dtype, prologue type): every case for fp16 and bf16 with 16-bit offsets / logits; bf16 also with fp32 ones
COMBOS = (("fp16", "h16"), ("bf16", "h16"), ("bf16", "f32"))


@functools.lru_cache(maxsize=None)
def inputs(name, dtype, prologue_type):
    """dict(shapes, mask, value, gout, ref, off, logits: float32 arrays; 16-bit operands hold exact 16-bit values) of a case.
    Cached, never modified."""
    c = make_case(CASES[name])
    h16 = prologue_type == "h16"
    out = dict(shapes=c["shapes"], mask=c["mask"], value=H.round16(c["value"], dtype), gout=H.round16(c["gout"], dtype), ref=c["ref"],
               off=H.round16(c["off"], dtype) if h16 else c["off"], logits=H.round16(c["logits"], dtype) if h16 else c["logits"])
    for a in out.values():
        if a is not None:
            a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def reference(name, dtype, prologue_type):
    """The fp64 reference with the bounds of a case (msda_h16_fused_ref.reference).  Cached, shared by the tests that need it."""
    c = inputs(name, dtype, prologue_type)
    return F.reference(c["value"], c["shapes"], c["ref"], c["off"], c["logits"], c["gout"] if CASES[name]["backward"] else None,
                       c["mask"], dtype, prologue_type)
