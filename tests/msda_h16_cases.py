"""Cases of the mixed-precision MSDA op, shared by tests/test_msda_h16_ref.py (CPU) and tests/test_gpu_msda_h16.py (GPU).

Inputs come from test_gpu_msda_bounds.make_case (value signed and spread over five decades per head, grad_out ~ N(0, 1),
attention a softmax of N(0, 2) logits), with mask = None and no level_range (10^2 on a level times 10^2 on a head would leave
fp16's range); value and grad_out are rounded to the 16-bit type first (torch, CPU), locations and weights stay fp32.

The smallest shapes at which the kernels can still go wrong: every forward split and both backward row counts of the D = 32
kernels, a workgroup tail, an odd head count, L * P = 20, one-pixel-wide levels, rows without a single sample on the map, and the
generic kernels for D != 32, > 32 heads and a value pointer off the 8-byte grid.
"""
import functools

import numpy as np

import msda_h16_ref as H
from test_gpu_msda_bounds import DINO, PYR4, PYR5, _spec, make_case

DTYPES = ("fp16", "bf16")
FWD1, FWD2, FWD4, FWD_GENERIC = "msda_fwd_h16<1", "msda_fwd_h16<2", "msda_fwd_h16<4", "msda_fwd_h16_generic"
BWD, BWD_GENERIC = "msda_bwd_h16+msda_h16_convert", "msda_bwd_h16_generic+msda_h16_convert"
THIN = [(1, 5), (4, 1)]

CASES = {
    # decoder, D = 32: 8 query rows per backward workgroup, forward split 4
    "dec_offmap": _spec(DINO, 2, Lq=100, spread="offmap", fwd=FWD4, bwd=BWD, seed=101),
    "dec_anywhere": _spec(DINO, 4, Lq=300, spread="anywhere", fwd=FWD4, bwd=BWD, seed=102),
    "dec_tail_m3": _spec(DINO, 1, Lq=33, M=3, spread="offmap", fwd=FWD4, bwd=BWD, seed=103),      # workgroup tail, odd head count
    # encoder, D = 32, Lq = S: split 2 and 32 rows per backward workgroup at two images, split 1 at four
    "enc_pyr4": _spec(PYR4, 2, spread=2.0, fwd=FWD2, bwd=BWD, seed=104),
    "enc_pyr5": _spec(PYR5, 2, spread=2.0, fwd=FWD2, bwd=BWD, seed=105),                            # L * P = 20
    "enc_pyr4_bs4": _spec(PYR4, 4, spread=2.0, fwd=FWD1, bwd=BWD, seed=106, backward=False),
    # degenerate
    "thin_levels": _spec(THIN, 2, Lq=40, spread="offmap", fwd=FWD4, bwd=BWD, seed=107),
    "all_offmap": _spec(DINO, 2, Lq=70, spread="anywhere", fwd=FWD4, bwd=BWD, seed=108),           # locations moved to [1.5, 2]: below
    # generic kernels
    "generic_d16": _spec(DINO, 2, Lq=50, D=16, spread="offmap", fwd=FWD_GENERIC, bwd=BWD_GENERIC, seed=109),
    "generic_d64": _spec(DINO, 2, Lq=50, D=64, spread="anywhere", fwd=FWD_GENERIC, bwd=BWD_GENERIC, seed=110),
    "generic_d30": _spec(DINO, 2, Lq=50, D=30, spread="offmap", fwd=FWD_GENERIC, bwd=BWD_GENERIC, seed=111),
    "generic_m33": _spec(DINO, 1, Lq=40, M=33, spread="offmap", fwd=FWD_GENERIC, bwd=BWD_GENERIC, seed=112),
    "generic_unaligned": _spec(DINO, 2, Lq=70, unaligned=True, spread=3.0, fwd=FWD_GENERIC, bwd=BWD_GENERIC, seed=113),
}
ALL_OFFMAP = "all_offmap"


@functools.lru_cache(maxsize=None)
def inputs(name, dtype):
    """dict(shapes, value, gout: float32 arrays of exact 16-bit values; loc, attn: float32) of a case.  Cached, never modified."""
    c = make_case(CASES[name])
    loc = c["loc"]
    if name == ALL_OFFMAP:
        loc = (1.5 + 0.5 * loc).astype(np.float32)
    out = dict(shapes=c["shapes"], value=H.round16(c["value"], dtype), gout=H.round16(c["gout"], dtype), loc=loc, attn=c["attn"])
    for a in out.values():
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def reference(name, dtype):
    """The fp64 reference with the 16-bit bounds of a case (msda_h16_ref.reference).  Cached, shared by the tests that need it."""
    c = inputs(name, dtype)
    return H.reference(c["value"], c["shapes"], c["loc"], c["attn"], c["gout"] if CASES[name]["backward"] else None, dtype)
