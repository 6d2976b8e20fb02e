"""The yardstick of the fused prologue / epilogue on a 16-bit value map (semidetr_msda_fused_forward_h16 / _backward_h16):
tests/msda_ref64.fused on the EXACTLY up-cast operands, its per-element fp32 bounds widened by the one rounding of each 16-bit
result (tests/msda_h16_ref.widen16: B32 + u16 (|ref| + B32) + s16).

Test helper (not a conftest); tests/test_msda_h16_fused_ref.py shows the bound admissible and sharp, tests/test_gpu_msda_h16_fused.py
judges the kernels by it.

Contract (include/semidetr_hip.h): value / grad_out are 16-bit numbers, offsets and logits are `prologue_type` numbers (fp32, or
value's 16-bit type), reference points are fp32; every 16-bit number is an fp32 number, so the fp32 fused op on the up-cast operands
is well defined and msda_ref64.fused's bounds (prologue delta / eps, epilogue) hold for the kernel's fp32 values before they are
stored.  `out` and `grad_value` are always rounded once; `grad_offsets` / `grad_logits` are rounded once when prologue_type is
16-bit and keep the plain fp32 bound when it is fp32.  No per-test factor; grad_offsets keeps the reference's kink set.
"""
import numpy as np

import msda_h16_ref as H
import msda_ref64 as R

PROLOGUE_TYPES = ("h16", "f32")      # the 16-bit type of `dtype`, or fp32


class Rounded(H.Bounded16):
    """msda_h16_ref.Bounded16 that keeps the fp32 result's skip set (grad_offsets: the kink set of the bilinear interpolant)."""

    def ratio(self, got):
        r = super().ratio(got)
        return r if self.skip is None else np.where(self.skip, 0.0, r)


def rounded_keys(prologue_type):
    return ("out", "grad_value") + (("grad_offsets", "grad_logits") if prologue_type == "h16" else ())


def reference(value16, shapes, ref, off, logits, gout16, mask, dtype, prologue_type):
    """value16 / gout16 (and off / logits for prologue_type 'h16'): float32 arrays holding 16-bit values exactly; ref: float32.
    -> dict of 'out' and, with gout16, 'grad_value', 'grad_offsets', 'grad_logits' (Rounded where the contract rounds,
    msda_ref64.Bounded otherwise) and 'prologue' (msda_ref64.prologue's dict)."""
    assert prologue_type in PROLOGUE_TYPES
    r = R.fused(np.asarray(value16, np.float64), shapes, ref, off, logits, None if gout16 is None else np.asarray(gout16, np.float64),
                mask=mask)
    keys = rounded_keys(prologue_type)
    return {k: (Rounded(v, dtype) if k in keys else v) for k, v in r.items()}


def check(route, what, got, ref):
    """Assert got within the bound elementwise (msda_h16_ref.check / msda_ref64.check); returns the worst err / bound."""
    return H.check(route, what, got, ref)
