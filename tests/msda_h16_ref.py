"""The yardstick of the mixed-precision MSDA op (fp16 / bf16 value, output and their gradients; fp32 locations, weights and
arithmetic): tests/msda_ref64.py on the EXACTLY up-cast inputs, its per-element fp32 bound widened by the one output rounding.

Test helper (not a conftest); tests/test_msda_h16_ref.py shows the bound admissible and sharp, tests/test_gpu_msda_h16.py judges the
kernels by it.

Contract (include/semidetr_hip.h, semidetr_msda_forward_h16): a result is the fp32 op applied to the up-cast 16-bit inputs --
every 16-bit number is an fp32 number, so the up-cast is exact and msda_ref64's bound B32 (2u n A + 2 C + tiny, derived there) holds
for the kernel's fp32 value r' before it is stored: |r' - ref| <= B32.  `out` and `grad_value` are then rounded ONCE to nearest
even, got = rn16(r'):

  * r' in the normal range of the 16-bit type: |got - r'| <= u16 |r'| with u16 = half an ulp relative = 2^-p for a p-bit
    significand (hidden bit included): fp16 p = 11 -> 2^-11, bf16 p = 8 -> 2^-8;
  * r' in the subnormal range: the spacing is 2^(emin - p + 1) -- fp16 2^-24, bf16 2^-133 -- and |got - r'| <= half of it:
    s16 = 2^-25 (fp16), 2^-134 (bf16);
  * |r'| <= |ref| + B32.

    |got - ref| <= B32 + u16 (|ref| + B32) + s16

No per-test factor.  The bound says nothing once |ref| + B32 reaches the type's largest finite number (the rounding may then
overflow to inf, as the contract says it does): tests/test_msda_h16_ref.py asserts that no fp16 case gets there, so overflow can
never excuse a kernel.  grad_sampling_loc and grad_attn_weight are returned in fp32, unrounded: the plain bound of msda_ref64.
"""
import numpy as np

import msda_ref64 as R

U16 = {"fp16": 2.0 ** -11, "bf16": 2.0 ** -8}
S16 = {"fp16": 2.0 ** -25, "bf16": 2.0 ** -134}
MAX16 = {"fp16": 65504.0, "bf16": float(np.float32(3.3895313892515355e38))}
ROUNDED = ("out", "grad_value")


def torch_dtype(dtype):
    import torch
    return {"fp16": torch.float16, "bf16": torch.bfloat16}[dtype]


def round16(x, dtype):
    """x (any float array) rounded to nearest even into the 16-bit type by torch on the CPU, returned as float32 (exact)."""
    import torch
    t = torch.from_numpy(np.array(x, dtype=np.float32, order="C"))      # (a copy: the cases' arrays are read-only)
    return t.to(torch_dtype(dtype)).to(torch.float32).numpy()


def widen16(b32, val, dtype):
    """The fp32 bound ``b32`` of a result whose reference value is ``val``, widened by the one rounding into the 16-bit type
    (module docstring): B32 + u16 (|ref| + B32) + s16.  Shared by every judge of a 16-bit result (add_norm_ref64,
    self_attn_ref64, query_select_ref64)."""
    return b32 + U16[dtype] * (np.abs(val) + b32) + S16[dtype]


class Bounded16:
    """A msda_ref64.Bounded result of a 16-bit output: the fp32 bound widened by the one rounding."""

    def __init__(self, b32, dtype):
        self.b32, self.dtype, self.val, self.skip = b32, dtype, b32.val, b32.skip

    def bound(self):
        return widen16(self.b32.bound(np.float32), self.val, self.dtype)

    def reach(self):
        """|ref| + B32: what the value before the rounding can be at most (the fp16 range condition)."""
        return np.abs(self.val) + self.b32.bound(np.float32)

    def ratio(self, got):
        got = np.asarray(got, np.float64).reshape(self.val.shape)
        r = np.abs(got - self.val) / self.bound()
        return np.where(np.isfinite(got), r, np.inf)


def reference(value16, shapes, loc, attn, gout16, dtype, exact=None):
    """value16 / gout16: float32 arrays holding 16-bit values exactly (round16).  -> dict of 'out', 'grad_value' (Bounded16) and
    'grad_loc', 'grad_attn' (msda_ref64.Bounded, fp32 bound); without gout16 only 'out'.  exact: msda_ref64.msda's flag of the
    samples whose fp32 pixel coordinates carry no rounding (locations stay fp32 in this op, so it means the same here)."""
    r = R.msda(np.asarray(value16, np.float64), shapes, loc, attn, None if gout16 is None else np.asarray(gout16, np.float64),
               exact=exact)
    return {k: (Bounded16(v, dtype) if k in ROUNDED else v) for k, v in r.items()}


def check(route, what, got, ref):
    """Assert got within the bound elementwise; returns the worst err / bound."""
    if not isinstance(ref, Bounded16):
        return R.check(route, what, got, ref)
    r = ref.ratio(got)
    worst = float(r.max()) if r.size else 0.0
    if not worst <= 1.0:
        idx = np.unravel_index(int(np.argmax(r)), r.shape)
        g = np.asarray(got, np.float64).reshape(ref.val.shape)[idx]
        raise AssertionError(f"{route} {what} ({ref.dtype}): {int((r > 1.0).sum())} element(s) out of bound, worst at "
                             f"{tuple(int(i) for i in idx)}: got {g!r} ref {ref.val[idx]!r} err/bound {worst:.3g} (bound "
                             f"{ref.bound()[idx]:.3g}, fp32 part {ref.b32.bound(np.float32)[idx]:.3g})")
    return worst
