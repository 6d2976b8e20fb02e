"""The self-attention's C ABI on the GPU, as the tests drive it (tests/test_gpu_self_attn_h16.py, tests/test_gpu_self_attn_bits.py,
tools/gen_self_attn_bits.py): one forward and one backward of a problem of tests/self_attn_cases.py through the entry points
of either arithmetic, into NaN-filled buffers, in the case's own layout."""
import ctypes
import hashlib

import torch

import self_attn_cases as C
import self_attn_h16_ref64 as R16
from msda_h16_ref import torch_dtype

DEV = "cuda:0"
DTYPES = ("fp32",) + tuple(R16.DTYPES)
# what tests/golden/self_attn_bits.json pins: these cases (``full_size`` is ``self_attn_cases.full_size()``), each in every type,
# with all three gradients; the named ones also with a gradient subset (``q``: no dK / dV launch; ``kv``: the query-side
# kernel returns after delta)
BITS_CASES = ("L1_B1", "L33_B1", "L65_B3_masked", "L257_B3_masked", "lq_ne_lk", "lq_ne_lk_wide", "dn_edges_in_tiles",
              "dn_skipped_tiles", "one_open_key", "large_scores", "scale_given", "blocked_row", "full_size")
BITS_SUBSETS = {"lq_ne_lk": ("q", "kv")}


def _nan(shape, dtype):
    return torch.full(shape, float("nan"), dtype=dtype, device=DEV)


def run_abi(p, dt, want="qkv", layout=None, grads=None, shift8=False, raw=False):
    """One forward (+ one backward for the gradients named in ``want``) through the C ABI, every result buffer pre-filled with
    NaN.  ``dt`` in ``DTYPES``: ``"fp16"`` / ``"bf16"`` drive ``semidetr_self_attn_{forward,backward}_h16`` on the operands of
    ``p`` rounded to that type, ``"fp32"`` drives ``semidetr_self_attn_{forward,backward}_f32`` with the ``SelfAttn`` block on the
    unrounded operands.  ``shift8``: q, k, v are slices whose rows start 8 bytes into a 16-byte line.  -> dict of CPU tensors
    (``out``, ``lse``, ``dq``, ``dk``, ``dv``; an unasked gradient keeps its fill), up-cast to fp32 unless ``raw``."""
    from semi_detr_amd import _lib, self_attn
    native = dt != "fp32"
    tdt = torch_dtype(dt) if native else torch.float32
    ops = R16.rounded(p, dt) if native else p
    suffix, block = ("h16", _lib.SelfAttnH16) if native else ("f32", _lib.SelfAttn)
    q, k, v = (torch.from_numpy(ops[n]).to(DEV).to(tdt) for n in "qkv")
    (Lq, B, E), Lk = q.shape, k.shape[0]
    layout = layout or p["layout"]
    packed = layout == "packed" and Lq == Lk
    if packed:
        buf = torch.cat([q, k, v], dim=2)
        q, k, v = buf[..., :E], buf[..., E:2 * E], buf[..., 2 * E:]
        gbuf = _nan((Lq, B, 3 * E), tdt)
        gq, gk, gv = gbuf[..., :E], gbuf[..., E:2 * E], gbuf[..., 2 * E:]
    else:
        gq, gk, gv = _nan(q.shape, tdt), _nan(k.shape, tdt), _nan(v.shape, tdt)
    if shift8:
        q, k, v = (torch.cat([t.new_zeros(t.shape[0], B, 4), t], dim=2)[..., 4:] for t in (q, k, v))
        assert all(t.data_ptr() % 16 == 8 and t.stride(0) % 4 == 0 for t in (q, k, v))
    mask = None if p["mask"] is None else torch.from_numpy(p["mask"]).to(DEV).view(torch.uint8)
    scale = 32 ** -0.5 if p["scale"] is None else float(p["scale"])
    blk = self_attn._params(q, k, v, mask, p["heads"], scale, block)
    if native:
        blk.type = _lib.row_type(tdt)
    out, lse = _nan((Lq, B, E), tdt), _nan((B, p["heads"], Lq), torch.float32)
    blk.out, blk.lse = out.data_ptr(), lse.data_ptr()
    work, nbytes = self_attn._workspace(blk, q.device)
    _lib.call("semidetr_self_attn_forward_" + suffix, q.device, ctypes.byref(blk), work, nbytes)
    got = {"out": out, "lse": lse}
    if (grads if grads is not None else not p["forward_only"]):
        g = torch.from_numpy(ops["gout"]).to(DEV).to(tdt)
        blk.grad_out = g.data_ptr()
        for n, t in (("q", gq), ("k", gk), ("v", gv)):
            if n in want:
                _lib.set_rows(blk, "grad_" + n, t, f"g{n}_stride")
        work2, nbytes = self_attn._workspace(blk, q.device)
        work2.fill_(0xFF)                    # the backward may use another workspace than the forward, uninitialised
        _lib.call("semidetr_self_attn_backward_" + suffix, q.device, ctypes.byref(blk), work2, nbytes)
        got.update(dq=gq, dk=gk, dv=gv)
    torch.cuda.synchronize()
    return {n: (t if raw else t.float()).cpu() for n, t in got.items()}


def bits(dt):
    """``"<case>/<dt>/<want>"`` -> {result name: sha256 of its raw bytes} for every run of ``BITS_CASES`` in type ``dt``."""
    out = {}
    for name in BITS_CASES:
        p = C.full_size() if name == "full_size" else C.cases()[name]
        for want in ("qkv",) + BITS_SUBSETS.get(name, ()):
            got = run_abi(p, dt, want=want, raw=True)
            out[f"{name}/{dt}/{want}"] = {n: hashlib.sha256(t.contiguous().view(torch.uint8).numpy().tobytes()).hexdigest()
                                          for n, t in got.items()}
    return out
