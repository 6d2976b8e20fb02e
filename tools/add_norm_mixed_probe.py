#!/usr/bin/env python
"""Time the glue of one transformer layer (tools/add_norm_probe.py: the positional add, the residual adds and the LayerNorms,
forward + backward) in the mixed-precision contexts, three routes side by side in the same run:

    torch    the stock ops of the restatement in that context
    upcast   what ``add_layer_norm`` did before the kernels read 16-bit rows: explicit ``.float()`` copies of every 16-bit
             operand, the ``*_f32`` entry points, ``.to(dtype)`` of every result; the backward up-casts the saved 16-bit tensors
             again and casts ``dx`` once per dtype asked for (tests/test_gpu_add_norm_mixed.py shows it to be the same
             computation bit for bit)
    mixed    ``semi_detr_amd.add_layer_norm``: the ``*_mixed`` entry points, every row read and written in its own dtype

    python tools/add_norm_mixed_probe.py [--calls 50] [--out profiles/add_norm_mixed_probe.txt]

contexts: ``autocast_bf16`` / ``autocast_fp16`` -- fp32 parameters and residual stream, the branches (and the decoder's query_pos)
16-bit, as the GEMMs under autocast leave them; ``half_module`` -- everything fp16, autocast off; ``fp32`` -- everything fp32
(``upcast`` and ``mixed`` are then the same ``*_f32`` launches: the row that shows the fp32 path did not move).
Protocol of tools/add_norm_probe.py: device events over ``--calls`` calls after a warm-up, the routes alternating in ``--blocks``
blocks, every call on the next of ``--rotate`` (>= 4) input sets, median of the blocks (min .. max); kernels per call counted with
torch.profiler in a pass of their own.
"""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import add_norm_probe as P                                           # noqa: E402

D = P.D
ROUTES = ("torch", "upcast", "mixed")
CONTEXTS = ("autocast_bf16", "autocast_fp16", "half_module", "fp32")


class UpcastRoute(torch.autograd.Function):
    """``add_layer_norm`` as it ran on 16-bit operands before the mixed kernels: torch cast passes around the fp32 kernels"""

    @staticmethod
    def forward(ctx, x, residual, weight, bias, eps, pos):
        from semi_detr_amd import _lib
        from semi_detr_amd.add_norm import _result_dtypes, add_layer_norm_forward
        f = lambda t: None if t is None else t.float()
        y, q, mean, rstd = add_layer_norm_forward(f(x), f(residual), weight, bias, eps, f(pos))
        ctx.save_for_backward(x, residual, weight, mean, rstd)
        ctx.set_materialize_grads(False)
        ctx.dtypes = (x.dtype, None if residual is None else residual.dtype, weight.dtype, bias.dtype, None if pos is None else pos.dtype)
        y_dtype, q_dtype = _result_dtypes(*ctx.dtypes[:2], ctx.dtypes[4])
        return _lib.cast(y, y_dtype) if pos is None else (_lib.cast(y, y_dtype), _lib.cast(q, q_dtype))

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, gy, gq=None):
        from semi_detr_amd import _lib
        from semi_detr_amd.add_norm import add_layer_norm_backward
        x, residual, weight, mean, rstd = ctx.saved_tensors
        dt = ctx.dtypes
        f = lambda t: None if t is None else t.float()
        dx, dw, db = add_layer_norm_backward(f(gy), f(gq), f(x), f(residual), weight, mean, rstd)
        gx = _lib.cast(dx, dt[0])
        gres = None if residual is None else (gx if dt[1] == dt[0] else _lib.cast(dx, dt[1]))
        return gx, gres, _lib.cast(dw, dt[2]), _lib.cast(db, dt[3]), None, _lib.cast(gq, dt[4])


def add_ln(route):
    if route == "mixed":
        from semi_detr_amd import add_layer_norm
        return add_layer_norm
    return lambda x, res, w, b, eps, pos=None: UpcastRoute.apply(x, res, w, b, eps, pos)


def encoder_glue(route, ln, src, pos, b1, b2):
    if route == "torch":
        x1 = ln[0](src + b1)
        x2 = ln[1](x1 + b2)
        return [x2 + pos, x2]
    op = add_ln(route)
    x1 = op(b1, src, ln[0].weight, ln[0].bias, ln[0].eps)
    x2, q = op(b2, x1, ln[1].weight, ln[1].bias, ln[1].eps, pos=pos)
    return [q, x2]


def decoder_glue(route, ln, tgt, pos, b_sa, b_ca, b_ffn):
    if route == "torch":
        q1 = tgt + pos
        t1 = ln[1](tgt + b_sa)
        q2 = t1 + pos
        t2 = ln[0](t1 + b_ca)
        t3 = ln[2](t2 + b_ffn)
        return [q1, q2, t3, ln[3](t3)]
    op = add_ln(route)
    q1 = tgt + pos
    t1, q2 = op(b_sa, tgt, ln[1].weight, ln[1].bias, ln[1].eps, pos=pos)
    t2 = op(b_ca, t1, ln[0].weight, ln[0].bias, ln[0].eps)
    t3 = op(b_ffn, t2, ln[2].weight, ln[2].bias, ln[2].eps)
    return [q1, q2, t3, op(t3, None, ln[3].weight, ln[3].bias, ln[3].eps)]


# inputs: which are 16-bit under autocast (the stream and the encoder's pos stay fp32; branches and the decoder's query_pos are
# GEMM outputs)
SHAPES = {"encoder": dict(shape=(4, 20000, D), glue=encoder_glue, inputs=("f32", "f32", "h16", "h16"), outputs=2, norms=2),
          "decoder": dict(shape=(1100, 4, D), glue=decoder_glue, inputs=("f32", "h16", "h16", "h16", "h16"), outputs=4, norms=4)}


def autocast(context):
    if context in ("half_module", "fp32"):
        return torch.autocast("cuda", enabled=False)
    return torch.autocast("cuda", dtype=torch.bfloat16 if context == "autocast_bf16" else torch.float16)


def dtype_of(kind, context):
    if context == "fp32":
        return torch.float32
    if context == "half_module":
        return torch.float16
    return torch.float32 if kind == "f32" else (torch.bfloat16 if context == "autocast_bf16" else torch.float16)


def call(cfg, route, context, ln, ins, seeds):
    ins = [t.detach().requires_grad_(True) for t in ins]
    with autocast(context):
        outs = cfg["glue"](route, ln, *ins)
    params = [p for m in ln for p in (m.weight, m.bias)]
    return outs, torch.autograd.grad(outs, ins + params, [s.to(o.dtype) if s.dtype != o.dtype else s for s, o in zip(seeds, outs)])


def timed(cfg, route, context, ln, sets, calls):
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for i in range(calls):
        call(cfg, route, context, ln, *sets[i % len(sets)])
    stop.record()
    stop.synchronize()
    return start.elapsed_time(stop) * 1e3 / calls                # microseconds per call


def kernels_per_call(cfg, route, context, ln, sets):
    from torch.profiler import ProfilerActivity, profile
    try:
        with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
            call(cfg, route, context, ln, *sets[0])
            torch.cuda.synchronize()
        names = {}
        for e in prof.events():
            if "cuda" in str(e.device_type).lower() and "memcpy" not in e.name.lower() and "memset" not in e.name.lower():
                key = e.name.replace("(anonymous namespace)::", "").replace("void ", "").split("(")[0][:48]
                names[key] = names.get(key, 0) + 1
        return (sum(names.values()), names) if names else None
    except Exception as exc:                                      # the measurement is optional; the timing is not
        print("profiler:", exc)
        return None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--blocks", type=int, default=5)
    ap.add_argument("--rotate", type=int, default=4)
    ap.add_argument("--contexts", default=",".join(CONTEXTS))
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert a.rotate >= 4, "at least four input sets, so that the tensors come from HBM"
    assert torch.cuda.is_available(), "the probe needs a GPU"
    dev = torch.device("cuda:0")
    lines = [f"# tools/add_norm_mixed_probe.py on {torch.cuda.get_device_name(0)}, torch {torch.__version__}: glue of one "
             f"transformer layer, forward + backward, D = {D}; {a.calls} calls x {a.blocks} alternating blocks, {a.rotate} rotating "
             "input sets; us per call: median of the blocks (min .. max)"]

    def flush():
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "w") as f:
                f.write("\n".join(lines) + "\n")

    for label, cfg in SHAPES.items():
        shape = cfg["shape"]
        g = torch.Generator(device="cpu").manual_seed(len(label))
        base = [([torch.randn(shape, generator=g) for _ in cfg["inputs"]], [torch.randn(shape, generator=g) for _ in range(cfg["outputs"])])
                for _ in range(a.rotate)]
        for context in a.contexts.split(","):
            ln = P.norms(cfg["norms"], dev)
            if context == "half_module":
                ln = [m.half() for m in ln]
            sets = [([t.to(dev).to(dtype_of(k, context)) for t, k in zip(ins, cfg["inputs"])],
                     [t.to(dev).to(dtype_of("h16", context) if context == "half_module" else torch.float32) for t in seeds])
                    for ins, seeds in base]
            res = {r: call(cfg, r, context, ln, *sets[0]) for r in ROUTES}
            same = all(torch.equal(x, y) for x, y in zip(list(res["upcast"][0]) + list(res["upcast"][1]),
                                                         list(res["mixed"][0]) + list(res["mixed"][1])))
            diff = max(float((x.detach().float() - y.detach().float()).abs().max() / x.detach().float().abs().max())
                       for x, y in zip(list(res["torch"][0]) + list(res["torch"][1]), list(res["mixed"][0]) + list(res["mixed"][1])))
            del res
            lines.append(f"{label} layer, {shape[0]} x {shape[1]} x {D}, {context}: upcast and mixed bitwise equal: {same}; largest "
                         f"max |torch - mixed| / max |torch| over outputs and gradients {diff:.2e}")
            t = {r: [] for r in ROUTES}
            for r in ROUTES:
                timed(cfg, r, context, ln, sets, 10)
            for _ in range(a.blocks):
                for r in ROUTES:
                    t[r].append(timed(cfg, r, context, ln, sets, a.calls))
            med = {r: float(np.median(v)) for r, v in t.items()}
            lines.append("  forward + backward  " + "   ".join(f"{r} {med[r]:8.1f} ({min(t[r]):.1f} .. {max(t[r]):.1f})" for r in ROUTES)
                         + f"   upcast / mixed = {med['upcast'] / med['mixed']:.2f}   torch / mixed = {med['torch'] / med['mixed']:.2f}")
            print("\n".join(lines[-2:]), flush=True)
            flush()
            for r in ROUTES:
                n = kernels_per_call(cfg, r, context, ln, sets)
                if n is None:
                    lines.append(f"  kernels per call, {r}: not measured (the profiler gave no device events)")
                else:
                    top = ", ".join(f"{c} x {nm}" for nm, c in sorted(n[1].items(), key=lambda kv: -kv[1]))
                    lines.append(f"  kernels per call, {r}: {n[0]}   [{top}]")
                print(lines[-1], flush=True)
            flush()
            del sets
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
