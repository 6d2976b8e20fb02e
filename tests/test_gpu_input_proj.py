"""GPU: semi_detr_amd.group_norm_to_tokens / project_pyramid (csrc/group_norm_tokens.hip) against the float64 statement
tests/input_proj_ref64.py: every element of ``tokens``, ``q``, ``mean``, ``rstd``, ``dx`` of every level, ``dweight`` and ``dbias``
through ``check_gn_tokens`` on the cases of tests/input_proj_cases.py.  Before each call NaN-filled buffers of the results' sizes
are freed into the caching allocator, so an element a kernel does not write shows.

The module-level checks run the SAME modules (tests/input_proj_torch_restated.py) once through their own stock-torch forward and
once through ``project_pyramid``, and judge both against the restatement in float64 with the rule of tests/test_gpu_add_norm.py:
``max |hip - f64| <= FACTOR * max |fp32 restatement - f64|`` per tensor, FACTOR = 4.  The justification is the one given there:
across a conv, a norm, a second conv on the normalised level and a second norm the per-op bounds do not compose into anything
useful, the two fp32 sides share every conv and differ only in the order of sums of comparable depth, so their errors are draws
from the same distribution (a factor of 2 between the maxima of two draws) with another factor of 2 of head-room for the
256-element tensors (the norms' gradients); a wrong term is off by 1e-2 or more against errors of 1e-6.
"""
import ctypes

import numpy as np
import pytest
import torch
from torch import nn

import input_proj_cases as C
import input_proj_ref64 as R
import input_proj_torch_restated as T

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FACTOR = 4.0
TORCH16 = {None: torch.float32, "fp16": torch.float16, "bf16": torch.bfloat16}


def _poison(*shapes):
    junk = [torch.full(s, float("nan"), dtype=torch.float32, device=DEV) for s in shapes for _ in range(2)]
    del junk


def _dev(a, dtype=None):
    return None if a is None else torch.from_numpy(np.array(a)).to(DEV).to(TORCH16[dtype])


def _strided(t):
    """the same rows as the slice ``buf[:, 1:-1, :256]`` of a NaN-filled (N, S + 2, 512) buffer: row stride 512, batch stride
    (S + 2) * 512, an offset of one row -- never contiguous, whatever N is"""
    buf = torch.full((t.shape[0], t.shape[1] + 2, 2 * t.shape[2]), float("nan"), device=DEV, dtype=t.dtype)
    buf[:, 1:-1, :t.shape[2]] = t
    out = buf[:, 1:-1, :t.shape[2]]
    assert not out.is_contiguous() and out.stride(1) == 2 * t.shape[2] and torch.equal(out, t)
    return out


def _pos(case, dtype):
    t = _dev(case["pos"], dtype)
    if t is not None and case["pos_layout"] == "strided":
        t = _strided(t)
    return t


def _norms(case):
    norms = []
    for w, b in zip(case["weights"], case["biases"]):
        m = nn.GroupNorm(32, 256, eps=case["eps"]).to(DEV)
        with torch.no_grad():
            m.weight.copy_(_dev(w))
            m.bias.copy_(_dev(b))
        norms.append(m)
    return norms


def run(case, xs=None):
    """the raw forward (mean, rstd) and the autograd path of one case -> dict of numpy outputs (16-bit results up-cast)"""
    import semi_detr_amd as s
    x16, o16 = case["x16"], case["out16"]
    xs = [_dev(x, x16) for x in case["xs"]] if xs is None else xs
    pos, gy, gq = _pos(case, o16), _dev(case["gy"], o16), _dev(case["gq"], o16)
    norms = _norms(case)
    n, rows = xs[0].shape[0], sum(h * w for h, w in case["shapes"])
    full = (n, rows, 256)
    _poison(full, full)
    t0, q0, mean, rstd = s.group_norm_tokens_forward(xs, [m.weight for m in norms], [m.bias for m in norms], case["eps"], pos,
                                                     dtype=TORCH16[o16])
    got = {"mean": mean.cpu().numpy(), "rstd": rstd.cpu().numpy()}
    leaves = [x.detach().requires_grad_(True) for x in xs]
    if pos is not None:
        pos.requires_grad_(True)
    _poison(full, full)
    # 16-bit x and fp32 results is what autocast gives: GroupNorm is on its fp32 list, and the levels are read in place
    with torch.autocast("cuda", dtype=TORCH16[x16], enabled=x16 is not None and o16 is None):
        out, shapes, starts = s.group_norm_to_tokens(leaves, norms, pos)
    tokens, q = out if pos is not None else (out, None)
    assert tokens.dtype == TORCH16[o16] and tokens.is_contiguous() and torch.equal(tokens, t0) and (q is None or torch.equal(q, q0))
    assert shapes.tolist() == [list(hw) for hw in case["shapes"]] and starts.tolist() == list(R.level_rows(case)[1][:-1])
    got["tokens"] = tokens.detach().float().cpu().numpy()
    if q is not None:
        got["q"] = q.detach().float().cpu().numpy()
        if o16 is None:
            assert torch.equal(q, tokens + pos), "q is tokens + pos, from the same y"
    outs, grads = ([tokens], [gy]) if gy is not None else ([], [])
    if gq is not None:
        outs.append(q)
        grads.append(gq)
    _poison(*[tuple(x.shape) for x in xs], (256,), (256,))
    torch.autograd.backward(outs, grads)
    for l, x in enumerate(leaves):
        assert x.grad.dtype == x.dtype and x.grad.shape == x.shape
        got[f"dx{l}"] = x.grad.float().cpu().numpy()
    got["dweight"] = np.stack([m.weight.grad.cpu().numpy() for m in norms])
    got["dbias"] = np.stack([m.bias.grad.cpu().numpy() for m in norms])
    if pos is not None:
        assert (pos.grad is None) if gq is None else torch.equal(pos.grad, gq), "the gradient of pos is gq itself"
    return got


@pytest.mark.parametrize("name", C.names())
def test_case_within_bounds(name):
    case = C.cases()[name]
    got = run(case)
    for k, v in got.items():                         # the figures before the verdict: |err| / bound, a 16-bit output widened
        print(f"  {name}: {k} {R.ratio(v, R.widen16(C.reference(name)[k], C.out_dtypes(case).get(k))):.3g}")
    R.check_gn_tokens(case, got, name, C.reference(name), C.out_dtypes(case))


@pytest.mark.parametrize("name", ["pyr4_odd", "ragged_chunks"])
def test_two_runs_are_bitwise_equal(name):
    case = C.cases()[name]
    a, b = run(case), run(case)
    assert {"tokens", "mean", "rstd", "dx0", "dweight", "dbias"} <= set(a)
    assert all(a[k].tobytes() == b[k].tobytes() for k in a), "not bit-identical from run to run"


@pytest.mark.parametrize("name", ["pyr4_odd", "aligned_vec"])
def test_constant_group_gives_the_bias_bit_for_bit(name):
    case = C.cases()[name]
    got = run(case)
    hw = case["shapes"][0][0] * case["shapes"][0][1]
    assert got["tokens"][0, :hw, 0:8].tobytes() == np.broadcast_to(case["biases"][0][0:8], (hw, 8)).tobytes()
    assert got["mean"][0, 0, 0] == 1.375


@pytest.mark.parametrize("name", ["pyr4_odd", "aligned_vec"])
def test_channels_last_and_batch_sliced_inputs_give_the_contiguous_bits(name):
    case = C.cases()[name]
    want = run(case)
    cl = [_dev(x).to(memory_format=torch.channels_last) for x in case["xs"]]
    assert not cl[0].is_contiguous()
    sliced = []
    for x in case["xs"]:
        buf = torch.full((x.shape[0] + 2,) + x.shape[1:], float("nan"), device=DEV)
        buf[1:-1] = _dev(x)
        sliced.append(buf[1:-1])
    strided = [torch.stack([_dev(x), torch.full(x.shape, float("nan"), device=DEV)], 1)[:, 0] for x in case["xs"]]
    assert strided[0].stride(0) == 2 * 256 * case["shapes"][0][0] * case["shapes"][0][1] and not strided[0].is_contiguous()
    for xs in (cl, sliced, strided):
        got = run(case, xs)
        assert all(got[k].tobytes() == want[k].tobytes() for k in want)


@pytest.mark.parametrize("name", ["pyr4_odd", "pyr4_odd_fp16_out16", "pyr4_odd_bf16_out16"])
def test_strided_upstream_gradients_give_the_contiguous_bits(name):
    """autograd hands the backward contiguous gradients, so the reads through ``gy_stride`` / ``gq_stride`` are driven here:
    N = 2, 16-byte rows (fp32) and 8-byte rows (16-bit), gy and gq each as a strided slice"""
    import semi_detr_amd as s
    case = C.cases()[name]
    x16, o16 = case["x16"], case["out16"]
    xs, norms = [_dev(x, x16) for x in case["xs"]], _norms(case)
    weights = [m.weight for m in norms]
    _, _, mean, rstd = s.group_norm_tokens_forward(xs, weights, [m.bias for m in norms], case["eps"], None, dtype=TORCH16[o16])
    gy, gq = _dev(case["gy"], o16), _dev(case["gq"], o16)
    for a, b in ((gy, gq), (gy, None), (None, gq)):
        want = s.group_norm_tokens_backward(a, b, xs, weights, mean, rstd)
        layouts = [(None if a is None else _strided(a), None if b is None else _strided(b))]
        if a is not None and b is not None:
            layouts.append((_strided(a), b))
        for sa, sb in layouts:
            got = s.group_norm_tokens_backward(sa, sb, xs, weights, mean, rstd)
            for u, v in zip(got[0] + got[1] + got[2], want[0] + want[1] + want[2]):
                assert torch.equal(u, v)
        if a is not None and b is not None:                  # and those bits are the admissible ones
            res = {f"dx{l}": d.float().cpu().numpy() for l, d in enumerate(got[0])}
            res["dweight"], res["dbias"] = np.stack([d.cpu().numpy() for d in got[1]]), np.stack([d.cpu().numpy() for d in got[2]])
            R.check_gn_tokens(case, res, name, C.reference(name), C.out_dtypes(case))


@pytest.mark.parametrize("x16", ["fp16", "bf16"])
def test_a_16_bit_output_is_the_fp32_output_rounded_once(x16):
    import semi_detr_amd as s
    for shape_name in ("pyr4_odd", "one_9x33"):
        case = C.cases()[f"{shape_name}_{x16}_out16"]
        xs, norms = [_dev(x, x16) for x in case["xs"]], _norms(case)
        pos = _pos(case, x16)
        args = (xs, [m.weight for m in norms], [m.bias for m in norms], case["eps"])
        t16, q16, mean16, rstd16 = s.group_norm_tokens_forward(*args, pos, dtype=TORCH16[x16])
        t32, q32, mean32, rstd32 = s.group_norm_tokens_forward(*args, pos.float(), dtype=torch.float32)
        assert t16.dtype == TORCH16[x16] and torch.equal(t16, t32.to(TORCH16[x16])) and torch.equal(q16, q32.to(TORCH16[x16]))
        assert torch.equal(mean16, mean32) and torch.equal(rstd16, rstd32)
        gq = _dev(case["gq"], x16)
        d16 = s.group_norm_tokens_backward(None, gq, xs, args[1], mean16, rstd16)
        d32 = s.group_norm_tokens_backward(None, gq.float(), [x.float() for x in xs], args[1], mean16, rstd16)
        for a, b in zip(d16[0], d32[0]):
            assert a.dtype == TORCH16[x16] and torch.equal(a, b.to(TORCH16[x16]))
        for a, b in zip(d16[1] + d16[2], d32[1] + d32[2]):
            assert torch.equal(a, b)


def test_autocast_gives_fp32_tokens_without_an_fp32_copy_of_x():
    import semi_detr_amd as s
    n, shapes = 2, [(64, 96), (64, 96)]
    g = torch.Generator().manual_seed(3)
    xs = [torch.randn((n, 256) + hw, generator=g).to(DEV).bfloat16() for hw in shapes]
    norms = [nn.GroupNorm(32, 256).to(DEV) for _ in shapes]
    rows = sum(h * w for h, w in shapes)
    pos = torch.randn(n, rows, 256, generator=g).to(DEV)
    x_bytes = sum(x.numel() for x in xs)                      # elements: an fp32 copy of x would take 4 bytes of each
    results = 2 * n * rows * 256 * 4                          # tokens and q in fp32
    small = 4 << 20                                           # statistics, workspace, the allocator's rounding of two blocks
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16):
        (tokens, q), _, _ = s.group_norm_to_tokens(xs, norms, pos)
    torch.cuda.synchronize()
    assert tokens.dtype == torch.float32 and q.dtype == torch.float32
    peak = torch.cuda.max_memory_allocated() - before
    assert results <= peak <= results + small < results + 4 * min(x.numel() for x in xs), (peak, results, x_bytes)
    want, _ = T.norm_tokens([x.float() for x in xs], norms)
    assert (tokens - want).abs().max() < 1e-4


# ------------------------------------------------------------------------------------------------------------------
# module level
# ------------------------------------------------------------------------------------------------------------------
def _judge(name, hip, rest32, ref64):
    assert len(hip) == len(rest32) == len(ref64)
    worst = 0.0
    for i, (h, r, d) in enumerate(zip(hip, rest32, ref64)):
        if d is None:
            assert h is None and r is None, (name, i)
            continue
        scale = float((r.double() - d).abs().max())
        err = float((h.double() - d).abs().max())
        assert torch.isfinite(h).all(), (name, i)
        if scale == 0:                                   # the restatement is exact here (the gradient of pos is the seed of q)
            assert err == 0, (name, i, err)
            continue
        worst = max(worst, err / scale)
        assert err <= FACTOR * scale, f"{name}[{i}]: |hip - f64| = {err:.3e}, |fp32 restatement - f64| = {scale:.3e}"
    print(f"  {name}: {len(hip)} tensors, worst |hip - f64| / |fp32 restatement - f64| = {worst:.2f}")


def _pyramid_problem(levels):
    g = torch.Generator().manual_seed(20 + levels)
    torch.manual_seed(20 + levels)                                    # the convs draw from the global generator
    channels = [24, 40, 56]
    proj = T.build_input_proj(channels, levels)
    T.randomize_norms(proj, g)
    sizes = [(21, 30), (11, 15), (6, 8)]
    feats = [torch.randn((2, c) + hw, generator=g) for c, hw in zip(channels, sizes)]
    out_sizes = sizes + [(3, 4), (2, 2)][:levels - 3]
    rows = sum(h * w for h, w in out_sizes)
    pos, seed_t, seed_q = (torch.randn(2, rows, 256, generator=g) for _ in range(3))
    return proj.to(DEV), [f.to(DEV) for f in feats], pos.to(DEV), [seed_t.to(DEV), seed_q.to(DEV)], out_sizes


@pytest.mark.parametrize("levels", [4, 5])
def test_project_pyramid_against_the_restatement(levels):
    import semi_detr_amd as s
    proj, feats, pos, seeds, out_sizes = _pyramid_problem(levels)
    sides = {}
    for side in ("rest", "hip", "f64"):
        m = T.in_float64(proj) if side == "f64" else proj
        cast = (lambda t: t.double()) if side == "f64" else (lambda t: t)
        fs, p_ = [cast(f).requires_grad_(True) for f in feats], cast(pos).requires_grad_(True)
        if side == "hip":
            tokens, q, shapes, starts, srcs = s.project_pyramid(m, fs, levels, p_)
            assert shapes.tolist() == [list(hw) for hw in out_sizes] and len(srcs) == levels
            want_t, _, want_shapes, want_starts = T.project(m, fs, levels)
            assert torch.equal(shapes, want_shapes) and torch.equal(starts, want_starts)
            for src, st, hw in zip(srcs, starts.tolist(), out_sizes):   # the NCHW views hold the reference's srcs
                assert src.shape == (2, 256) + hw and torch.equal(src.flatten(2).transpose(1, 2), tokens[:, st:st + hw[0] * hw[1]])
            assert torch.equal(q, tokens + p_)
        else:
            tokens, q = T.project(m, fs, levels, p_)[:2]
        grads = torch.autograd.grad([tokens, q], fs + [p_] + list(m.parameters()), [cast(t) for t in seeds], allow_unused=True)
        sides[side] = [tokens.detach(), q.detach()] + list(grads)
    assert all(t is not None for t in sides["hip"]), "every conv and norm parameter of every level receives a gradient"
    _judge(f"project_pyramid, {levels} levels", sides["hip"], sides["rest"], sides["f64"])


def test_encoder_forward_takes_the_query_the_projection_wrote():
    import add_norm_torch_restated as TA
    from semi_detr_amd import add_norm
    import semi_detr_amd as s
    proj, feats, pos, seeds, out_sizes = _pyramid_problem(4)
    g = torch.Generator().manual_seed(9)
    torch.manual_seed(9)
    enc = TA.Encoder(1, 512, 0.0)
    TA.randomize_norms(enc, g)
    enc = enc.to(DEV)
    sides = {}
    for side in ("rest", "hip", "f64"):
        m, e = (T.in_float64(proj), TA.in_float64(enc)) if side == "f64" else (proj, enc)
        cast = (lambda t: t.double()) if side == "f64" else (lambda t: t)
        fs, p_ = [cast(f).requires_grad_(True) for f in feats], cast(pos).requires_grad_(True)
        if side == "hip":
            tokens, q, shapes, starts, _ = s.project_pyramid(m, fs, 4, p_)
            out = add_norm.encoder_forward(e, tokens, p_, shapes, starts, None, None, query=q)[0]
            plain = add_norm.encoder_forward(e, tokens, p_, shapes, starts, None, None)[0]
            assert torch.equal(out, plain), "q is tokens + pos bit for bit, so layer 0 sees the same query"
        else:
            tokens, _, shapes, starts = T.project(m, fs, 4, p_)
            out = e(tokens, p_, shapes, starts, None, None)[0]
        grads = torch.autograd.grad([out], fs + [p_] + list(m.parameters()) + list(e.parameters()), [cast(seeds[0])])
        sides[side] = [out.detach()] + list(grads)
    _judge("projection + one encoder layer", sides["hip"], sides["rest"], sides["f64"])


# ------------------------------------------------------------------------------------------------------------------
# C ABI
# ------------------------------------------------------------------------------------------------------------------
def test_cabi_refusals_return_the_status_and_write_nothing():
    from semi_detr_amd import _lib
    lib = _lib.lib()
    fill = dict.fromkeys(("x", "w", "b", "tokens", "q", "pos", "mean", "rstd", "gy", "dx", "dw", "work"), 7.0)
    fill["b"] = 3.0                                   # x is constant, so the accepted call below writes the bias
    bufs = {k: torch.full((4096,), v, device=DEV) for k, v in fill.items()}

    def block(**kw):
        p = _lib.GnTokens()
        p.batch, p.levels, p.channels, p.groups, p.eps, p.tokens_per_image = 1, 2, 256, 32, 1e-5, 3
        for l, (hw, start) in enumerate(((2, 0), (1, 2))):
            p.hw[l], p.start[l] = hw, start
            p.x[l], p.weight[l], p.bias[l] = bufs["x"].data_ptr(), bufs["w"].data_ptr(), bufs["b"].data_ptr()
            p.grad_x[l], p.grad_weight[l] = bufs["dx"].data_ptr(), bufs["dw"].data_ptr()
        p.tokens, p.mean, p.rstd, p.gy = (bufs[k].data_ptr() for k in ("tokens", "mean", "rstd", "gy"))
        p.gy_stride[0], p.gy_stride[1] = 768, 256
        for k, v in kw.items():
            setattr(p, k, v)
        return p

    stream = _lib.current_stream_ptr()
    work = ctypes.c_void_p(bufs["work"].data_ptr())
    fwd, bwd = lib.semidetr_gn_tokens_forward, lib.semidetr_gn_tokens_backward
    for fn, kw, rc, text in ((fwd, dict(channels=128), -1, b"128 channels"), (fwd, dict(levels=9), -1, b"9 levels"),
                             (fwd, dict(q=bufs["q"].data_ptr()), -1, b"q and pos"), (bwd, dict(gy=None), -1, b"gy and gq"),
                             (fwd, dict(x_type=5), -1, b"unknown type code"), (bwd, dict(out_type=7), -1, b"unknown type code"),
                             (fwd, dict(batch=1 << 12, tokens_per_image=1 << 12), -2, b"too large")):
        assert fn(stream, ctypes.byref(block(**kw)), work, 4096 * 4) == rc and text in lib.semidetr_last_error(), (kw, lib.semidetr_last_error())
    torch.cuda.synchronize()
    assert all(bool((t == fill[k]).all()) for k, t in bufs.items()), "a refused call wrote something"
    assert fwd(stream, ctypes.byref(block()), work, 4096 * 4) == 0        # the same block, accepted
    torch.cuda.synchronize()
    assert bool((bufs["tokens"][:768] == 3.0).all()) and bool((bufs["tokens"][768:] == 7.0).all()) and bool((bufs["q"] == 7.0).all())
