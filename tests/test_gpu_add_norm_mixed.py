"""GPU: the mixed-type add + LayerNorm kernels (csrc/add_norm.hip, ``semidetr_add_norm_forward_mixed`` /
``semidetr_add_norm_backward_mixed``): rows of fp32, fp16 and bf16 elements read and written inside the kernels.

1. The C ABI directly, on the dtype matrix of tests/mixed_precision_cases.py and a 1-row case: every result is bit for bit the
   ``*_f32`` entry point on the up-cast operands followed by torch's ``.to(dtype)``, admissible under ``check_add_norm16``, and
   the same from run to run; ``mean``, ``rstd``, ``grad_weight`` and ``grad_bias`` are the fp32 call's bits.
2. Rounding where it is controllable: ``grad_pos`` is a pure conversion of ``gq`` (ties of both parities, their neighbours, the
   largest finite value, the first that rounds to inf, subnormals, signed zeros), and a ``y`` beyond 65504 leaves as inf in fp16.
3. Layout: 16-bit slices whose rows start 8 bytes into a 16-byte line are read in place.
4. No detour through fp32: the peak memory of ``add_layer_norm`` forward and backward.
5. The identity contracts of the gradients of ``residual`` and ``pos``.
6. The two instances of the one kernel template against each other: the ``*_mixed`` entry points with every type code
   ``SEMIDETR_ROW_F32`` are bit for bit the ``*_f32`` entry points on the same buffers.
"""
import ctypes

import numpy as np
import pytest
import torch
from torch.nn import functional as F

import add_norm_cases as AC
import add_norm_ref64 as AR
import mixed_precision_cases as M
from msda_h16_ref import round16, torch_dtype

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F32 = torch.float32


def _rows3(t):
    return t if t is None or t.dim() == 3 else t.reshape(1, -1, 256)


def _block(cls, eps, operands, results, mixed):
    from semi_detr_amd import _lib
    x = operands["x"]
    p = cls()
    p.rows0, p.rows1, p.dim, p.eps = x.shape[0], x.shape[1], 256, eps
    for n, t in operands.items():
        if t is not None:
            assert t.stride(2) == 1
            _lib.set_rows(p, n, t)
            if mixed:
                setattr(p, n + "_type", _lib.row_type(t.dtype))
    for n, t in results.items():
        if t is not None:
            assert t.is_contiguous()
            setattr(p, n, t.data_ptr())
            if mixed and n not in ("mean", "rstd", "weight", "bias", "grad_weight", "grad_bias"):
                setattr(p, n + "_type", _lib.row_type(t.dtype))
    return p


def abi_forward(x, res, pos, w, b, eps, y_dtype=F32, q_dtype=F32, mixed=True):
    """the forward entry point itself (``mixed``: semidetr_add_norm_forward_mixed, else _f32) -> y, q, mean, rstd"""
    from semi_detr_amd import _lib
    rows = x.shape[0] * x.shape[1]
    y = torch.full(x.shape, float("nan"), dtype=y_dtype, device=DEV)
    q = torch.full(x.shape, float("nan"), dtype=q_dtype, device=DEV) if pos is not None else None
    mean, rstd = (torch.full((rows,), float("nan"), device=DEV) for _ in range(2))
    p = _block(_lib.AddNormMixed if mixed else _lib.AddNorm, eps, dict(x=x, residual=res, pos=pos),
               dict(y=y, q=q, mean=mean, rstd=rstd, weight=w, bias=b), mixed)
    _lib.call("semidetr_add_norm_forward_mixed" if mixed else "semidetr_add_norm_forward_f32", x.device, ctypes.byref(p), None, 0)
    return y, q, mean, rstd


def abi_backward(gy, gq, x, res, w, mean, rstd, gx_dtype=F32, gres_dtype=None, gpos_dtype=None, mixed=True, sums=True):
    """the backward entry point itself -> grad_x, grad_residual, grad_pos, grad_weight, grad_bias (None: not asked for;
    ``sums`` = False asks for neither parameter gradient and hands over no workspace: one launch)"""
    from semi_detr_amd import _lib
    rows = x.shape[0] * x.shape[1]
    gx, gres, gpos = (None if d is None else torch.full(x.shape, float("nan"), dtype=d, device=DEV)
                      for d in (gx_dtype, gres_dtype, gpos_dtype))
    dw, db = (torch.full((256,), float("nan"), device=DEV) if sums else None for _ in range(2))
    results = dict(grad_x=gx, grad_weight=dw, grad_bias=db, mean=mean, rstd=rstd, weight=w)
    if mixed:
        results.update(grad_residual=gres, grad_pos=gpos)
    p = _block(_lib.AddNormMixed if mixed else _lib.AddNorm, 0.0, dict(x=x, residual=res, gy=gy, gq=gq), results, mixed)
    nbytes = _lib.lib().semidetr_add_norm_workspace_bytes(rows) if sums else 0
    work = torch.full((nbytes // 4,), float("nan"), device=DEV) if sums else None
    _lib.call("semidetr_add_norm_backward_mixed" if mixed else "semidetr_add_norm_backward_f32", x.device, ctypes.byref(p),
              work, nbytes)
    return gx, gres, gpos, dw, db


def _place(a, kind, dt, layout="contiguous"):
    if a is None:
        return None
    t = torch.from_numpy(np.array(a, np.float32)).to(DEV)
    if kind == "h16":
        t = t.to(torch_dtype(dt))
    t = _rows3(t)
    return t.transpose(0, 1).contiguous().transpose(0, 1) if layout == "transposed" else t


def _up(t):
    return None if t is None else t.float()


def _np(t):
    return t.detach().float().cpu().numpy()


def _same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8))


def _one_row_case(combo, context):
    """``r1_plain`` of add_norm_cases in the dtypes of ``combo`` / ``context`` (mixed_precision_cases.add_norm_case needs three
    rows for its special ones)"""
    dt, src = M.DTYPE16[context], AC.cases()["r1_plain"]
    res_kind, pos_kind = M.COMBOS[combo]
    half = context == "half_module"
    r16 = lambda a: round16(a, dt)
    as_kind = lambda a, kind: None if kind is None else (r16(a) if kind == "h16" else np.array(a, np.float32))
    return dict(name=f"r1_plain/{combo}/{context}", shape=src["shape"], layout="contiguous", eps=src["eps"], dtype16=dt,
                x=r16(src["x"]), residual=as_kind(src["residual"], res_kind), pos=as_kind(src["pos"], pos_kind),
                weight=r16(src["weight"]) if half else src["weight"], bias=r16(src["bias"]) if half else src["bias"],
                gy=r16(src["gy"]) if half else src["gy"], gq=(r16(src["gq"]) if half else src["gq"]) if pos_kind else None,
                kinds=dict(x="h16", residual=res_kind, pos=pos_kind, weight="h16" if half else "f32",
                           bias="h16" if half else "f32"), context=context)


NAMES = M.add_norm_names() + [("r1_plain", c, ctx) for ctx in M.CONTEXTS
                              for c in (M.HALF_COMBOS if ctx == "half_module" else M.AUTOCAST_COMBOS)]


# ------------------------------------------------------------------------------------------------------------------
# 1. the C ABI on the dtype matrix
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("base,combo,context", NAMES, ids=["/".join(n) for n in NAMES])
def test_entry_points_are_the_fp32_entry_points_rounded_once(base, combo, context):
    if base == "r1_plain":
        case = _one_row_case(combo, context)
        ref = AR.ref64(case)
    else:
        case, ref = M.add_norm_case(base, combo, context), M.add_norm_reference(base, combo, context)
    dt, k, lay, want = case["dtype16"], case["kinds"], case["layout"], M.derived_dtypes(case)
    tdt = lambda kind: None if kind is None else (torch_dtype(dt) if kind == "h16" else F32)
    x, res, pos = (_place(case[n], k[n], dt, lay) for n in ("x", "residual", "pos"))
    w, b = (torch.from_numpy(np.array(case[n])).to(DEV) for n in ("weight", "bias"))          # fp32 vectors, exact
    gy = _place(case["gy"], want["y"], dt, lay)                      # an upstream gradient has its result's dtype
    gq = _place(case["gq"], want["q"], dt, lay)
    if lay == "transposed":
        assert not x.is_contiguous()

    def run(mixed):
        if mixed:
            y, q, mean, rstd = abi_forward(x, res, pos, w, b, case["eps"], tdt(want["y"]), tdt(want["q"]) or F32)
            gx, gres, gpos, dw, db = abi_backward(gy, gq, x, res, w, mean, rstd, tdt(want["dx"]), tdt(want["dx_res"]),
                                                  tdt(want["dpos"]))
        else:
            y, q, mean, rstd = abi_forward(_up(x), _up(res), _up(pos), w, b, case["eps"], mixed=False)
            gx, _, _, dw, db = abi_backward(_up(gy), _up(gq), _up(x), _up(res), w, mean, rstd, mixed=False)
            gres, gpos = (gx if res is not None else None), (_up(gq) if pos is not None else None)
        return dict(y=y, q=q, mean=mean, rstd=rstd, dx=gx, dx_res=gres, dpos=gpos, dweight=dw, dbias=db)
    got, plain, again = run(True), run(False), run(True)
    for n, t in got.items():
        if t is None:
            assert plain[n] is None or n == "dpos", n
            continue
        assert torch.equal(t, plain[n].to(t.dtype)) and t.dtype == (tdt(want.get(n)) if n in ("y", "q", "dx", "dx_res", "dpos") else F32), \
            f"{case['name']}: {n} is not the fp32 entry point's result converted once"
        assert _same_bits(t, again[n]), f"{case['name']}: {n} differs from run to run"
    for n in ("mean", "rstd", "dweight", "dbias"):
        assert _same_bits(got[n], plain[n]), f"{case['name']}: {n} is not the fp32 call's"
    judged = {n: _np(got[n]) for n in ("y", "q", "dx", "dx_res", "dweight", "dbias") if got[n] is not None}
    judged["kinds"] = {n: ("f32" if got[n].dtype == F32 else "h16") for n in judged}
    rep = M.check_add_norm16(case, judged, ref)
    print("\n" + " ".join(f"{n}[{judged['kinds'][n]}]={v:.3g}" for n, v in rep.items()) + f"  {case['name']}")


@pytest.mark.parametrize("dt", M.DTYPES)
@pytest.mark.parametrize("sums", [True, False])
def test_every_row_in_one_16_bit_type(dt, sums):
    """all rows fp16, all rows bf16 (no context of mixed_precision_cases has the second), with and without the parameter sums:
    the bits of the fp32 entry points on the up-cast operands"""
    from semi_detr_amd import _lib
    case = M.add_norm_case("r2051_contiguous", "res16_pos16", "half_module")
    t16 = torch_dtype(dt)
    x, res, pos, gy, gq = (_place(case[n], "f32", dt).to(t16) for n in ("x", "residual", "pos", "gy", "gq"))
    w, b = (torch.from_numpy(np.array(case[n])).to(DEV) for n in ("weight", "bias"))

    def run(mixed):
        c = (lambda t: t) if mixed else _up
        d = t16 if mixed else F32
        y, q, mean, rstd = abi_forward(c(x), c(res), c(pos), w, b, case["eps"], d, d, mixed=mixed)
        if sums:
            gx = abi_backward(c(gy), c(gq), c(x), c(res), w, mean, rstd, d, mixed=mixed)[0]
        else:                                                        # one launch: neither parameter gradient
            gx = torch.full(x.shape, float("nan"), dtype=d, device=DEV)
            p = _block(_lib.AddNormMixed if mixed else _lib.AddNorm, 0.0, dict(x=c(x), residual=c(res), gy=c(gy), gq=c(gq)),
                       dict(grad_x=gx, mean=mean, rstd=rstd, weight=w), mixed)
            _lib.call("semidetr_add_norm_backward_mixed" if mixed else "semidetr_add_norm_backward_f32", x.device, ctypes.byref(p), None, 0)
        return y, q, gx
    for n, a, c in zip(("y", "q", "dx"), run(True), run(False)):
        assert a.dtype == t16 and torch.equal(a, c.to(t16)), f"{dt}: {n} is not the fp32 entry point's result converted once"


def test_grad_x_alone_and_grad_residual_alone_are_the_same_dx():
    """``grad_x`` and ``grad_residual`` may each be NULL: either one alone carries the bits it carries next to the other"""
    case = M.add_norm_case("r65_transposed", "res32", "autocast_bf16")
    x, res = _place(case["x"], "h16", "bf16", "transposed"), _place(case["residual"], "f32", "bf16", "transposed")
    w, b = (torch.from_numpy(np.array(case[n])).to(DEV) for n in ("weight", "bias"))
    gy = _place(case["gy"], "f32", "bf16")
    _, _, mean, rstd = abi_forward(x, res, None, w, b, case["eps"])
    both = abi_backward(gy, None, x, res, w, mean, rstd, torch.bfloat16, F32)
    only_x = abi_backward(gy, None, x, res, w, mean, rstd, torch.bfloat16, None)
    only_res = abi_backward(gy, None, x, res, w, mean, rstd, None, F32)
    assert only_x[1] is None and only_res[0] is None
    assert torch.equal(only_x[0], both[0]) and torch.equal(only_res[1], both[1]) and torch.equal(both[0], both[1].bfloat16())
    assert torch.equal(only_x[3], both[3]) and torch.equal(only_res[4], both[4]) and torch.isfinite(both[1]).all()


# ------------------------------------------------------------------------------------------------------------------
# 2. rounding
# ------------------------------------------------------------------------------------------------------------------
def _special_values(dt):
    """fp32 values around every rounding decision of the conversion into ``dt``"""
    f = np.float32
    frac, emin, sub = (10, -14, -24) if dt == "fp16" else (7, -126, -133)          # kept fraction bits, smallest normal, subnormal
    ulp = 2.0 ** -frac
    ties = [1.0 + 0.5 * ulp, 1.0 + 1.5 * ulp, 1.0 + 2.5 * ulp, 2.0 - 0.5 * ulp,    # kept mantissa even / odd below the tie
            3.0 * 2.0 ** 7 + 0.5 * ulp * 2.0 ** 8]
    big = float(M.MAX16[dt])
    first_inf = big + 2.0 ** (15 - frac - 1) if dt == "fp16" else None               # fp16: 65520
    vals = []
    for t in ties:
        vals += [t, np.nextafter(f(t), f(np.inf)), np.nextafter(f(t), f(0))]
    vals += [big, np.nextafter(f(big), f(0))]
    if dt == "fp16":
        assert first_inf == 65520.0
        vals += [first_inf, np.nextafter(f(first_inf), f(0)), np.nextafter(f(first_inf), f(np.inf)), 1e6, 3.0e38]
    else:
        bits = np.array([0x7f7f8000, 0x7f7f7fff, 0x7f7f8001], np.uint32).view(np.float32)    # the tie to inf and its neighbours
        vals += list(bits)
    tiny = 2.0 ** sub                                                    # the smallest subnormal of the type
    vals += [tiny, 0.5 * tiny, np.nextafter(f(0.5 * tiny), f(1)), np.nextafter(f(0.5 * tiny), f(0)), 1.5 * tiny, 2.5 * tiny,
             3.0 * tiny, 2.0 ** emin, 2.0 ** emin - tiny, 2.0 ** emin - 0.5 * tiny, 0.0]
    vals = np.array(vals, np.float32)
    return np.concatenate([vals, -vals])


@pytest.mark.parametrize("dt", M.DTYPES)
def test_grad_pos_is_torchs_conversion_of_gq(dt):
    rng = np.random.default_rng(5)
    r0, r1 = 3, 7
    special = _special_values(dt)
    assert special.size <= 256 and np.signbit(special[special == 0]).any()
    gq_np = rng.standard_normal((r0, r1, 256)).astype(np.float32)
    flat = gq_np.reshape(-1, 256)
    flat[0, :special.size] = special
    flat[1, 256 - special.size:] = special[::-1]
    flat[2] = np.resize(special, 256)
    gq = torch.from_numpy(gq_np).to(DEV)
    x = torch.from_numpy(rng.standard_normal((r0, r1, 256)).astype(np.float32)).to(DEV).to(torch_dtype(dt))
    w, b = torch.ones(256, device=DEV), torch.zeros(256, device=DEV)
    _, _, mean, rstd = abi_forward(x, None, None, w, b, 1e-5)
    gx, _, gpos, _, _ = abi_backward(None, gq, x, None, w, mean, rstd, torch_dtype(dt), None, torch_dtype(dt))
    want = gq.to(torch_dtype(dt))
    got_bits, want_bits = (t.view(torch.int16).cpu().numpy().reshape(-1) for t in (gpos, want))
    bad = np.flatnonzero(got_bits != want_bits)
    assert bad.size == 0, [(float(gq_np.reshape(-1)[i]), hex(got_bits[i] & 0xffff), hex(want_bits[i] & 0xffff)) for i in bad[:8]]
    host = want.float().cpu().numpy().reshape(-1, 256)[0, :special.size]
    assert np.isinf(host).any() and (host == 0).sum() > 2                      # the values do reach inf and zero
    if dt == "fp16":
        assert np.abs(host[host != 0]).min() == 2.0 ** -24 and (np.abs(host) == 65504.0).any()
    assert torch.isfinite(gx[1:]).all()


def test_a_y_beyond_the_fp16_range_leaves_as_inf():
    rng = np.random.default_rng(6)
    x = torch.from_numpy(rng.standard_normal((2, 9, 256)).astype(np.float32)).to(DEV).half()
    pos = torch.from_numpy(rng.standard_normal((2, 9, 256)).astype(np.float32)).to(DEV).half()
    w = torch.full((256,), 1.0e5, device=DEV)
    w[::2] = 3.0e4
    b = torch.zeros(256, device=DEV)
    y, q, _, _ = abi_forward(x, None, pos, w, b, 1e-5, torch.float16, torch.float16)
    y32, q32, _, _ = abi_forward(x.float(), None, pos.float(), w, b, 1e-5, mixed=False)
    assert torch.equal(y, y32.half()) and torch.equal(q, q32.half())
    assert torch.isinf(y).any() and torch.isfinite(y).any() and not torch.isnan(y).any()
    assert torch.equal(torch.isinf(y), y32.abs() >= 65520.0)


# ------------------------------------------------------------------------------------------------------------------
# 3. layout: rows 8 bytes into a 16-byte line
# ------------------------------------------------------------------------------------------------------------------
def _slice8(t):
    """``t`` (r0, r1, 256), 16-bit, as the slice [:, :, 4:260] of a NaN-filled (r0, r1, 264) buffer"""
    buf = torch.full(t.shape[:2] + (264,), float("nan"), dtype=t.dtype, device=DEV)
    assert buf.data_ptr() % 16 == 0
    buf[:, :, 4:260] = t
    return buf[:, :, 4:260]


@pytest.mark.parametrize("context", ["half_module", "autocast_bf16"])
def test_16_bit_slices_at_8_bytes_are_read_in_place(context):
    import semi_detr_amd as s
    from semi_detr_amd import _lib
    combo = "res16_pos16" if context == "half_module" else "res32_pos16"
    case = M.add_norm_case("r65_transposed", combo, context)
    dt, k = case["dtype16"], case["kinds"]
    plain = {n: _place(case[n], k[n], dt) for n in ("x", "residual", "pos")}
    w, b = (_place(case[n], k[n], dt).reshape(256) for n in ("weight", "bias"))
    sliced = {n: (_slice8(t) if t.dtype != F32 else t) for n, t in plain.items()}
    for n, t in sliced.items():
        if t.dtype != F32:
            assert t.data_ptr() % 16 == 8 and not t.is_contiguous()
            assert _lib.rows_native(t).data_ptr() == t.data_ptr(), f"{n} was copied"

    def run(ops):
        leaves = {n: t.detach().requires_grad_(True) for n, t in ops.items()}
        with M.autocast(context):
            y, q = s.add_layer_norm(leaves["x"], leaves["residual"], w, b, case["eps"], leaves["pos"])
        gy, gq = _place(case["gy"], "f32", dt).to(y.dtype), _place(case["gq"], "f32", dt).to(q.dtype)
        if ops is sliced and gy.dtype != F32:
            gy, gq = _slice8(gy), _slice8(gq)
        torch.autograd.backward([y, q], [gy, gq])
        return [y.detach(), q.detach()] + [leaves[n].grad for n in ("x", "residual", "pos")]
    a, c = run(plain), run(sliced)
    for i, (u, v) in enumerate(zip(a, c)):
        assert u.dtype == v.dtype and torch.equal(u, v) and not torch.isnan(v).any(), i


# ------------------------------------------------------------------------------------------------------------------
# 4. no detour through fp32
# ------------------------------------------------------------------------------------------------------------------
def _nbytes(*tensors):
    return sum(t.numel() * t.element_size() for t in tensors if t is not None)


@pytest.mark.parametrize("context,combo", [("half_module", "res16_pos16"), ("autocast_bf16", "res32")])
def test_peak_memory_has_no_fp32_copies(context, combo):
    import semi_detr_amd as s
    from semi_detr_amd import _lib
    case = M.add_norm_case("r2051_contiguous", combo, context)
    dt, k = case["dtype16"], case["kinds"]
    x, res, pos = (_place(case[n], k[n], dt) for n in ("x", "residual", "pos"))
    w, b = (_place(case[n], k[n], dt).reshape(256) for n in ("weight", "bias"))
    leaves = [t.requires_grad_(True) for t in (x, res, pos, w, b) if t is not None]
    rows = x.shape[0] * x.shape[1]
    s.add_layer_norm(x.detach(), res.detach(), w.detach(), b.detach(), case["eps"])       # the library is loaded
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    with M.autocast(context):
        out = s.add_layer_norm(x, res, w, b, case["eps"], pos)
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    outs = list(out) if pos is not None else [out]
    kept = _nbytes(*outs) + 2 * rows * 4                                 # y, q and the saved fp32 mean and rstd
    print(f"\n{case['name']}: forward peak {peak} B, returned and saved {kept} B")
    assert peak <= 2 * kept, f"forward: peak {peak} B above twice the {kept} B of y, q, mean, rstd"
    seeds = [_place(case["gy"], "f32", dt).to(outs[0].dtype)] + ([_place(case["gq"], "f32", dt).to(outs[1].dtype)] if pos is not None else [])
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    torch.autograd.backward(outs, seeds)
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    assert all(t.grad is not None and t.grad.dtype == t.dtype for t in leaves)
    wanted = _nbytes(*[t.grad for t in leaves]) + _lib.lib().semidetr_add_norm_workspace_bytes(rows)
    print(f"{case['name']}: backward peak {peak} B, gradients of the leaves and workspace {wanted} B")
    assert peak <= 2 * wanted, f"backward: peak {peak} B above twice the {wanted} B of the leaves' gradients and the workspace"


# ------------------------------------------------------------------------------------------------------------------
# 5. identity contracts
# ------------------------------------------------------------------------------------------------------------------
@pytest.fixture
def launches(monkeypatch):
    """[(entry point, {field: pointer or None})] of every add_norm launch made through ``_lib.call``"""
    from semi_detr_amd import _lib
    seen, inner = [], _lib.call

    def call(name, dev, *args):
        if name.startswith("semidetr_add_norm_backward"):
            p = args[0]._obj
            seen.append((name, {f: getattr(p, f, None) for f in ("grad_x", "grad_residual", "grad_pos")}))
        return inner(name, dev, *args)
    monkeypatch.setattr(_lib, "call", call)
    return seen


def test_equal_16_bit_dtypes_share_one_kernel_output(launches):
    import semi_detr_amd as s
    g = torch.Generator().manual_seed(3)
    x, res, pos = (torch.randn(5, 13, 256, generator=g).to(DEV).half().requires_grad_(True) for _ in range(3))
    w, b = (torch.randn(256, generator=g).to(DEV).half().requires_grad_(True) for _ in range(2))
    gy, gq = (torch.randn(5, 13, 256, generator=g).to(DEV).half() for _ in range(2))
    y, q = s.add_layer_norm(x, res, w, b, 1e-5, pos)
    assert y.dtype == q.dtype == torch.float16
    torch.autograd.backward([y, q], [gy, gq])
    assert len(launches) == 1 and launches[0][0] == "semidetr_add_norm_backward_mixed"
    assert launches[0][1]["grad_x"] and not launches[0][1]["grad_residual"] and not launches[0][1]["grad_pos"]
    assert x.grad.dtype == res.grad.dtype == torch.float16 and torch.equal(x.grad, res.grad)
    assert pos.grad.dtype == torch.float16 and torch.equal(pos.grad, gq)
    # the values: the fp32 call on the up-cast operands, rounded once
    leaves = [t.detach().float().requires_grad_(True) for t in (x, res, pos, w, b)]
    y32, q32 = s.add_layer_norm(leaves[0], leaves[1], leaves[3], leaves[4], 1e-5, leaves[2])
    torch.autograd.backward([y32, q32], [gy.float(), gq.float()])
    assert launches[-1][0] == "semidetr_add_norm_backward_f32"
    assert torch.equal(y, y32.half()) and torch.equal(q, q32.half())
    for t, t32 in zip((x, res, w, b), (leaves[0], leaves[1], leaves[3], leaves[4])):
        assert torch.equal(t.grad, t32.grad.half())


def test_fp16_x_with_bf16_residual_promotes_and_splits_dx(launches):
    import semi_detr_amd as s
    g = torch.Generator().manual_seed(4)
    x0, r0 = torch.randn(3, 22, 256, generator=g).to(DEV).half(), torch.randn(3, 22, 256, generator=g).to(DEV).bfloat16()
    w0, b0 = (torch.randn(256, generator=g).to(DEV) for _ in range(2))
    gy = torch.randn(3, 22, 256, generator=g).to(DEV)

    def run(op, cast=lambda t: t):
        leaves = [cast(t).detach().clone().requires_grad_(True) for t in (x0, r0, w0, b0)]
        with torch.autocast("cuda", enabled=False):
            y = op(*leaves)
        y.backward(gy.to(y.dtype))
        return [y.detach()] + [t.grad for t in leaves]
    stock = run(lambda x, r, w, b: F.layer_norm(x + r, (256,), w, b, 1e-5))
    got = run(lambda x, r, w, b: s.add_layer_norm(x, r, w, b, 1e-5))
    assert [t.dtype for t in got] == [t.dtype for t in stock] == [F32, torch.float16, torch.bfloat16, F32, F32]
    assert launches[0][0] == "semidetr_add_norm_backward_mixed" and launches[0][1]["grad_x"] and launches[0][1]["grad_residual"]
    plain = run(lambda x, r, w, b: s.add_layer_norm(x, r, w, b, 1e-5), cast=lambda t: t.float())
    assert all(t.dtype == F32 for t in plain)
    for n, a, c in zip(("y", "dx", "dres", "dweight", "dbias"), got, plain):
        assert torch.equal(a, c.to(a.dtype)), f"{n} is not the fp32 result rounded once"
    assert torch.equal(plain[1], plain[2])


# ------------------------------------------------------------------------------------------------------------------
# 6. the two instances of the one kernel template
# ------------------------------------------------------------------------------------------------------------------
# rows0 x rows1: 1 row; 5 = a partly filled batch of four; 17 crosses a backward wave's 16 rows; 67 puts a second backward
# workgroup on a 3-row tail; 129 = three slots, an uneven chunk of the parameter sums
INSTANCE_SHAPES = [(1, 1), (5, 1), (1, 17), (67, 1), (3, 43)]
PRESENCE = {"residual_pos_gy_gq": dict(residual=True, pos=True, gy=True, gq=True),
            "residual_gy": dict(residual=True, pos=False, gy=True, gq=False),
            "pos_gq": dict(residual=False, pos=True, gy=False, gq=True)}
INSTANCE_CASES = [(sh, pr, "contiguous") for sh in INSTANCE_SHAPES for pr in PRESENCE] + [((3, 43), "residual_pos_gy_gq", "transposed")]


@pytest.mark.parametrize("shape,presence,layout", INSTANCE_CASES,
                         ids=[f"r{a * b}_{a}x{b}/{pr}/{lay}" for (a, b), pr, lay in INSTANCE_CASES])
def test_all_fp32_codes_are_the_fp32_entry_points_bit_for_bit(shape, presence, layout):
    """Every output buffer starts as NaN, so an element one instance leaves unwritten shows; the operands are finite."""
    have, g = PRESENCE[presence], torch.Generator().manual_seed(11 * shape[0] + shape[1])

    def rows(present=True):
        if not present:
            return None
        if layout == "transposed":                                   # read through a (rows1, rows0, 256) tensor's strides
            t = torch.randn(shape[1], shape[0], 256, generator=g).to(DEV).transpose(0, 1)
            assert not t.is_contiguous() or 1 in shape
            return t
        return torch.randn(*shape, 256, generator=g).to(DEV)
    x, res, pos, gy, gq = rows(), rows(have["residual"]), rows(have["pos"]), rows(have["gy"]), rows(have["gq"])
    w, b = (torch.randn(256, generator=g).to(DEV) for _ in range(2))

    def run(mixed, sums):
        y, q, mean, rstd = abi_forward(x, res, pos, w, b, 1e-5, mixed=mixed)
        only_mixed = dict(gres_dtype=F32 if res is not None else None, gpos_dtype=F32 if gq is not None else None) if mixed else {}
        gx, gres, gpos, dw, db = abi_backward(gy, gq, x, res, w, mean, rstd, mixed=mixed, sums=sums, **only_mixed)
        return dict(y=y, q=q, mean=mean, rstd=rstd, grad_x=gx, grad_weight=dw, grad_bias=db), gres, gpos
    for sums in (True, False):
        (typed, gres, gpos), (plain, _, _) = run(True, sums), run(False, sums)
        for n, t in plain.items():
            assert (t is None) == (typed[n] is None) == (n == "q" and pos is None or n in ("grad_weight", "grad_bias") and not sums), n
            if t is not None:
                assert not torch.isnan(t).any() and not torch.isnan(typed[n]).any(), f"{n}: elements left unwritten"
                assert _same_bits(typed[n], t), f"{n} (sums={sums}): the typed instance on fp32 codes is not the fp32 instance"
        assert (gres is not None) == have["residual"] and (gpos is not None) == have["gq"]
        assert gres is None or _same_bits(gres, typed["grad_x"]), "grad_residual is not grad_x"
        assert gpos is None or _same_bits(gpos, gq), "grad_pos is not gq"
