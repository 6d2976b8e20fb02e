"""GPU: the exact MSDA backward (semidetr_msda_backward_exact_f32, MSDeformAttnExactFunction, MSDeformAttn.exact_backward).

grad_value is the exact sum of its fp32 contributions rounded once, so on ONE run each its bits must not move under anything that
keeps the set of contributions: a second call, a permutation of the queries or of the points of a level, the pixel flag (another
gather kernel, the same entries), the image's position in the batch, a swap of the heads.  tests/test_msda_exact_ref.py shows that
sequential fp32 summation fails the permutation test on case (a), i.e. that these tests discriminate.  Every result is also within
the fp64 reference's per-element bounds (tests/msda_ref64.py; grad_value with n = DEPTH + 1, derived in tests/msda_exact_ref.py),
and equal bit for bit to the numpy + integer model of the route.  Cases: tests/msda_exact_cases.py.  Run with -s for the figures.
"""
import ctypes

import numpy as np
import pytest
import torch

import msda_exact_cases as C
import msda_exact_ref as X
import msda_ref64 as R

pytestmark = pytest.mark.gpu

PIXELS = 1          # SEMIDETR_MSDA_QUERIES_ARE_PIXELS


def _dev(case):
    t = {k: torch.from_numpy(np.ascontiguousarray(case[k])).cuda() for k in ("value", "loc", "attn", "gout")}
    t["shapes"] = torch.from_numpy(case["shapes"]).cuda()
    t["starts"] = torch.cat([t["shapes"].new_zeros(1), (t["shapes"][:, 0] * t["shapes"][:, 1]).cumsum(0)[:-1]])
    return t


def run_front_end(t):
    """through the compiled front end (it sets the pixel flag itself when the queries are the pixels) -> numpy gv, gl, ga"""
    import semi_detr_amd  # noqa: F401  (registers the compiled front end under the reference's module name)
    import MultiScaleDeformableAttention as MSDA
    gv, gl, ga = MSDA.ms_deform_attn_exact_backward(t["value"], t["shapes"], t["starts"], t["loc"], t["attn"], t["gout"], 64)
    return gv.cpu().numpy(), gl.cpu().numpy(), ga.cpu().numpy()


def run_c_abi(t, flags=0, prefill=None):
    """a direct call of the C entry with `flags`; grad_value pre-filled with `prefill` -> numpy gv, gl, ga and the kernels' names"""
    from semi_detr_amd import _lib
    lib = _lib.lib()
    N, S, M, D = t["value"].shape
    _, Lq, _, L, P, _ = t["loc"].shape
    need = lib.semidetr_msda_exact_workspace_bytes(N, S, M, L, Lq, P)
    assert need > 0
    work = torch.empty(need, dtype=torch.uint8, device="cuda")
    gv = torch.empty_like(t["value"]) if prefill is None else torch.full_like(t["value"], prefill)
    gl, ga = torch.empty_like(t["loc"]), torch.empty_like(t["attn"])
    _lib.call("semidetr_msda_backward_exact_f32", t["value"].device, t["gout"], t["value"], t["shapes"], t["starts"], t["loc"], t["attn"],
              N, S, M, D, L, Lq, P, flags, work, ctypes.c_size_t(need), gv, gl, ga)
    names = lib.semidetr_msda_last_kernels().decode()
    return gv.cpu().numpy(), gl.cpu().numpy(), ga.cpu().numpy(), names


def same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint32), np.ascontiguousarray(b).view(np.uint32))


def check_bounds(name, case, gv, gl, ga):
    ref = R.msda(case["value"], case["shapes"], case["loc"], case["attn"], case["gout"])
    w = [R.check(name, "grad_value", gv, X.bounded_exact(ref["grad_value"])), R.check(name, "grad_loc", gl, ref["grad_loc"]),
         R.check(name, "grad_attn", ga, ref["grad_attn"])]
    print("%s: worst err / bound grad_value %.3f (n = DEPTH + 1) grad_loc %.3f grad_attn %.3f" % (name, *w))


_results = {}


def result(name):
    """one run of each case through the front end, shared by the tests below (the arrays are not modified)"""
    if name not in _results:
        case = getattr(C, "case_" + name)()
        _results[name] = (case, _dev(case)) + run_front_end(_dev(case))
    return _results[name]


@pytest.mark.parametrize("name", ["a", "b", "c5", "c1", "d"])
def test_within_the_fp64_bounds_and_equal_to_the_model(name):
    case, _, gv, gl, ga = result(name)
    check_bounds(name, case, gv, gl, ga)
    assert same_bits(gv, X.model(case["shapes"], case["loc"], case["attn"], case["gout"])), "grad_value differs from the exact model"


def test_long_row_is_split_and_merged():
    case, _, gv, _, _ = result("d")
    dest, contrib = X.contributions(case["shapes"], case["loc"], case["attn"], case["gout"])
    assert len(dest) == 8192 > C.split_len() and len(set(dest.tolist())) == 1
    assert same_bits(gv.reshape(-1), X.exact_grad_value(1, 1, 1, dest, contrib)[0].reshape(-1))


def test_exact_fraction_sum_bit_for_bit():
    """case (e): contributions equal grad_out exactly, so grad_value is the Fraction sum of the grad_out rows sampling the pixel"""
    case, _, gv, _, _ = result("e")
    N, Lq, M, _, P, _ = case["loc"].shape
    g = case["gout"].reshape(N, Lq, M, C.D)
    pix = case["pix"].reshape(N, Lq, M, P, 2)
    want = np.zeros((N, 16, M, C.D), np.uint32)
    for n in range(N):
        for m in range(M):
            rows = pix[n, :, m, :, 1] * 4 + pix[n, :, m, :, 0]              # (Lq, P)
            for r in range(16):
                qs = np.nonzero(rows == r)[0]                               # a query counts once per point on the pixel
                for d in range(C.D):
                    want[n, r, m, d] = X.exact_sum_bits(g[n, qs, m, d])
    assert np.array_equal(gv.view(np.uint32), want)
    big = np.abs(gv) >= 2.0 ** 99
    assert big.any() and (np.abs(gv[~big]) < 1e3).all()      # both outcomes occur: 2^100 survives, or cancels and leaves the small sum


def test_two_calls_give_the_same_bits():
    _, t, gv, gl, ga = result("a")
    gv2, gl2, ga2 = run_front_end(t)
    assert same_bits(gv, gv2) and same_bits(gl, gl2) and same_bits(ga, ga2)


def test_query_permutation():
    _, t, gv, _, _ = result("a")
    perm = torch.from_numpy(np.random.default_rng(1).permutation(t["loc"].shape[1])).cuda()
    tp = dict(t, loc=t["loc"][:, perm].contiguous(), attn=t["attn"][:, perm].contiguous(), gout=t["gout"][:, perm].contiguous())
    assert same_bits(gv, run_front_end(tp)[0])


def test_point_permutation_within_a_level():
    _, t, gv, _, _ = result("a")
    pp = torch.tensor([2, 0, 3, 1]).cuda()
    tp = dict(t, loc=t["loc"][:, :, :, :, pp].contiguous(), attn=t["attn"][:, :, :, :, pp].contiguous())
    assert same_bits(gv, run_front_end(tp)[0])


@pytest.mark.parametrize("name", ["b", "c5"])
def test_pixel_flag_changes_the_gather_not_the_bits(name):
    case, t, gv, gl, ga = result(name)
    assert case["pixels"]
    with_flag = run_c_abi(t, PIXELS)
    without = run_c_abi(t, 0)
    assert same_bits(with_flag[0], without[0]) and same_bits(gv, without[0])
    # the front end set the flag itself (queries = pixels of an exact tiling): its small gradients are the patch gather's
    assert same_bits(gl, with_flag[1]) and same_bits(ga, with_flag[2])
    check_bounds(name + " (no flag)", case, *without[:3])


def test_batch_position():
    _, t, gv, _, _ = result("a")
    one = {k: (v[1:2].contiguous() if k in ("value", "loc", "attn", "gout") else v) for k, v in t.items()}
    assert same_bits(gv[1:2], run_front_end(one)[0])


def test_head_swap():
    _, t, gv, _, _ = result("a")
    N, Lq, M = t["loc"].shape[:3]
    sw = dict(t, value=t["value"].flip(2).contiguous(), loc=t["loc"].flip(2).contiguous(), attn=t["attn"].flip(2).contiguous(),
              gout=t["gout"].view(N, Lq, M, C.D).flip(2).reshape(N, Lq, M * C.D).contiguous())
    assert same_bits(gv[:, :, ::-1], run_front_end(sw)[0])


def test_non_finite_grad_out():
    """case (f): NaN if a NaN or both infinities reach the element, else the infinity, else the finite exact sum -- and elements no
    planted row reaches keep the bits of case (a)"""
    case, _, gv, _, _ = result("f")
    _, _, gv_a, _, _ = result("a")
    dest, contrib = X.contributions(case["shapes"], case["loc"], case["attn"], case["gout"])
    N, S, M = case["value"].shape[:3]
    assert same_bits(gv, X.exact_grad_value(N, S, M, dest, contrib)[0])
    touched = np.zeros((N * S * M, C.D), bool)
    np.logical_or.at(touched, dest, ~np.isfinite(contrib))
    touched = touched.reshape(N, S, M, C.D)
    assert same_bits(gv[~touched], gv_a[~touched]) and not np.isfinite(gv[touched]).any() and np.isfinite(gv[~touched]).all()
    last = gv[0, S - 1, 0]                                       # the 1 x 1 level's pixel, head 0: all three planted rows meet
    assert np.isnan(last[0:16]).all() and (last[16:24] == -np.inf).all() and np.isfinite(last[24:]).all()
    assert np.isposinf(gv).any() and np.isneginf(gv).any()


def test_grad_value_needs_no_fill_and_reports_its_kernels():
    case, t, gv, _, _ = result("a")
    got, _, _, names = run_c_abi(t, 0, prefill=float("nan"))
    assert np.isfinite(got).all() and same_bits(got, gv)
    assert (got.reshape(-1, C.D)[X.exact_grad_value(*case["value"].shape[:3], *X.contributions(
        case["shapes"], case["loc"], case["attn"], case["gout"]))[1].reshape(-1) == 0] == 0).all()      # rows nobody samples: zeros
    assert names.startswith("msda_bwd_gather_d32+") and "exact_reduce" in names and "fillBufferAligned" not in names


# ---- module level ---------------------------------------------------------------------------------------------------------------

def _module_setup(dtype=torch.float32):
    from semi_detr_amd import MSDeformAttn
    torch.manual_seed(0)
    m = MSDeformAttn(256, 4, 8, 4).cuda()
    with torch.no_grad():
        m.sampling_offsets.weight.normal_(0, 0.02)
        m.attention_weights.weight.normal_(0, 0.1)
    levels = [(20, 27), (10, 14), (5, 7), (3, 4)]
    shapes = torch.as_tensor(levels, dtype=torch.long).cuda()
    ls = torch.cat([shapes.new_zeros(1), (shapes[:, 0] * shapes[:, 1]).cumsum(0)[:-1]])
    S = sum(h * w for h, w in levels)
    q, src = torch.randn(2, 50, 256).cuda(), torch.randn(2, S, 256).cuda()
    ref = torch.rand(2, 50, 4, 4).cuda()
    ref[..., 2:] = ref[..., 2:] * 0.2 + 0.05
    gout = torch.randn(2, 50, 256).cuda()
    return m, (q, ref, src, shapes, ls), gout


def _module_grads(m, inputs, gout):
    import semi_detr_amd  # noqa: F401
    import MultiScaleDeformableAttention as MSDA
    q, ref, src, shapes, ls = inputs
    q, src = q.clone().requires_grad_(True), src.clone().requires_grad_(True)
    m.zero_grad(set_to_none=True)
    calls = []
    orig = MSDA.ms_deform_attn_exact_backward
    MSDA.ms_deform_attn_exact_backward = lambda *a: (calls.append(1), orig(*a))[1]
    try:
        m(q, ref, src, shapes, ls).backward(gout)
    finally:
        MSDA.ms_deform_attn_exact_backward = orig
    grads = {"query": q.grad, "src": src.grad}
    grads.update({k: p.grad for k, p in m.named_parameters()})
    return {k: v.detach().cpu().numpy() for k, v in grads.items()}, bool(calls)


def test_module_exact_backward_matches_the_default_and_repeats_bit_for_bit():
    m, inputs, gout = _module_setup()
    want, used = _module_grads(m, inputs, gout)
    assert not used
    m.exact_backward = True
    got, used = _module_grads(m, inputs, gout)
    assert used, "exact_backward = True and a backward follows: the exact entry must be what runs"
    for k in want:        # the tolerances of tests/test_gpu_module.py (close())
        np.testing.assert_allclose(got[k], want[k], rtol=1e-3, atol=2e-4 * np.abs(want[k]).max(), err_msg=k)
    again, _ = _module_grads(m, inputs, gout)
    for k in got:
        assert same_bits(got[k], again[k]), k


def test_module_auto_follows_torchs_switch_and_no_grad_is_untouched():
    from semi_detr_amd import _lib, convert_exact_backward
    m, inputs, gout = _module_setup()
    lib = _lib.lib()
    with torch.no_grad():
        m(*inputs)
    today = lib.semidetr_msda_last_kernels().decode()
    assert convert_exact_backward(m, "auto") == 1
    assert not _module_grads(m, inputs, gout)[1]
    was = torch.are_deterministic_algorithms_enabled()
    torch.use_deterministic_algorithms(True)
    try:
        assert _module_grads(m, inputs, gout)[1]
    finally:
        torch.use_deterministic_algorithms(was)
    assert not _module_grads(m, inputs, gout)[1]
    m.exact_backward = True
    with torch.no_grad():
        m(*inputs)
    assert lib.semidetr_msda_last_kernels().decode() == today, "a no-grad call does what it does today"
    # channels per head != 32: the entry refuses, the module takes today's route
    from semi_detr_amd import MSDeformAttn
    m16 = MSDeformAttn(64, 4, 4, 4).cuda()
    m16.exact_backward = True
    q, ref, src, shapes, ls = inputs
    assert not _module_grads(m16, (q[..., :64].contiguous(), ref, src[..., :64].contiguous(), shapes, ls), gout[..., :64].contiguous())[1]


def test_module_16bit_value_goes_through_the_upcast_into_the_exact_function():
    m, inputs, gout = _module_setup()
    m = m.half()
    m.exact_backward = True
    q, ref, src, shapes, ls = inputs
    got, used = _module_grads(m, (q.half(), ref.half(), src.half(), shapes, ls), gout.half())
    assert used and all(np.isfinite(v.astype(np.float32)).all() for v in got.values())
    again, _ = _module_grads(m, (q.half(), ref.half(), src.half(), shapes, ls), gout.half())
    for k in got:
        assert np.array_equal(got[k].view(np.uint16), again[k].view(np.uint16)), k
