"""GPU: every MSDA kernel route at samples exactly on the pixel lattice, on the map's skip edges, on the last valid line of a
padded image, and at non-finite locations (tests/msda_lattice_cases.py), against the fp64 reference built with msda_ref64's
`exact` flag: on those samples delta is 0, nothing is excluded from grad_loc and no edge allowance is made, so floor's cell, the
strict skip test and zero padding are judged by the derived bound like any other number.  No tolerance is introduced here.

Beside the bound, with no allowance at all: every result is finite; grad_attn and grad_loc / grad_offsets of a sample that no
correct kernel can take (skipped and exact, non-finite, or further than 2 delta from the skip edge) are 0; padded pixels receive
exactly zero grad_value; a (query, head) row without a sample on the map gives exact zeros in `out`.  Before every call
NaN-filled buffers of the results' sizes are freed into the caching allocator: an element a kernel leaves unwritten shows up.

Where a non-finite or out-of-int-range coordinate is stopped (read before these cases were first run: no load, store or atomic
address is formed from an ungated conversion):
  * sample_setup / sample_setup_oob (msda_geom.h): the skip test `!(h > -1 && w > -1 && h < H && w < W)` comes BEFORE
    (int)floor; NaN fails it, +-inf and 1e10 px fail it; the sample returns with every corner offset -1 / kOob and zero
    fractions.  Everything below samples through these two: msda_fwd_generic / msda_bwd_generic (msda.hip), the strip and patch
    forward, msda_bwd_d32, the patch gather and lvl_scatter_body of the merged backward (msda_fast.h), the region scatter
    (msda_region.h: h0 / w0 stay 0 and the corner flags come from the offsets' signs), all four kernels of msda_h16.hip, and the
    far paths of the window kernels (publish in msda_rw.h, the far loop of msda_gw.h);
  * mask_corners_oob (msda_fast.h) converts floorf ungated, but only compares the result to turn offsets into kOob, and its byte
    path reads the mask only where `off[c] != kOob`, which a skipped sample never has;
  * the window forward (msda_rw.h) and the window gather (msda_gw.h) convert (int)h0f ungated into a window row, but the LDS
    address is that row only under `inwin`, which requires `inside` (the same skip test); every other sample reads the zero rows,
    and its record holds zeros (forward: zero weights; gather: zero fractions and attention), so 0 * NaN cannot arise; level 0's
    global corner offsets are kOob unless `inside`; the compact far record is written only under `inside && !inwin`;
  * buffer loads are bounds-checked against the image's slice: kOob reads as the op's zero padding.

Run with -s to see the worst err / bound of every result of every case (profiles/msda_lattice_bounds.txt keeps a run's).
"""
import numpy as np
import pytest

import msda_h16_cases as C16
import msda_h16_ref as H
import msda_lattice_cases as LC
import msda_ref64 as R
from test_gpu_msda_bounds import _geometry_note

pytestmark = pytest.mark.gpu

FP32_LATTICE = [n for n, s in LC.CASES.items() if s["kind"] == "lattice"]
FP32_NON_FINITE = [n for n, s in LC.CASES.items() if s["kind"] == "nonfinite"]
H16_LATTICE = [n for n, s in LC.H16_CASES.items() if s["kind"] == "lattice"]
H16_NON_FINITE = [n for n, s in LC.H16_CASES.items() if s["kind"] == "nonfinite"]


def _t(a, dtype=None):
    import torch
    t = torch.from_numpy(np.array(a, order="C")).cuda()      # (a contiguous copy: the cases' arrays are read-only, some are broadcast views)
    return t if dtype is None else t.to(H.torch_dtype(dtype))


def _poison(*specs):
    """(shape, torch dtype) ...: NaN-filled buffers of these sizes go back to the caching allocator, which hands them to the next
    allocations of the same sizes -- the results."""
    import torch
    junk = [torch.full(shape, float("nan"), dtype=dt, device="cuda") for shape, dt in specs for _ in range(2)]
    torch.cuda.synchronize()
    del junk


def _off_grid(t, modulus):
    import torch
    buf = torch.empty(t.numel() + 1, dtype=t.dtype, device=t.device)
    v = buf[1:].view(t.shape).copy_(t)
    assert v.data_ptr() % modulus != 0 and v.is_contiguous()
    return v


def _run(name, dtype=None):
    """One case through the compiled front end under its policy; routes asserted; every result against the reference built with
    the case's `exact` flag, and the exact-zero / finite assertions of the module docstring."""
    import torch
    import MultiScaleDeformableAttention as MSDA
    import semi_detr_amd as sda
    s, c = LC.ALL_CASES[name], LC.inputs(name, dtype)
    shp = c["shapes"]
    tsh = _t(shp)
    tls = torch.cat([tsh.new_zeros(1), (tsh[:, 0] * tsh[:, 1]).cumsum(0)[:-1]])
    sda._lib.set_forward_policy(s["policy"])
    last = (sda._lib.lib().semidetr_msda_h16_last_kernels if dtype else sda._lib.lib().semidetr_msda_last_kernels)
    np_dt = np.float64 if s["dtype"] == "f64" else np.float32
    t_res = H.torch_dtype(dtype) if dtype else (torch.float64 if s["dtype"] == "f64" else torch.float32)
    t_small = torch.float32 if dtype else t_res
    tv = _t(c["value"], dtype)
    if s["unaligned"]:
        tv = _off_grid(tv, 8 if dtype else 16)
    N, Lq, M, D, P, L = s["N"], c["gout"].shape[1], s["M"], s["D"], s["P"], len(shp)
    out_spec = ((N, Lq, M * D), t_res)
    grad_specs = [(tuple(tv.shape), t_res), ((N, Lq, M, L, P, 2), t_small), ((N, Lq, M, L, P), t_small)]
    if dtype:
        grad_specs.append((tuple(tv.shape), torch.float32))      # (the 16-bit backward accumulates grad_value in an fp32 workspace)
    routes = []
    if s["io"] == "fused":
        tm = _t(c["mask"]) if c["mask"] is not None else None
        args = (tv, tsh, tls, _t(c["ref"]), _t(c["off"]), _t(c["logits"]))
        _poison(out_spec)
        got = dict(out=MSDA.ms_deform_attn_fused_forward(*args, tm))
        routes.append(last().decode())
        if s["backward"]:
            g = _t(c["gout"])
            _poison(*grad_specs)
            got["grad_value"], got["grad_offsets"], got["grad_logits"] = MSDA.ms_deform_attn_fused_backward(*args, g, tm)
            routes.append(last().decode())
    else:
        fwd, bwd = ((MSDA.ms_deform_attn_h16_forward, MSDA.ms_deform_attn_h16_backward) if dtype
                    else (MSDA.ms_deform_attn_forward, MSDA.ms_deform_attn_backward))
        args = (tv, tsh, tls, _t(c["loc"]), _t(c["attn"]))
        _poison(out_spec)
        got = dict(out=fwd(*args, 64))
        routes.append(last().decode())
        if s["backward"]:
            g = _t(c["gout"], dtype)
            _poison(*grad_specs)
            got["grad_value"], got["grad_loc"], got["grad_attn"] = bwd(*args, g, 64)
            routes.append(last().decode())
    torch.cuda.synchronize()
    assert routes[0] == s["fwd"], (name, "forward", routes[0], s["fwd"])
    if s["backward"]:
        assert routes[1] == s["bwd"], (name, "backward", routes[1], s["bwd"])
    assert got["out"].dtype == t_res and tuple(got["out"].shape) == out_spec[0]
    got = {k: t.detach().float().cpu().numpy() if dtype else t.detach().cpu().numpy() for k, t in got.items()}

    # ---- no allowance: finite everywhere, zeros where nothing may arrive
    for k, a in got.items():
        assert np.isfinite(a).all(), (name, k, "not finite at", np.argwhere(~np.isfinite(a))[:4].tolist())
    skip, sure = LC.skipped(name, dtype)
    dead = sure.all((-1, -2))
    assert dead.any() and not got["out"].reshape(N, Lq, M, D)[dead].any(), "a row without a sample on the map must be exact zeros"
    if s["backward"]:
        for k in ("grad_attn", "grad_loc", "grad_offsets"):
            if k in got:
                bad = (got[k][sure] != 0)
                assert not bad.any(), (name, k, "a skipped sample has a gradient: sample", np.argwhere(sure)[np.argwhere(bad)[0, 0]].tolist())
        if c["mask"] is not None:
            assert not got["grad_value"][c["mask"]].any(), "padded pixels must receive exactly zero gradient"

    # ---- the bound, with delta = 0 on the exact samples
    ref = LC.reference(name, dtype)
    info = dict(c, D=D, P=P)
    if s["io"] == "fused":
        info["loc"] = np.nan_to_num(ref["prologue"]["loc"], nan=0.0, posinf=0.0, neginf=0.0)
    note = _geometry_note(info, shp)
    label = f"{name}{' ' + dtype if dtype else ''} [{' / '.join(routes)}]"
    if dtype:
        worst = {k: H.check(label, k, a, ref[k]) for k, a in got.items()}
    else:
        worst = {k: R.check(label, k, a, ref[k], np_dt, note) for k, a in got.items()}
    print(f"\n{label}: exact {c['exact'].mean():.3f} skipped {skip.mean():.3f}; worst err/bound " +
          ", ".join(f"{k} {v:.3f}" for k, v in worst.items()))


@pytest.fixture(autouse=True)
def _restore_policy():
    import semi_detr_amd as sda
    yield
    sda._lib.set_forward_policy("adaptive")


@pytest.mark.parametrize("name", FP32_LATTICE)
def test_lattice_case_within_bound(name):
    _run(name)


@pytest.mark.parametrize("dtype", C16.DTYPES)
@pytest.mark.parametrize("name", H16_LATTICE)
def test_h16_lattice_case_within_bound(name, dtype):
    _run(name, dtype)


@pytest.mark.parametrize("name", FP32_NON_FINITE)
def test_non_finite_locations_are_skipped(name):
    _run(name)


@pytest.mark.parametrize("dtype", C16.DTYPES)
@pytest.mark.parametrize("name", H16_NON_FINITE)
def test_h16_non_finite_locations_are_skipped(name, dtype):
    _run(name, dtype)
