"""GPU: the run-time region grid of the three encoder window kernels (msda_rw_d32 forward, msda_gw_d32 gather,
msda_bwd_scatter_d32_reg scatter; csrc/msda_grid.h region_grid_choice) against the fp64 reference with its per-element bounds
(tests/msda_ref64.py).  Every grid a launch may be given -- the coarsest, uneven tiles, one-row regions, regions without a level-0
pixel -- must produce every query exactly once: the kernels run through the C ABI into buffers filled with NaN beforehand, so a query
no region took stays NaN, and a query two regions of the scatter took doubles its grad_value rows and leaves the bound.  (The forward
and the gather STORE their results: a query produced twice there stores the same words twice; that every pixel has one region is
what tests/test_region_grid_host.py shows for the map itself.)

Bit-identity of the `_v2` entry points without a host table (grid 0 / 0) with the entry points they extend: out, grad_sampling_loc
and grad_attn_weight (resp. the fused gradients) are compared bit for bit; grad_value is accumulated with fp32 atomics whose order
differs from run to run in either entry point (include/semidetr_hip.h), so it is compared within the reference's bound, twice."""
import ctypes

import numpy as np
import pytest
import torch

import msda_ref64 as R
import semi_detr_amd as sda
from test_gpu_msda_bounds import _spec, make_case
from test_region_grid_host import KERNELS, SMALL4, SMALL5, pinned_grids

pytestmark = pytest.mark.gpu

M, D, P = 2, 32, 4
PIXELS, GATHER_WINDOW = 1, 1 << 16          # SEMIDETR_MSDA_QUERIES_ARE_PIXELS, SEMIDETR_MSDA_GATHER_WINDOW
FWD, BWD = "msda_rw_d32", "msda_gw_d32+msda_bwd_scatter_d32_reg"


@pytest.fixture(autouse=True)
def _window_kernels_unpinned():
    sda._lib.set_forward_policy("window")
    yield
    sda._lib.set_forward_policy("adaptive")
    for k in KERNELS:
        sda._lib.set_region_grid(k, 0, 0)


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _nan(*shape):
    return torch.full(shape, float("nan"), dtype=torch.float32, device="cuda")


def _last():
    return sda._lib.lib().semidetr_msda_last_kernels().decode()


_CASES = {}


def _case(levels, N, io, sigma):
    """inputs (device tensors) and the fp64 reference of one case, built once and left unchanged"""
    key = (len(levels), N, io, sigma)
    if key in _CASES:
        return _CASES[key]
    mask_kind = {"contract": None, "fused_band": "band", "fused_hole": "band"}[io]
    c = make_case(_spec(levels, N, M=M, io="contract" if io == "contract" else "fused", mask=mask_kind, spread=sigma,
                        policy="window", seed=40 + len(_CASES)))
    shp = c["shapes"]
    if io == "fused_hole":      # one padded pixel inside the last image's valid area, one valid pixel at its padded end: the bytes decide
        st = np.concatenate([[0], np.cumsum(shp[:, 0] * shp[:, 1])])
        rng = np.random.default_rng(7)
        for pix, padded in ((int(st[1]) + 3, True), (int(st[-1]) - 1, False)):
            c["mask"][N - 1, pix] = padded
            c["value"][N - 1, pix] = np.nan if padded else rng.standard_normal((M, D)).astype(np.float32)
    S = int((shp[:, 0] * shp[:, 1]).sum())
    t = dict(N=N, S=S, L=len(levels), shp=shp, io=io, host=(ctypes.c_int64 * (2 * len(levels)))(*[int(v) for v in shp.reshape(-1)]),
             value=_dev(c["value"]), shapes=_dev(shp), gout=_dev(c["gout"]), mask=None, ext=None, np_mask=c["mask"])
    t["starts"] = torch.cat([t["shapes"].new_zeros(1), (t["shapes"][:, 0] * t["shapes"][:, 1]).cumsum(0)[:-1]])
    if io == "contract":
        t.update(loc=_dev(c["loc"]), attn=_dev(c["attn"]))
        t["ref64"] = R.msda(c["value"], shp, c["loc"], c["attn"], c["gout"])
        t["small"] = ("grad_loc", "grad_attn")
    else:
        t.update(ref=_dev(c["ref"]), off=_dev(c["off"]), logits=_dev(c["logits"]), mask=_dev(c["mask"].astype(np.uint8)))
        t["ext"] = torch.empty(N, len(levels), dtype=torch.int32, device="cuda")
        sda._lib.call("semidetr_msda_mask_extents", t["value"].device, t["mask"], t["shapes"], t["starts"], N, S, len(levels), t["ext"])
        t["ref64"] = R.fused(c["value"], shp, c["ref"], c["off"], c["logits"], c["gout"], mask=c["mask"])
        t["small"] = ("grad_offsets", "grad_logits")
    _CASES[key] = t
    return t


def _run(t, host, v2=True):
    """forward + backward of a case through the C ABI into NaN-filled buffers -> {result: tensor}; host: the host level table or None"""
    N, S, L = t["N"], t["S"], t["L"]
    dev = t["value"].device
    out, gv = _nan(N, S, M * D), _nan(N, S, M, D)
    dims = (N, S, M, D, L, S, P)
    tail = (host,) if v2 else ()
    sfx = "_v2" if v2 else ""
    if t["io"] == "contract":
        ga, gb = _nan(N, S, M, L, P, 2), _nan(N, S, M, L, P)
        sda._lib.call("semidetr_msda_forward_f32" + sfx, dev, t["value"], t["shapes"], t["starts"], t["loc"], t["attn"], *dims, PIXELS, out,
                      *tail)
        assert _last() == FWD, _last()
        sda._lib.call("semidetr_msda_backward_f32" + sfx, dev, t["gout"], t["value"], t["shapes"], t["starts"], t["loc"], t["attn"], *dims,
                      PIXELS | GATHER_WINDOW, gv, ga, gb, *tail)
    else:
        ga, gb = _nan(N, S, M, L, P, 2), _nan(N, S, M, L * P)
        fused = (t["ref"], 2, t["off"], t["logits"], t["mask"], t["ext"])
        sda._lib.call("semidetr_msda_fused_forward_f32" + sfx, dev, t["value"], t["shapes"], t["starts"], *fused, *dims, PIXELS, out, *tail)
        assert _last() == FWD, _last()
        sda._lib.call("semidetr_msda_fused_backward_f32" + sfx, dev, t["gout"], t["value"], t["shapes"], t["starts"], *fused, *dims,
                      PIXELS | GATHER_WINDOW, gv, ga, gb, *tail)
    assert _last() == BWD, _last()
    torch.cuda.synchronize()
    return dict(zip(("out", "grad_value") + t["small"], (out, gv, ga, gb)))


def _check(t, got, what):
    worst = {}
    for name, ten in got.items():
        a = ten.cpu().numpy()
        assert np.isfinite(a).all(), f"{what}: {name} has {int((~np.isfinite(a)).sum())} elements no region produced"
        worst[name] = R.check(what, name, a, t["ref64"][name])
    if t["np_mask"] is not None:
        assert np.all(got["grad_value"].cpu().numpy()[t["np_mask"]] == 0.0), f"{what}: padded pixels must receive exactly zero gradient"
    print(f"\n{what}: worst err / bound " + ", ".join(f"{k} {v:.3f}" for k, v in worst.items()))


@pytest.mark.parametrize("sigma", [1.0, 6.0], ids=["sigma1", "sigma6"])
@pytest.mark.parametrize("io", ["contract", "fused_band", "fused_hole"])
@pytest.mark.parametrize("N", [1, 2])
@pytest.mark.parametrize("levels", [SMALL4, SMALL5], ids=["four_levels", "five_levels"])
def test_pinned_grids_produce_every_query_once_within_the_bounds(levels, N, io, sigma):
    t = _case(levels, N, io, sigma)
    grids = {k: pinned_grids(k, levels) for k in KERNELS}
    for name in grids["forward"]:
        for k in KERNELS:
            sda._lib.set_region_grid(k, *grids[k][name])
        for host in (t["host"], None):          # exact grid size from the host table / the size hint, regions taken in strides
            _check(t, _run(t, host), f"{name} {'with' if host is not None else 'without'} host table")
    for k in KERNELS:
        sda._lib.set_region_grid(k, 0, 0)
    _check(t, _run(t, t["host"]), "chosen grids")


@pytest.mark.parametrize("io", ["contract", "fused_band", "fused_hole"])
@pytest.mark.parametrize("levels", [SMALL4, SMALL5], ids=["four_levels", "five_levels"])
def test_no_table_and_no_pin_is_the_old_entry_point_bit_for_bit(levels, io):
    t = _case(levels, 2, io, 1.0)
    old, new = _run(t, None, v2=False), _run(t, None)
    for name in ("out",) + t["small"]:
        assert torch.equal(old[name].view(torch.int32), new[name].view(torch.int32)), name
    _check(t, dict(grad_value=old["grad_value"]), "old entry points")
    _check(t, dict(grad_value=new["grad_value"]), "v2 entry points without a table")
