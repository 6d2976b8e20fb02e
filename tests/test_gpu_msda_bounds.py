"""GPU: every MSDA kernel route of the product dispatcher against the fp64 reference with per-element fp32 error bounds
(tests/msda_ref64.py: |got - ref64| <= 2u n_e A_e + 2 C_e + tiny, derived there, no per-test factor).

The older parity tests compare with the fp32 oracle under absolute tolerances sized for positive, narrow inputs (value in
[0, 0.01), near-uniform attention), where a kernel that reads value as fp16 still passes.  Here the inputs are signed and spread
over five decades per head (value ~ N(0, 1) * 10^k, k in [-3, 2]), grad_out ~ N(0, 1), attention is a softmax of N(0, 2) logits,
some cases add a 10^{+-2} range between levels, samples spread 2 px, 9 px, anywhere, or partly off the map, and padded pixels hold
NaN.  Each case names the route it must take (semidetr_msda_last_kernels) for its forward and its backward; ROUTES maps every
product route to the cases that assert it, and tests/test_msda_ref64.py checks that map against the dispatcher's source.

Run with -s to see the worst err / bound of every result of every case.
"""
import math

import numpy as np
import pytest

import msda_ref64 as R

DINO = [(20, 27), (10, 14), (5, 7), (3, 4)]
PYR4 = [(37, 53), (19, 27), (10, 14), (5, 7)]
PYR5 = PYR4 + [(3, 4)]
LEVELS = [(100, 167), (50, 84), (25, 42), (13, 21)]                   # 800 x 1333 input, strides 8 .. 64
MIXED_IMG_SHAPES = [(800, 1333), (800, 1201), (750, 1333), (704, 1066)]   # the bench's padded batch (restated, see bench.py)

FWD_STRIP1, FWD_STRIP2, FWD_STRIP4 = "msda_fwd_d32<1, 4, 0", "msda_fwd_d32<2, 4, 0", "msda_fwd_d32<4, 4, 0"
FWD_PATCH, FWD_WINDOW, FWD_GENERIC = "msda_fwd_d32<1, 4, 408", "msda_rw_d32", "msda_fwd_generic"
BWD_D32_32, BWD_D32_8 = "fillBufferAligned+msda_bwd_d32<32", "fillBufferAligned+msda_bwd_d32<8"
BWD_MERGED = "fillBufferAligned+msda_bwd_lvl_merged_wide"
BWD_PATCH = "msda_bwd_gather_d32+msda_bwd_scatter_d32_reg"
BWD_PATCH_FILL = "fillBufferAligned+msda_bwd_gather_d32+msda_bwd_scatter_d32_reg"
BWD_WINDOW = "msda_gw_d32+msda_bwd_scatter_d32_reg"
BWD_GENERIC = "fillBufferAligned+msda_bwd_generic"


def _spec(levels, N, Lq=None, M=8, D=32, P=4, io="contract", ref_dim=2, mask=None, spread=2.0, level_range=False, policy="patch",
          dtype="f32", unaligned=False, fwd=None, bwd=None, seed=0, backward=True):
    return dict(levels=levels, N=N, Lq=Lq, M=M, D=D, P=P, io=io, ref_dim=ref_dim, mask=mask, spread=spread, level_range=level_range,
                policy=policy, dtype=dtype, unaligned=unaligned, fwd=fwd, bwd=bwd, seed=seed, backward=backward)


# spread: sigma in pixels of the level around the query's own pixel (encoder) / reference point; "anywhere": uniform on the map;
# "offmap": uniform on [-0.15, 1.15]^2 (some samples partly or wholly outside)
SMALL_CASES = {
    # decoder strips (query sets that are not the pixels): pick_split by (N, Lq, M); backward by N * Lq and the workgroup count
    "dec_strip1_merged": _spec(DINO, 4, Lq=2100, spread="offmap", fwd=FWD_STRIP1, bwd=BWD_MERGED, seed=1),
    "dec_strip2_merged": _spec(DINO, 4, Lq=1100, spread="anywhere", level_range=True, fwd=FWD_STRIP2, bwd=BWD_MERGED, seed=2),
    "dec_strip4_merged_ref4": _spec(DINO, 2, Lq=300, io="fused", ref_dim=4, spread=1.5, fwd=FWD_STRIP4, bwd=BWD_MERGED, seed=3),
    "dec_strip4_bwd8": _spec(DINO, 2, Lq=100, spread="offmap", fwd=FWD_STRIP4, bwd=BWD_D32_8, seed=4),
    "dec_strip2_bwd32": _spec(DINO, 32, Lq=15, M=32, spread="anywhere", fwd=FWD_STRIP2, bwd=BWD_D32_32, seed=5),
    "dec_fused_ref2_bwd8": _spec(DINO, 2, Lq=33, io="fused", spread=6.0, fwd=FWD_STRIP4, bwd=BWD_D32_8, seed=6),
    # encoder, patch kernel + patch gather (the gather clears grad_value for L * P = 16 and 20)
    "signed_dino": _spec(DINO, 2, spread=2.0, fwd=FWD_PATCH, bwd=BWD_PATCH, seed=7),
    "patch_fused_ref2": _spec(PYR4, 2, io="fused", spread=9.0, level_range=True, fwd=FWD_PATCH, bwd=BWD_PATCH, seed=8),
    "patch_fused_ref4": _spec(PYR4, 2, io="fused", ref_dim=4, spread=2.0, fwd=FWD_PATCH, bwd=BWD_PATCH, seed=9),
    "patch_fused_mask": _spec(PYR4, 3, io="fused", mask="band", spread=9.0, fwd=FWD_PATCH, bwd=BWD_PATCH, seed=10),
    "five_levels": _spec(PYR5, 2, spread="offmap", fwd=FWD_PATCH, bwd=BWD_PATCH, seed=11),
    # encoder, L * P neither 16 nor 20: separate fill; a level wider than 1423 px: the region scatter's one-by-one path
    "three_levels_fill": _spec(PYR4[:3], 2, spread=2.0, fwd=FWD_PATCH, bwd=BWD_PATCH_FILL, seed=12),
    "wide_level": _spec([(3, 1500), (2, 750)], 1, M=4, spread=9.0, fwd=FWD_PATCH, bwd=BWD_PATCH_FILL, seed=13),
    # encoder, region-window forward + lane-per-sample window gather
    "window4_contract": _spec(PYR4, 2, spread=2.0, policy="window", level_range=True, fwd=FWD_WINDOW, bwd=BWD_WINDOW, seed=14),
    "window4_fused": _spec(PYR4, 2, io="fused", spread=9.0, policy="window", fwd=FWD_WINDOW, bwd=BWD_WINDOW, seed=15),
    "window4_mask_band": _spec(PYR4, 3, io="fused", mask="band", spread=2.0, policy="window", fwd=FWD_WINDOW, bwd=BWD_WINDOW, seed=16),
    "window4_mask_holes": _spec(PYR4, 3, io="fused", mask="band_with_holes", spread=9.0, policy="window", fwd=FWD_WINDOW,
                                bwd=BWD_WINDOW, seed=17),
    "window4_mask_random": _spec(PYR4, 3, io="fused", mask="random", spread="anywhere", policy="window", fwd=FWD_WINDOW,
                                 bwd=BWD_WINDOW, seed=18),
    "boxes_window": _spec(PYR4, 2, io="fused", ref_dim=4, spread=2.0, policy="window", fwd=FWD_WINDOW, bwd=BWD_WINDOW, seed=19),
    "boxes_window_mask": _spec(PYR4, 2, io="fused", ref_dim=4, mask="band", spread=9.0, policy="window", fwd=FWD_WINDOW,
                               bwd=BWD_WINDOW, seed=20),
    "window5_contract": _spec(PYR5, 2, spread=9.0, policy="window", fwd=FWD_WINDOW, bwd=BWD_WINDOW, seed=21),
    "window5_fused": _spec(PYR5, 2, io="fused", spread=2.0, level_range=True, policy="window", fwd=FWD_WINDOW, bwd=BWD_WINDOW, seed=22),
    "window5_mask": _spec(PYR5, 3, io="fused", mask="random", spread=2.0, policy="window", fwd=FWD_WINDOW, bwd=BWD_WINDOW, seed=23),
    "boxes_window5": _spec(PYR5, 2, io="fused", ref_dim=4, spread="offmap", policy="window", fwd=FWD_WINDOW, bwd=BWD_WINDOW, seed=24),
    # generic kernels: channels != 32, a value pointer off the 16-byte grid, more heads than the fast path takes, fp64
    "generic_d16": _spec(DINO, 2, Lq=50, D=16, spread="offmap", fwd=FWD_GENERIC, bwd=BWD_GENERIC, seed=25),
    "generic_d64": _spec(DINO, 2, Lq=50, D=64, spread="anywhere", fwd=FWD_GENERIC, bwd=BWD_GENERIC, seed=26),
    "generic_unaligned": _spec(DINO, 2, Lq=70, unaligned=True, spread=3.0, fwd=FWD_GENERIC, bwd=BWD_GENERIC, seed=27),
    "generic_m33": _spec(DINO, 1, Lq=40, M=33, spread="offmap", fwd=FWD_GENERIC, bwd=BWD_GENERIC, seed=28),
    "generic_f64": _spec(DINO, 2, Lq=60, dtype="f64", spread="offmap", level_range=True, fwd=FWD_GENERIC, bwd=BWD_GENERIC, seed=29),
}

FULL_CASES = {
    # bench.py's encoder call: bs 4, fused prologue + padding mask of four differently sized images, valid-ratio reference points
    "bench_encoder_bs4": _spec(LEVELS, 4, io="fused", mask="mixed", spread=2.0, policy="window", fwd=FWD_WINDOW, bwd=BWD_WINDOW,
                               seed=31),
    # the COCO-Full pyramid at full size through the patch kernels (20 samples per row)
    "five_levels_full": _spec(LEVELS + [(7, 11)], 2, spread=2.0, policy="patch", fwd=FWD_PATCH, bwd=BWD_PATCH, seed=32),
    # one image: the window forward's tail split
    "window_tail_split_bs1": _spec(LEVELS, 1, io="fused", spread=2.0, policy="window", fwd=FWD_WINDOW, seed=33, backward=False),
}

ROUTES = {}
for _name, _s in list(SMALL_CASES.items()) + list(FULL_CASES.items()):
    ROUTES.setdefault(_s["fwd"], []).append(_name)
    if _s["backward"]:
        ROUTES.setdefault(_s["bwd"], []).append(_name)


def _pixel_centres(levels):
    return np.concatenate([np.stack(np.meshgrid((np.arange(w) + 0.5) / w, (np.arange(h) + 0.5) / h), -1).reshape(-1, 2)
                           for h, w in levels])


def _band_mask(shp, fracs):
    rows = []
    for fh, fw in fracs:
        per = []
        for h, w in shp:
            mk = np.zeros((int(h), int(w)), bool)
            mk[int(np.ceil(fh * h)):, :] = True
            mk[:, int(np.ceil(fw * w)):] = True
            per.append(mk.reshape(-1))
        rows.append(np.concatenate(per))
    return np.stack(rows)


def _mixed_geometry(levels, n):
    """bench.py Workload.geometry restated: padding mask (n, S) of MIXED_IMG_SHAPES[:n] on the 800 x 1333 canvas, valid ratios, and
    the encoder's reference points = pixel centre / valid extent x valid ratio (transformer.py:675-691)."""
    mks, vrs = [], []
    for h, w in levels:
        mk = np.ones((n, h, w), bool)
        for i, (ih, iw) in enumerate(MIXED_IMG_SHAPES[:n]):
            mk[i, :math.ceil(ih * h / 800), :math.ceil(iw * w / 1333)] = False
        mks.append(mk.reshape(n, -1))
        vrs.append(np.stack([(~mk[:, 0, :]).sum(1) / w, (~mk[:, :, 0]).sum(1) / h], -1).astype(np.float32))
    vr = np.stack(vrs, 1)                                                        # (n, L, 2) [w, h]
    refs = []
    for lvl, (h, w) in enumerate(levels):
        ry, rx = np.meshgrid(np.arange(h, dtype=np.float32) + 0.5, np.arange(w, dtype=np.float32) + 0.5, indexing="ij")
        refs.append(np.stack((rx.reshape(-1)[None] / (vr[:, None, lvl, 0] * w), ry.reshape(-1)[None] / (vr[:, None, lvl, 1] * h)), -1))
    ref = np.concatenate(refs, 1)[:, :, None] * vr[:, None]
    return np.concatenate(mks, 1), ref.astype(np.float32)


def make_case(s):
    """Inputs of a case spec (numpy, deterministic): dict(value, shapes, gout, mask, and loc / attn (contract) or ref / off / logits
    (fused)).  Padded pixels of value hold NaN."""
    rng = np.random.default_rng(1000 + s["seed"])
    levels, N, M, D, P = s["levels"], s["N"], s["M"], s["D"], s["P"]
    shp = np.asarray(levels, np.int64)
    L = len(levels)
    S = int((shp[:, 0] * shp[:, 1]).sum())
    encoder = s["Lq"] is None
    Lq = S if encoder else s["Lq"]
    ft = np.float64 if s["dtype"] == "f64" else np.float32
    head_scale = 10.0 ** np.linspace(-3, 2, M)
    value = rng.standard_normal((N, S, M, D)) * head_scale[None, None, :, None]
    if s["level_range"]:
        lv = 10.0 ** np.array([2, -2, 1, -1, 0, 0][:L], np.float64)
        value *= np.repeat(lv, shp[:, 0] * shp[:, 1])[None, :, None, None]
    logits = rng.standard_normal((N, Lq, M, L * P)) * 2
    gout = rng.standard_normal((N, Lq, M * D))
    wh = shp[:, ::-1].astype(np.float64)                                        # (W, H) per level
    mask = None
    if s["mask"] == "mixed":
        mask, ref2 = _mixed_geometry(levels, N)
    else:
        ref2 = (np.broadcast_to(_pixel_centres(levels)[None, :, None, :], (N, S, L, 2)) if encoder
                else rng.random((N, Lq, L, 2)))
    if s["mask"] in ("band", "band_with_holes"):
        mask = _band_mask(shp, [(1.0, 1.0), (0.8, 0.55), (0.47, 0.93)][:N])
        if s["mask"] == "band_with_holes":
            st = np.concatenate([[0], np.cumsum(shp[:, 0] * shp[:, 1])])
            mask[1, st[1] + 3] = True
            mask[1, st[L] - 1] = False
    elif s["mask"] == "random":
        mask = rng.random((N, S)) < 0.15
    sp = s["spread"]
    if sp == "anywhere":
        loc = rng.random((N, Lq, M, L, P, 2))
    elif sp == "offmap":
        loc = rng.random((N, Lq, M, L, P, 2)) * 1.3 - 0.15
    else:
        loc = None
    c = dict(shapes=shp, mask=mask, value=None, gout=gout.astype(ft), ref=None)
    if s["io"] == "fused":
        if s["ref_dim"] == 4:
            ref = np.concatenate([np.asarray(ref2, np.float64), rng.random(ref2.shape[:-1] + (2,)) * 0.2 + 0.02], -1)
        else:
            ref = np.asarray(ref2, np.float64)
        if loc is not None:                                                     # offsets that land on the given locations
            scale = (1.0 / wh)[None, None, None, :, None, :] if s["ref_dim"] == 2 else ref[:, :, None, :, None, 2:] * 0.5 / P
            off = (loc - ref[:, :, None, :, None, :2]) / scale
        else:
            px = rng.standard_normal((N, Lq, M, L, P, 2)) * sp                  # sigma in pixels of the level
            off = px if s["ref_dim"] == 2 else px / wh[None, None, None, :, None, :] / (ref[:, :, None, :, None, 2:] * 0.5 / P)
        c.update(ref=ref.astype(np.float32), off=off.astype(np.float32), logits=logits.astype(np.float32))
    else:
        if loc is None:
            loc = np.asarray(ref2, np.float64)[:, :, None, :, None, :] + \
                rng.standard_normal((N, Lq, M, L, P, 2)) * sp / wh[None, None, None, :, None, :]
        a = np.exp(logits - logits.max(-1, keepdims=True))
        a = (a / a.sum(-1, keepdims=True)).reshape(N, Lq, M, L, P)
        c.update(loc=loc.astype(ft), attn=a.astype(ft))
    if mask is not None:
        value[mask] = np.nan
    c["value"] = value.astype(ft)
    return c


# ---------------------------------------------------------------------------------------------------------------------------- GPU

def _t(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _last():
    import semi_detr_amd as sda
    return sda._lib.lib().semidetr_msda_last_kernels().decode()


def _geometry_note(c, shp):
    """-> geometry(what, idx) for msda_ref64.check: the samples behind a failing element."""
    def note(what, idx):
        if what == "grad_value":
            n, s, m = idx[:3]
            st = np.concatenate([[0], np.cumsum(shp[:, 0] * shp[:, 1])])
            lvl = int(np.searchsorted(st, s, side="right") - 1)
            W = int(shp[lvl, 1])
            return f"value row: image {n} level {lvl} pixel (y {(s - st[lvl]) // W}, x {(s - st[lvl]) % W}) head {m}"
        if what == "grad_logits":
            idx = tuple(idx[:3]) + divmod(int(idx[3]), c["P"])
        x, y = R.pixel_coords(c["loc"][idx[0], idx[1], idx[2] if what != "out" else idx[2] // c["D"]], shp)
        if what == "out":
            return "samples of the row (x, y px per level): " + "; ".join(
                f"L{lv}: " + ", ".join(f"({a:.3f}, {b:.3f})" for a, b in zip(x[lv], y[lv])) for lv in range(len(shp)))
        return f"sample level {idx[3]} point {idx[4]}: x {x[idx[3], idx[4]]:.5f} px, y {y[idx[3], idx[4]]:.5f} px"
    return note


def run_case(name, s):
    """Kernels of one case under its policy, every result against ref64; returns {result: worst err / bound}."""
    import torch
    import MultiScaleDeformableAttention as MSDA
    import semi_detr_amd as sda
    c = make_case(s)
    shp = c["shapes"]
    tsh = _t(shp)
    tls = torch.cat([tsh.new_zeros(1), (tsh[:, 0] * tsh[:, 1]).cumsum(0)[:-1]])
    sda._lib.set_forward_policy(s["policy"])
    dt = np.float64 if s["dtype"] == "f64" else np.float32
    tv = _t(c["value"])
    if s["unaligned"]:
        buf = torch.empty(tv.numel() + 1, dtype=tv.dtype, device=tv.device)
        tv = buf[1:].view(tv.shape).copy_(tv)
        assert tv.data_ptr() % 16 != 0
    worst = {}
    routes = []
    if s["io"] == "fused":
        tm = _t(c["mask"]) if c["mask"] is not None else None
        args = (tv, tsh, tls, _t(c["ref"]), _t(c["off"]), _t(c["logits"]))
        out = MSDA.ms_deform_attn_fused_forward(*args, tm)
        routes.append(_last())
        if s["backward"]:
            gv, goff, glog = MSDA.ms_deform_attn_fused_backward(*args, _t(c["gout"]), tm)
            routes.append(_last())
        torch.cuda.synchronize()
        ref = R.fused(c["value"], shp, c["ref"], c["off"], c["logits"], c["gout"] if s["backward"] else None, mask=c["mask"])
        c["loc"] = ref["prologue"]["loc"]
        got = dict(out=out)
        if s["backward"]:
            got.update(grad_value=gv, grad_offsets=goff, grad_logits=glog)
    else:
        args = (tv, tsh, tls, _t(c["loc"]), _t(c["attn"]))
        out = MSDA.ms_deform_attn_forward(*args, 64)
        routes.append(_last())
        if s["backward"]:
            gv, gl, ga = MSDA.ms_deform_attn_backward(*args, _t(c["gout"]), 64)
            routes.append(_last())
        torch.cuda.synchronize()
        ref = R.msda(c["value"], shp, c["loc"], c["attn"], c["gout"] if s["backward"] else None)
        got = dict(out=out)
        if s["backward"]:
            got.update(grad_value=gv, grad_loc=gl, grad_attn=ga)
    assert routes[0] == s["fwd"], (name, "forward", routes[0], s["fwd"])
    if s["backward"]:
        assert routes[1] == s["bwd"], (name, "backward", routes[1], s["bwd"])
    if s["mask"] is not None and s["backward"]:
        assert np.all(got["grad_value"].cpu().numpy()[c["mask"]] == 0.0), "padded pixels must receive exactly zero gradient"
    c["D"], c["P"] = s["D"], s["P"]
    note = _geometry_note(c, shp)
    for what, t in got.items():
        worst[what] = R.check(f"{name} [{' / '.join(routes)}]", what, t.detach().cpu().numpy(), ref[what], dt, note)
    # the median bound of the main results, to set against the old absolute tolerances
    med = {k: float(np.median(ref[k].bound(dt))) for k in got}
    print(f"\n{name}: routes {routes}; worst err/bound " + ", ".join(f"{k} {v:.3f}" for k, v in worst.items()) +
          "; median bound " + ", ".join(f"{k} {v:.3g}" for k, v in med.items()))
    return worst


@pytest.fixture(autouse=True)
def _restore_policy():
    import semi_detr_amd as sda
    yield
    sda._lib.set_forward_policy("adaptive")


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(SMALL_CASES))
def test_small_case_within_bound(name):
    run_case(name, SMALL_CASES[name])


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(FULL_CASES))
def test_full_size_case_within_bound(name):
    run_case(name, FULL_CASES[name])
