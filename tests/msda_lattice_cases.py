"""Cases that put MSDA samples exactly on the pixel lattice, on the map's skip edges and at non-finite locations, shared by
tests/test_msda_lattice_ref.py (CPU) and tests/test_gpu_msda_lattice.py (GPU).

The bounded cases of test_gpu_msda_bounds draw continuous locations, which never hit a pixel-centre line, and msda_ref64 leaves
grad_loc unjudged within 2 delta of one.  Here about half of the samples of a case sit where their fp32 pixel coordinate
x = fl(fl(lx * W) - 0.5) carries no rounding at all, and the reference is built with msda_ref64's `exact` flag for them (delta 0,
no kink exclusion, no edge allowance): floor's cell, the strict skip test and zero padding are then judged like any other number.

Exactness.  With a level extent E = 2^a * odd, the normalised coordinate l = j / 2^b is a dyadic number of a few bits, l * E is
one too, and so is l * E - 0.5: neither operation rounds, fused or not.  x = l * E - 0.5 is an integer (a lattice hit) exactly for
b = a + 1 and j odd, x = (j * odd - 1) / 2 -- every pixel on a power-of-two extent, every `odd`-th one otherwise; b = a + 3
gives off-lattice positions k / 8 * odd - 0.5.  _axis_tables() lists both; test_msda_lattice_ref.py checks every flagged sample
bit for bit.  Pyramids: POW2 (and POW2_5, L * P = 20), whose tables hold x = -1, 0, E - 1 and E; ODD (24 x 40 and halves), with
interior lattice hits on extents that are no powers of two and region edges that do not coincide with level edges; THIN, a
one-pixel-high and a one-pixel-wide level.

Sample kinds (KINDS, per sample; fused cases: per (image, query, level) reference point).  About half stay the ordinary
continuous samples of make_case(), so exact samples share rows and workgroups with the normal path.  The others: lattice in x
only / y only (the other coordinate dyadic, off the lattice) / both; one coordinate exactly on a skip edge (x = -1, x = W, y = -1,
y = H); on the first or last row / column (masked images: the last valid one, whose weight-0 partner is a NaN-filled padded
pixel, and the first padded one); normalised 0.0 and 1.0; lattice indices up to 3 px outside the map.  Encoder cases aim at
round(the query's pixel mapped to the level) + an integer offset within +-3 px (+-E / 2 on extents below 6; inside the
window kernels' LDS windows) or, on extents >= 32, of 12 .. 16 px (the far / compact-record path).  One row in a hundred has
nothing but skipped samples.

Fused cases.  The kernel forms loc = ref + off * rcp(W) itself, and whether v_rcp_f32 is exact on powers of two is unmeasured:
a fused sample is exact only where its offset is +-0 and its reference point comes from the tables (encoder: pixel centres of
the level; decoder: dyadic points, boxes with dyadic sizes).  The reference points are given per level, as the module's valid-
ratio scaling gives them.  The other half of the offsets is continuous; a few (INTEGER_OFFSET_SHARE) are whole pixels, judged
as ordinary samples (so the kink exclusion takes them: they must stay few).

Masked cases use band masks with valid extents 24 x 40 of 32 x 64 and its halves (_band_mask fractions 0.75 / 0.625); image 0
stays unmasked.  Padded pixels hold NaN.

Non-finite kind (the nf_* cases, of their own so that a failure names its cause): make_case()'s continuous samples, 5 % of which
have one coordinate (fused: one offset) replaced by NaN, +-inf, +-3e38 (overflows in loc * W) or +-1e10 (finite, beyond int32
after floor), and one row in a hundred wholly so.  Logits, attention, value and grad_out stay finite.
"""
import functools

import numpy as np

import msda_h16_cases as C16
import msda_h16_ref as H
import msda_ref64 as R
from test_gpu_msda_bounds import (BWD_D32_8, BWD_D32_32, BWD_GENERIC, BWD_MERGED, BWD_PATCH, BWD_PATCH_FILL, BWD_WINDOW, FWD_GENERIC,
                                  FWD_PATCH, FWD_STRIP1, FWD_STRIP2, FWD_STRIP4, FWD_WINDOW, _band_mask, _spec, make_case)

POW2 = [(32, 64), (16, 32), (8, 16), (4, 8)]
POW2_5 = POW2 + [(2, 4)]
ODD = [(24, 40), (12, 20), (6, 10), (3, 5)]
THIN = [(1, 8), (4, 1)]
MASK_FRACS = [(1.0, 1.0), (0.75, 0.625)]

# sample kinds: (name, share among the exact samples); the roles of the two coordinates are in _roles()
KINDS = (("lat_x", 0.14), ("lat_y", 0.14), ("lat_xy", 0.26), ("edge", 0.20), ("border", 0.16), ("zero_one", 0.06), ("outside", 0.04))
EXACT_SHARE = 0.5              # of the samples (fused: of the offsets that are +-0)
FAR_SHARE = 0.3                # encoder: of the integer offsets, on extents >= 32
ALL_SKIPPED_ROWS = 0.01
INTEGER_OFFSET_SHARE = 5e-4    # fused: whole-pixel offsets among the ordinary samples
NON_FINITE = (np.nan, np.inf, -np.inf, 3e38, -3e38, 1e10, -1e10)
NON_FINITE_SHARE = 0.05


def _lat(levels, N, kind="lattice", **kw):
    s = _spec(levels, N, **kw)
    s["kind"] = kind
    return s


CASES = {
    # decoder strips and the three query-set backwards
    "dec_strip1_merged": _lat(POW2, 4, Lq=2100, spread="offmap", fwd=FWD_STRIP1, bwd=BWD_MERGED, seed=201),
    "dec_strip2_merged_odd": _lat(ODD, 4, Lq=1100, spread="anywhere", level_range=True, fwd=FWD_STRIP2, bwd=BWD_MERGED, seed=202),
    "dec_strip4_merged_ref4": _lat(POW2, 2, Lq=300, io="fused", ref_dim=4, spread=1.5, fwd=FWD_STRIP4, bwd=BWD_MERGED, seed=203),
    "dec_strip4_bwd8_odd": _lat(ODD, 2, Lq=100, spread="offmap", fwd=FWD_STRIP4, bwd=BWD_D32_8, seed=204),
    "dec_strip2_bwd32": _lat(POW2_5[1:], 32, Lq=15, M=32, spread="anywhere", fwd=FWD_STRIP2, bwd=BWD_D32_32, seed=205),
    "dec_fused_ref2_bwd8": _lat(POW2, 2, Lq=33, io="fused", spread=6.0, fwd=FWD_STRIP4, bwd=BWD_D32_8, seed=206),
    "dec_thin": _lat(THIN, 2, Lq=40, spread="offmap", fwd=FWD_STRIP4, bwd=BWD_D32_8, seed=207),
    # encoder, patch kernel + patch gather, with (L * P neither 16 nor 20) and without the separate fill
    "patch_contract": _lat(POW2, 2, spread=2.0, fwd=FWD_PATCH, bwd=BWD_PATCH, seed=208),
    "patch_contract_odd": _lat(ODD, 2, spread=2.0, level_range=True, fwd=FWD_PATCH, bwd=BWD_PATCH, seed=209),
    "patch_fused_mask": _lat(POW2, 2, io="fused", mask="lattice_band", spread=3.0, fwd=FWD_PATCH, bwd=BWD_PATCH, seed=210),
    "patch_five_levels": _lat(POW2_5, 2, spread=2.0, fwd=FWD_PATCH, bwd=BWD_PATCH, seed=211),
    "patch_three_levels_fill": _lat(POW2[:3], 2, spread=2.0, fwd=FWD_PATCH, bwd=BWD_PATCH_FILL, seed=212),
    "patch_thin_fill": _lat(THIN, 2, spread=0.5, fwd=FWD_PATCH, bwd=BWD_PATCH_FILL, seed=213),
    # encoder, region-window forward + window gather: four and five levels, contract and fused, points and boxes, masked or not
    "window4_contract": _lat(POW2, 2, spread=2.0, policy="window", level_range=True, fwd=FWD_WINDOW, bwd=BWD_WINDOW, seed=214),
    "window4_contract_odd": _lat(ODD, 2, spread=2.0, policy="window", fwd=FWD_WINDOW, bwd=BWD_WINDOW, seed=215),
    "window4_fused": _lat(POW2, 2, io="fused", spread=3.0, policy="window", fwd=FWD_WINDOW, bwd=BWD_WINDOW, seed=216),
    "window4_fused_mask": _lat(POW2, 2, io="fused", mask="lattice_band", spread=2.0, policy="window", fwd=FWD_WINDOW, bwd=BWD_WINDOW,
                               seed=217),
    "window4_boxes": _lat(POW2, 2, io="fused", ref_dim=4, spread=2.0, policy="window", fwd=FWD_WINDOW, bwd=BWD_WINDOW, seed=218),
    "window4_boxes_mask": _lat(POW2, 2, io="fused", ref_dim=4, mask="lattice_band", spread=3.0, policy="window", fwd=FWD_WINDOW,
                               bwd=BWD_WINDOW, seed=219),
    "window5_contract": _lat(POW2_5, 2, spread=3.0, policy="window", fwd=FWD_WINDOW, bwd=BWD_WINDOW, seed=220),
    "window5_fused": _lat(POW2_5, 2, io="fused", spread=2.0, level_range=True, policy="window", fwd=FWD_WINDOW, bwd=BWD_WINDOW, seed=221),
    "window5_fused_mask": _lat(POW2_5, 2, io="fused", mask="lattice_band", spread=2.0, policy="window", fwd=FWD_WINDOW, bwd=BWD_WINDOW,
                               seed=222),
    "window5_boxes": _lat(POW2_5, 2, io="fused", ref_dim=4, spread=2.0, policy="window", fwd=FWD_WINDOW, bwd=BWD_WINDOW, seed=223),
    # generic kernels
    "generic_d16": _lat(POW2, 2, Lq=50, D=16, spread="offmap", fwd=FWD_GENERIC, bwd=BWD_GENERIC, seed=224),
    "generic_m33_odd": _lat(ODD, 1, Lq=40, M=33, spread="offmap", fwd=FWD_GENERIC, bwd=BWD_GENERIC, seed=225),
    "generic_unaligned": _lat(POW2, 2, Lq=70, unaligned=True, spread=3.0, fwd=FWD_GENERIC, bwd=BWD_GENERIC, seed=226),
    "generic_f64": _lat(POW2, 2, Lq=60, dtype="f64", spread="offmap", level_range=True, fwd=FWD_GENERIC, bwd=BWD_GENERIC, seed=227),
    # non-finite locations / offsets
    "nf_dec_strip": _lat(POW2, 2, Lq=100, kind="nonfinite", spread="offmap", fwd=FWD_STRIP4, bwd=BWD_D32_8, seed=231),
    "nf_patch": _lat(POW2, 2, kind="nonfinite", spread=2.0, fwd=FWD_PATCH, bwd=BWD_PATCH, seed=232),
    "nf_window_fused_mask": _lat(POW2, 2, kind="nonfinite", io="fused", mask="lattice_band", spread=2.0, policy="window",
                                 fwd=FWD_WINDOW, bwd=BWD_WINDOW, seed=233),
    "nf_generic_d16": _lat(POW2, 2, Lq=50, D=16, kind="nonfinite", spread="offmap", fwd=FWD_GENERIC, bwd=BWD_GENERIC, seed=234),
}

# the 16-bit op (fp32 locations and weights: the reference contract only); both types run every case
H16_CASES = {
    "h16_dec": _lat(POW2, 2, Lq=100, spread="offmap", fwd=C16.FWD4, bwd=C16.BWD, seed=241),
    "h16_dec_tail_m3_odd": _lat(ODD, 1, Lq=33, M=3, spread="offmap", fwd=C16.FWD4, bwd=C16.BWD, seed=242),
    "h16_enc": _lat(POW2, 2, spread=2.0, fwd=C16.FWD2, bwd=C16.BWD, seed=243),
    "h16_enc_five_levels_bs4": _lat(POW2_5, 4, spread=2.0, fwd=C16.FWD1, bwd=C16.BWD, seed=244, backward=False),
    "h16_thin": _lat(THIN, 2, Lq=40, spread="offmap", fwd=C16.FWD4, bwd=C16.BWD, seed=245),
    "h16_generic_d16": _lat(POW2, 2, Lq=50, D=16, spread="offmap", fwd=C16.FWD_GENERIC, bwd=C16.BWD_GENERIC, seed=246),
    "h16_generic_m33_odd": _lat(ODD, 1, Lq=40, M=33, spread="offmap", fwd=C16.FWD_GENERIC, bwd=C16.BWD_GENERIC, seed=247),
    "h16_nf_dec": _lat(POW2, 2, Lq=100, kind="nonfinite", spread="offmap", fwd=C16.FWD4, bwd=C16.BWD, seed=248),
}

ALL_CASES = dict(CASES, **H16_CASES)

ROUTES = {}
for _name, _s in ALL_CASES.items():
    if _s["kind"] == "lattice":
        ROUTES.setdefault(_s["fwd"], []).append(_name)
        if _s["backward"]:
            ROUTES.setdefault(_s["bwd"], []).append(_name)


def is_pow2_pyramid(levels):
    return all(e & (e - 1) == 0 for hw in levels for e in hw)


# ------------------------------------------------------------------------------------------------------------------ the tables

@functools.lru_cache(maxsize=None)
def _axis_tables(E):
    """Extent E = 2^a * odd -> (lat_x, lat_l, off_x, off_l): pixel coordinates (sorted, float64) and normalised coordinates of the
    lattice positions x = k, k in [-3, E + 2] (l = j / 2^(a + 1), j odd), and of the off-lattice dyadic positions in
    [-1.5, E + 0.5] (l = j / 2^(a + 3))."""
    a = (E & -E).bit_length() - 1
    odd = E >> a
    lat = [(k, ((2 * k + 1) // odd) / 2.0 ** (a + 1)) for k in range(-3, E + 3) if (2 * k + 1) % odd == 0]
    off = []
    for j in range(-2 ** (a + 3), 2 ** (a + 4)):
        x = j * odd / 8.0 - 0.5
        if -1.5 <= x <= E + 0.5 and (j * odd) % 8 != 4:
            off.append((x, j / 2.0 ** (a + 3)))
    return tuple(np.array(t, np.float64) for t in (*zip(*lat), *zip(*off)))


def _snap(target, xs, ls):
    """Nearest table position to every target pixel coordinate -> its normalised coordinate."""
    i = np.clip(np.searchsorted(xs, target), 1, len(xs) - 1)
    return ls[np.where(np.abs(xs[i - 1] - target) <= np.abs(xs[i] - target), i - 1, i)]


def _axis(rng, role, base, E, valid):
    """Normalised coordinates along one axis of extent E.  role (int array): 0 lattice near `base`, 1 off-lattice dyadic near
    `base`, 2 a skip edge, 3 first / last (valid) / first padded line, 4 normalised 0.0 or 1.0, 5 lattice outside the map.  base:
    target pixel coordinate (float array of role's shape); valid: the valid extent (int array broadcastable to role; == E where the
    image is not masked)."""
    lat_x, lat_l, off_x, off_l = _axis_tables(E)
    shape = role.shape
    valid = np.broadcast_to(valid, shape)
    pick = rng.random(shape)
    edge = np.where(pick < 0.5, -1.0, float(E))
    # last valid line half of the time; else the first line, or (masked image) the first padded one
    border = np.where(pick < 0.5, valid - 1.0, np.where((pick < 0.75) | (valid == E), 0.0, valid * 1.0))
    outside = np.select([pick < 0.25, pick < 0.5, pick < 0.75], [-3.0, -2.0, E + 1.0], E + 2.0)
    target = np.select([role == 0, role == 2, role == 3, role == 5], [np.round(base), edge, border, outside], base)
    out = _snap(target, lat_x, lat_l)
    out = np.where(role == 1, _snap(base + rng.choice([0.25, 0.5, 0.75], shape), off_x, off_l), out)
    return np.where(role == 4, np.where(pick < 0.5, 0.0, 1.0), out)


def _roles(rng, kind):
    """kind (int array, index into KINDS) -> (role_x, role_y) for _axis()."""
    swap = rng.random(kind.shape) < 0.5
    other = np.where(rng.random(kind.shape) < 0.5, 0, 1)          # lattice or off-lattice dyadic, inside
    a = np.select([kind == 0, kind == 1, kind == 2, kind == 3, kind == 4, kind == 5, kind == 6], [0, 1, 0, 2, 3, 4, 5])
    b = np.select([kind == 0, kind == 1, kind == 2, kind == 3, kind == 4, kind == 5, kind == 6], [1, 0, 0, other, 0, other, 0])
    free = kind >= 3                                               # which coordinate carries the special role is random
    return np.where(free & swap, b, a), np.where(free & swap, a, b)


def _draw_kinds(rng, shape, only_skipped=None):
    p = np.array([w for _, w in KINDS])
    kind = rng.choice(len(KINDS), size=shape, p=p / p.sum())
    if only_skipped is not None:      # rows without a sample on the map: skip edges and positions outside
        kind = np.where(only_skipped, np.where(rng.random(shape) < 0.7, 3, 6), kind)
    return kind


def _exact_positions(rng, shp, shape, qpix, valid, only_skipped):
    """Exact normalised positions of `shape` = (N, Lq, m, L, p) samples -> (..., 2).  qpix: None (decoder: targets uniform on the
    level) or (Lq, L, 2) pixel coordinates of the query's pixel on every level; valid (N, L, 2) valid extents (W, H)."""
    N, Lq, m, L, p = shape
    kind = _draw_kinds(rng, shape, only_skipped)
    rx, ry = _roles(rng, kind)
    # a sample of an all-skipped row keeps its other coordinate anywhere: the special one alone decides
    loc = np.zeros(shape + (2,))
    for lv in range(L):
        for ax, role in ((0, rx), (1, ry)):
            E = int(shp[lv, 1 - ax])
            sub = (N, Lq, m, p)
            if qpix is None:
                base = rng.integers(0, E, sub).astype(np.float64)
            else:
                r = min(3, E // 2)      # (+-3 px; fewer on a level of a few pixels, where they would all leave the map)
                near = rng.integers(-r, r + 1, sub).astype(np.float64)
                if E >= 32:      # 12 .. 16 px away, towards the side of the map that has the room
                    q = np.broadcast_to(qpix[None, :, None, lv, None, ax], sub)
                    far = rng.integers(12, 17, sub) * np.where(q + 16 <= E - 1, 1.0, np.where(q - 16 >= 0, -1.0, np.sign(E / 2 - q)))
                    near = np.where(rng.random(sub) < FAR_SHARE, far, near)
                base = qpix[None, :, None, lv, None, ax] + near
            loc[:, :, :, lv, :, ax] = _axis(rng, role[:, :, :, lv, :], base, E, valid[:, None, None, lv, None, ax])
    return loc


def _valid_extents(shp, mask_fracs, N):
    """(N, L, 2) valid extents (W, H) of every image and level (the whole level where the image has no mask)."""
    out = np.empty((N, len(shp), 2), np.int64)
    for n in range(N):
        fh, fw = mask_fracs[n] if mask_fracs is not None else (1.0, 1.0)
        out[n, :, 0] = np.ceil(fw * shp[:, 1])
        out[n, :, 1] = np.ceil(fh * shp[:, 0])
    return out


def _query_pixels(shp):
    """(S, L, 2): the pixel coordinate (x, y) of every encoder query (a pixel centre of its own level) on every level."""
    cen = np.concatenate([np.stack(np.meshgrid((np.arange(w) + 0.5) / w, (np.arange(h) + 0.5) / h), -1).reshape(-1, 2) for h, w in shp])
    return cen[:, None, :] * shp[None, :, ::-1] - 0.5


def _some_rows(rng, shape):
    """One row in a hundred, and at least one."""
    rows = rng.random(shape) < ALL_SKIPPED_ROWS
    rows.flat[rng.integers(rows.size)] = True
    return rows


def make_lattice_case(s):
    """Inputs of a case spec, as test_gpu_msda_bounds.make_case (whose value / logits / grad_out / ordinary locations these are),
    plus `exact` (N, Lq, M, L, P) bool.  Deterministic."""
    c = make_case(dict(s, mask=None))
    rng = np.random.default_rng(5000 + s["seed"])
    shp = c["shapes"]
    N, M, P, L = s["N"], s["M"], s["P"], len(shp)
    encoder = s["Lq"] is None
    Lq = c["gout"].shape[1]
    ft = c["value"].dtype
    fracs = MASK_FRACS[:N] if s["mask"] == "lattice_band" else None
    if fracs is not None:
        c["mask"] = _band_mask(shp, fracs)
        c["value"][c["mask"]] = np.nan
    valid = _valid_extents(shp, fracs, N)
    qpix = _query_pixels(shp) if encoder else None
    full = (N, Lq, M, L, P)
    if s["kind"] == "nonfinite":
        bad = rng.random(full) < NON_FINITE_SHARE
        bad |= _some_rows(rng, (N, Lq, M))[..., None, None]
        which = rng.integers(0, 2, full)
        vals = rng.choice(np.array(NON_FINITE), full)
        key = "off" if s["io"] == "fused" else "loc"
        arr = c[key].copy()
        for ax in range(2):
            arr[..., ax] = np.where(bad & (which == ax), vals, arr[..., ax]).astype(arr.dtype)
        c[key] = arr
        c["exact"] = np.zeros(full, bool)
        return c
    if s["io"] == "fused":
        # the reference points, one per (image, query, level), are ALL table positions; the offsets decide which samples are exact
        dead = _some_rows(rng, (N, Lq))
        ref2 = _exact_positions(rng, shp, (N, Lq, 1, L, 1), qpix, valid, dead[:, :, None, None, None])[:, :, 0, :, 0, :]
        exact = (rng.random(full) < EXACT_SHARE) | dead[:, :, None, None, None]
        wh = shp[:, ::-1].astype(np.float64)
        px = rng.standard_normal(full + (2,)) * s["spread"]
        whole = rng.random(full) < INTEGER_OFFSET_SHARE
        px = np.where(whole[..., None], np.round(px * 2) + np.where(np.round(px * 2) == 0, 1.0, 0.0), px)
        if s["ref_dim"] == 4:
            size = rng.choice([0.0625, 0.125, 0.25], (N, Lq, L, 2))
            ref = np.concatenate([ref2, size], -1)
            off = px / wh[None, None, None, :, None, :] / (size[:, :, None, :, None, :] * 0.5 / P)
        else:
            ref, off = ref2, px
        zero = np.where(rng.random(full + (2,)) < 0.25, -0.0, 0.0)
        off = np.where(exact[..., None], zero, off).astype(np.float32)
        exact = (off == 0).all(-1)
        c.update(ref=ref.astype(np.float32), off=off, exact=exact)
        assert np.array_equal(c["ref"].astype(np.float64), ref)
        return c
    dead = _some_rows(rng, (N, Lq, M))
    exact = (rng.random(full) < EXACT_SHARE) | dead[..., None, None]
    pos = _exact_positions(rng, shp, full, qpix, valid, dead[..., None, None])
    loc = np.where(exact[..., None], pos, c["loc"].astype(np.float64)).astype(ft)
    assert np.array_equal(loc.astype(np.float64)[exact], pos[exact])
    c.update(loc=loc, exact=exact)
    return c


# ------------------------------------------------------------------------------------------------- cached inputs and references

@functools.lru_cache(maxsize=None)
def inputs(name, dtype=None):
    """The case's arrays, read-only.  dtype "fp16" / "bf16" (H16_CASES): value and gout rounded to the 16-bit type, as float32."""
    c = make_lattice_case(ALL_CASES[name])
    if dtype is not None:
        c["value"], c["gout"] = H.round16(c["value"], dtype), H.round16(c["gout"], dtype)
    for a in c.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return c


def reference(name, dtype=None, with_exact=True):
    """The fp64 reference with its bounds, built with the case's `exact` flag (with_exact = False: withheld, as the bounded tests
    of test_gpu_msda_bounds would judge the same inputs)."""
    s, c = ALL_CASES[name], inputs(name, dtype)
    exact = c["exact"] if with_exact else None
    gout = c["gout"] if s["backward"] else None
    if dtype is not None:
        return H.reference(c["value"], c["shapes"], c["loc"], c["attn"], gout, dtype, exact=exact)
    if s["io"] == "fused":
        return R.fused(c["value"], c["shapes"], c["ref"], c["off"], c["logits"], gout, mask=c["mask"], exact=exact)
    return R.msda(c["value"], c["shapes"], c["loc"], c["attn"], gout, exact=exact)


def locations(name, dtype=None):
    """(loc float64 (N, Lq, M, L, P, 2), delta / u) of a case: what the op samples at, the fused prologue restated for fused cases."""
    s, c = ALL_CASES[name], inputs(name, dtype)
    with np.errstate(invalid="ignore", over="ignore"):
        if s["io"] == "fused":
            pro = R.prologue(c["ref"], c["off"], c["logits"], c["shapes"], s["P"])
            return pro["loc"], pro["delta"]
        return np.asarray(c["loc"], np.float64), R.contract_delta(c["loc"], c["shapes"])


def skipped(name, dtype=None):
    """-> (skip, sure): the samples the op skips (strict test on the fp64 coordinates, non-finite ones included), and those of
    them that no correct kernel can take: exact or non-finite, or further than 2 delta from the skip edge."""
    c = inputs(name, dtype)
    shp = c["shapes"]
    loc, delta = locations(name, dtype)
    bad = R.non_finite(loc, shp)
    with np.errstate(invalid="ignore", over="ignore"):
        x, y = R.pixel_coords(loc, shp)
        Hf, Wf = shp[:, 0].astype(np.float64)[:, None], shp[:, 1].astype(np.float64)[:, None]
        skip = ~((x > -1) & (y > -1) & (x < Wf) & (y < Hf))
        wide = 2 * delta * R.U32
        clear = ~((x > -1 - wide) & (y > -1 - wide) & (x < Wf + wide) & (y < Hf + wide))
    return skip, skip & (c["exact"] | bad | clear)
