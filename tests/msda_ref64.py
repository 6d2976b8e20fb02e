"""Plain float64 statement of multi-scale deformable attention, with a per-element error bound for fp32 / fp64 kernels.

Test helper (not a conftest): the GPU parity tests in tests/test_gpu_msda_bounds.py compare every kernel route against it, and
tests/test_msda_ref64.py pins it to the C oracle and shows the bound is both satisfiable by honest fp32 arithmetic and broken by
the shortcuts a rewrite might take.  It gathers corners explicitly in numpy (no call into the oracle), chunked over queries so a
full-size encoder call (N = 4, Lq = S = 22 223) fits in memory.

Operation (ms_deform_im2col_cuda.cuh semantics, align_corners = False, zero padding): for a sample at normalised (lx, ly) of level
l with weight a, x = lx * W - 0.5, y = ly * H - 0.5; it is skipped unless -1 < x < W and -1 < y < H; its four corners
(y0 + i, x0 + j), y0 = floor(y), x0 = floor(x), carry the bilinear weights c_k = (1 - |y - y_k|)(1 - |x - x_k|) and count only
inside the map.  out = sum_s a_s sum_k c_k v_k; grad_value[row_k] += a c_k g; grad_attn = g . sum_k c_k v_k;
grad_loc = (W a g . sum_k dc_k/dx v_k, H a g . sum_k dc_k/dy v_k).

Error model.  u = 2^-24 for fp32.  Every floating-point operation of a kernel is allowed ONE ulp (2u relative) rather than half an
ulp: that covers hardware reciprocal / exp (v_rcp_f32, v_exp_f32: 1 ulp) and the FMA-or-not choice of the compiler.  For an
element e formed as a sum of products, any summation order and any grouping gives (first order)

    |got - ref| <= 2u * n_e * A_e + 2 * C_e + tiny

  * A_e = sum over the terms summed into e of |term|, in fp64;
  * n_e = the number of those terms + DEPTH: a sum of n terms in any order has at most n - 1 roundings on a term's path, and
    DEPTH = 8 bounds the roundings inside one term (corner weight: 1 - ly, 1 - lx, product = 3; times value or grad_out = 1;
    four-corner sum = 3; times attention = 1).  out: n = 4 L P + DEPTH; grad_attn, grad_loc: n = 4 D + DEPTH (the sum runs over
    channels AND corners, whichever first); grad_value: n = number of (query, sample, corner) contributions to the row
    (np.bincount) + DEPTH;
  * C_e = input sensitivity, the part of the error that comes from the kernel forming the sample's inputs in fp32 rather than
    from summing: sum over contributing samples of  a * (sum over valid corners of |v_k|) * delta  +  eps * |term|.
    delta bounds the error of EACH pixel coordinate; the factor 2 in front of C_e is for the two coordinates (a bilinear weight
    moves by at most 1 per pixel per coordinate).  The corner sum is UNWEIGHTED: a corner whose weight is tiny still has full
    slope.  Contract path (normalised locations given): x = fl(fl(lx * W) - 0.5) -> |dx| <= 2u(|lx W| + |x|) <= 2u(|x| + 1), so
    delta = 2u(|x| + |y| + 2) covers both coordinates.  Fused prologue (locations formed in the kernel): per coordinate, with
    o the sampling offset in pixels of the level, offset scaling (off / W, or off / P * w * 0.5 for boxes, up to three ops on a
    quantity of size |o|) 3 * 2u|o|, + reference 2u|x + 0.5|, * W 2u|x + 0.5|, - 0.5 2u|x| -> 2u(3|o| + 3|x| + 2), so
    delta = 2u(3(|x| + |y|) + 3(|ox| + |oy|) + 2).  eps is the relative error of the attention weight: 0 when it is an input;
    for the fused softmax a_i = exp(t_i) / sum_j exp(t_j), t = logit - max: the subtraction 2u|t|, exp as exp2(t log2 e)
    2u|t| + 2u, the sum over n = L P positive terms 2u(n - 1) plus the others' exp errors 2u sum_j a_j (2|t_j| + 1), the division
    (reciprocal + multiply) 4u  ->  eps_i = 2u(2|t_i| + 2 sum_j a_j |t_j| + n + 4).
    A sample that is skipped (outside -1 < x < W, -1 < y < H) but within 2 delta of that edge adds the |v| of the corners it
    would have just inside: a kernel whose coordinate lands inside takes it with a weight of at most delta.
  * grad_loc / grad_offsets are excluded where a sample lies within 2 delta of a pixel-centre line (the kink set of the bilinear
    interpolant, as conftest.kink_mask; the one-sided derivative there depends on which side rounding puts the coordinate).
    Those two are linear in the coordinate along their own axis, so their C_e is a * W * sum_d |g| sum_k |v_k| * delta.
  * The fused epilogue: grad_offsets = grad_loc * s (s = 1 / W, or w * 0.5 / P for boxes): |s| times the grad_loc bound plus 3
    more roundings (n + 3).  grad_logits = a (g_a - sum_j a_j g_aj): the grad_attn bounds carried through with absolute values
    (|a_i| b_i + a_i sum_j a_j b_j), the softmax's eps on both a's, and 2u(n + 4) on a_i (|g_ai| + sum_j a_j |g_aj|).
  * tiny = n_e * 2^-126 (one flushed subnormal per term).
  * fp64 kernels: u = 2^-53, tiny with 2^-1022, and twice the bound.

The factor 2, DEPTH and the prologue constants are fixed here from this derivation; no test scales the bound.

Exact samples (msda(..., exact=...), tests/msda_lattice_cases.py).  delta pays for the rounding of x = fl(fl(lx * W) - 0.5).  Where
lx * W and lx * W - 0.5 are both fp32 numbers -- a dyadic lx on a level whose extent makes the product dyadic too: pixel centres,
the skip edges x = -1 and x = W, normalised 0 and 1 -- neither operation rounds, fused into one FMA or not, so every correct kernel
holds the very x of this reference and no delta is owed: C_e gets nothing from the sample, it is never in the kink set and never an
edge sample.  What the contract says AT such a point is then determinate and is judged like anything else: the cell is floor(x), so
on a pixel-centre line the far corner has weight exactly 0 and grad_loc is the right-hand derivative; the skip test is strict, so
x = -1 and x = W contribute nothing and have zero gradients; a corner off the map (or padded) is zero padding even at weight 0.
The flag is the caller's claim; tests/test_msda_lattice_ref.py proves it bit for bit for every flagged sample.  For the fused
prologue the location is formed in the kernel (ref + off * rcp(W)), so only a sample whose offset is exactly 0 may be flagged.

Non-finite samples.  A sample whose pixel coordinate is NaN, infinite or beyond fp32's range fails every comparison of the skip
test: it is skipped, contributes nothing and has zero gradients, like any other skipped sample, and it has zero sensitivity (no
rounding moves it onto the map).
"""
import numpy as np

U32 = 2.0 ** -24
U64 = 2.0 ** -53
DEPTH = 8

# (~8 M gathered corner channels per chunk: a few hundred MB of float64 temporaries at most)
_CHUNK_ELEMS = 1 << 23


class Bounded:
    """A reference result with what its bound is built from.  val, A, C (C in units of u: the bound scales with the kernel's
    precision) are arrays of the result's shape; n is an array or a scalar; skip (optional bool array) marks elements that are
    not compared (kink set)."""

    def __init__(self, val, A, n, C, skip=None):
        self.val, self.A, self.n, self.C, self.skip = val, A, n, C, skip

    def bound(self, dtype=np.float32):
        if np.dtype(dtype) == np.float64:
            return 2.0 * (2 * U64 * self.n * self.A + 2 * U64 * self.C + self.n * 2.0 ** -1022)
        return 2 * U32 * self.n * self.A + 2 * U32 * self.C + self.n * 2.0 ** -126

    def ratio(self, got, dtype=np.float32):
        """|got - ref| / bound elementwise (0 where skipped; inf where got is not finite)."""
        got = np.asarray(got, np.float64).reshape(self.val.shape)
        r = np.abs(got - self.val) / self.bound(dtype)
        r = np.where(np.isfinite(got), r, np.inf)
        if self.skip is not None:
            r = np.where(self.skip, 0.0, r)
        return r


def _level_table(shapes):
    shapes = np.asarray(shapes, np.int64)
    hw = shapes[:, 0] * shapes[:, 1]
    return shapes, np.concatenate([[0], np.cumsum(hw)[:-1]]).astype(np.int64)


def pixel_coords(loc, shapes):
    """(x, y) in pixels of the level (x = lx * W - 0.5), float64, shape loc.shape[:-1]."""
    shapes, _ = _level_table(shapes)
    H = shapes[:, 0].astype(np.float64).reshape(-1, 1)
    W = shapes[:, 1].astype(np.float64).reshape(-1, 1)
    loc = np.asarray(loc, np.float64)
    return loc[..., 0] * W - 0.5, loc[..., 1] * H - 0.5


def contract_delta(loc, shapes):
    """delta / u of the reference contract (locations are inputs): 2(|x| + |y| + 2)."""
    x, y = pixel_coords(loc, shapes)
    return 2.0 * (np.abs(x) + np.abs(y) + 2.0)


def prologue(ref, off, logits, shapes, P):
    """The fused prologue in fp64 (ms_deform_attn.py:99-111): softmax over L * P and locations from 2-d points or 4-d boxes.
    -> dict(loc, attn, delta (/u), eps (/u), scale (d loc / d offset per coordinate, broadcastable to off))."""
    shapes, _ = _level_table(shapes)
    off = np.asarray(off, np.float64)
    ref = np.asarray(ref, np.float64)
    N, Lq, M, L, P_, _ = off.shape
    assert P_ == P
    lg = np.asarray(logits, np.float64).reshape(N, Lq, M, L * P)
    t = lg - lg.max(-1, keepdims=True)
    e = np.exp(t)
    a = e / e.sum(-1, keepdims=True)
    eps = 2.0 * (2 * np.abs(t) + 2 * (a * np.abs(t)).sum(-1, keepdims=True) + L * P + 4)
    norm = np.stack([shapes[:, 1], shapes[:, 0]], -1).astype(np.float64)[None, None, None, :, None, :]   # (W, H)
    if ref.shape[-1] == 2:
        scale = np.broadcast_to(1.0 / norm, (1, 1, 1, L, 1, 2))
        loc = ref[:, :, None, :, None, :] + off * scale
    else:
        scale = ref[:, :, None, :, None, 2:] * 0.5 / P
        loc = ref[:, :, None, :, None, :2] + off * scale
    o_px = off * scale * norm
    x, y = pixel_coords(loc, shapes)
    delta = 2.0 * (3 * (np.abs(x) + np.abs(y)) + 3 * (np.abs(o_px[..., 0]) + np.abs(o_px[..., 1])) + 2)
    return dict(loc=loc, attn=a.reshape(N, Lq, M, L, P), delta=delta, eps=eps.reshape(N, Lq, M, L, P), scale=scale,
                logit_shift=t)


def _geometry(loc_c, H, W, start, M, clamp=None):
    """Corners of a chunk of samples.  loc_c (Q, M, L, P, 2) float64; H, W, start (L,) -> rows (..., 4) into the (S * M, D)
    value view, ok (..., 4) corner inside the map (and sample not skipped), c (..., 4) weights, dcx / dcy (..., 4) their
    derivatives (all 0 where not ok), x, y (..., ) pixel coordinates."""
    Hf, Wf = H.astype(np.float64)[:, None], W.astype(np.float64)[:, None]
    x = loc_c[..., 0] * Wf - 0.5
    y = loc_c[..., 1] * Hf - 0.5
    if clamp is not None:                      # (pixels; the samples just outside the map, moved just inside)
        x, y = np.clip(x, -1 + clamp, Wf - clamp), np.clip(y, -1 + clamp, Hf - clamp)
    inside = (y > -1) & (x > -1) & (y < Hf) & (x < Wf)
    y0, x0 = np.floor(y), np.floor(x)
    ly, lx = y - y0, x - x0
    hy, hx = 1 - ly, 1 - lx
    c = np.stack([hy * hx, hy * lx, ly * hx, ly * lx], -1)
    dcx = np.stack([-hy, hy, -ly, ly], -1)
    dcy = np.stack([-hx, -lx, hx, lx], -1)
    cy = y0[..., None] + np.array([0, 0, 1, 1])
    cx = x0[..., None] + np.array([0, 1, 0, 1])
    Hi, Wi = Hf[..., None], Wf[..., None]
    ok = inside[..., None] & (cy >= 0) & (cx >= 0) & (cy <= Hi - 1) & (cx <= Wi - 1)
    m = np.arange(M).reshape(1, M, 1, 1, 1)
    pix = start.reshape(-1, 1, 1) + np.where(ok, cy, 0).astype(np.int64) * W.reshape(-1, 1, 1) + np.where(ok, cx, 0).astype(np.int64)
    return pix * M + m, ok, np.where(ok, c, 0.0), np.where(ok, dcx, 0.0), np.where(ok, dcy, 0.0), x, y


F32_MAX = float(np.finfo(np.float32).max)


def non_finite(loc, shapes):
    """Samples whose pixel coordinate is NaN, infinite or beyond fp32's range (module docstring), shape loc.shape[:-1]."""
    with np.errstate(invalid="ignore", over="ignore"):
        x, y = pixel_coords(loc, shapes)
        return ~((np.abs(x) <= F32_MAX) & (np.abs(y) <= F32_MAX))


def msda(value, shapes, loc, attn, gout=None, delta=None, eps=None, mask=None, weights_hook=None, exact=None):
    """The op in fp64 with bounds.  value (N,S,M,D), loc (N,Lq,M,L,P,2), attn (N,Lq,M,L,P), gout (N,Lq,M*D) or None.
    delta / eps (per sample, units of u): default the reference contract's (contract_delta, 0).  mask (N,S) bool: value is
    masked_fill'ed with 0 there (NaN in padded rows never reaches a result) and grad_value is 0 there (masked_fill's backward).
    weights_hook(a, c) -> (a, c): test mutants only (tests/test_msda_ref64.py).  exact (N,Lq,M,L,P) bool: samples whose pixel
    coordinates the kernel holds without rounding (module docstring): delta 0, never in the kink set, never an edge sample.
    -> dict with Bounded 'out' and, with gout, 'grad_value', 'grad_loc', 'grad_attn'."""
    shapes, starts = _level_table(shapes)
    H, W = shapes[:, 0], shapes[:, 1]
    value = np.asarray(value)
    N, S, M, D = value.shape
    loc = np.asarray(loc)
    _, Lq, _, L, P, _ = loc.shape
    attn = np.asarray(attn)
    bad = non_finite(loc, shapes)
    if bad.any():      # skipped, zero sensitivity: moved to a finite place far off the map, so that nothing below meets inf - inf
        loc = np.where(bad[..., None], -2.0, loc)
        delta = None if delta is None else np.where(bad, 0.0, np.broadcast_to(delta, attn.shape))
    if delta is None:
        delta = contract_delta(loc, shapes)
        if bad.any():
            delta = np.where(bad, 0.0, delta)
    eps = np.zeros(attn.shape) if eps is None else np.broadcast_to(eps, attn.shape)
    delta = np.broadcast_to(delta, attn.shape)
    if exact is not None:
        exact = np.broadcast_to(np.asarray(exact, bool), attn.shape)
        delta = np.where(exact, 0.0, delta)
    out = [np.zeros((N, Lq, M, D)) for _ in range(3)]
    if gout is not None:
        gout = np.asarray(gout, np.float64).reshape(N, Lq, M, D)
        gv = [np.zeros((N, S * M + 1, D)) for _ in range(3)]
        cnt = np.zeros((N, S * M + 1))
        ga = [np.zeros((N, Lq, M, L, P)) for _ in range(3)]
        gl = [np.zeros((N, Lq, M, L, P, 2)) for _ in range(3)]
        kink = np.zeros((N, Lq, M, L, P), bool)
    qc = max(1, _CHUNK_ELEMS // (M * L * P * 4 * D))
    for n in range(N):
        v = np.asarray(value[n], np.float64).reshape(S, M, D)
        if mask is not None:
            v = np.where(np.asarray(mask[n], bool)[:, None, None], 0.0, v)
        vflat = np.concatenate([v.reshape(S * M, D), np.zeros((1, D))])
        for q0 in range(0, Lq, qc):
            sl = slice(q0, min(Lq, q0 + qc))
            rows, ok, c, dcx, dcy, x, y = _geometry(np.asarray(loc[n, sl], np.float64), H, W, starts, M)
            rows = np.where(ok, rows, S * M)
            # a skipped sample within delta of the map's edge (-1 < x < W, -1 < y < H) may be taken by a kernel: with weight
            # <= delta on the corners it would have inside -- their |v| join its sensitivity (C_e), nothing else
            wide = 2 * delta[n, sl] * U32
            Hf, Wf = H.astype(np.float64)[:, None], W.astype(np.float64)[:, None]
            edge = ~ok.any(-1) & (x > -1 - wide) & (y > -1 - wide) & (x < Wf + wide) & (y < Hf + wide)
            if exact is not None:      # (already so: wide == 0 there and the skip test is strict)
                edge &= ~exact[n, sl]
            edge_rows = None
            if edge.any():
                tight = np.minimum(wide, 0.25)
                er, eok = _geometry(np.asarray(loc[n, sl], np.float64), H, W, starts, M, clamp=tight)[:2]
                eok &= edge[..., None]
                edge_rows = np.where(eok, er, S * M)
            a = np.asarray(attn[n, sl], np.float64)
            if weights_hook is not None:
                a, c = weights_hook(a, c)
            dl, ep = delta[n, sl] * 1.0, eps[n, sl] * 1.0
            V = vflat[rows]                                                   # (Q, M, L, P, 4, D)
            aV = np.abs(V)
            val = np.einsum("...k,...kd->...d", c, V)
            wabs = np.einsum("...k,...kd->...d", c, aV)
            sabs = aV.sum(-2)
            if edge_rows is not None:
                sabs = sabs + np.abs(vflat[edge_rows]).sum(-2)
            aa = np.abs(a)[..., None]
            out[0][n, sl] = (a[..., None] * val).sum((2, 3))
            out[1][n, sl] = (aa * wabs).sum((2, 3))
            out[2][n, sl] = (aa * (sabs * dl[..., None] + ep[..., None] * wabs)).sum((2, 3))
            if gout is None:
                continue
            g = gout[n, sl][:, :, None, None, :]                              # (Q, M, 1, 1, D)
            ag = np.abs(g)
            ga[0][n, sl] = (g * val).sum(-1)
            ga[1][n, sl] = (ag * wabs).sum(-1)
            ga[2][n, sl] = (ag * sabs).sum(-1) * dl
            for j, (dc, ext) in enumerate(((dcx, W), (dcy, H))):
                e = ext.astype(np.float64).reshape(-1, 1)
                gl[0][n, sl, ..., j] = e * a * np.einsum("...d,...k,...kd->...", g, dc, V)
                A = e * np.abs(a) * np.einsum("...d,...k,...kd->...", ag, np.abs(dc), aV)
                gl[1][n, sl, ..., j] = A
                gl[2][n, sl, ..., j] = e * np.abs(a) * (ag * sabs).sum(-1) * dl + ep * A
            kink[n, sl] = (np.abs(y - np.round(y)) <= wide) | (np.abs(x - np.round(x)) <= wide)
            if exact is not None:      # on a line the contract is determinate: floor's cell, the right-hand derivative
                kink[n, sl] &= ~exact[n, sl]
            # grad_value: contribution i = (query, head, sample, corner) -> row; weights a c_k times the (query, head) row of gout
            w = (a[..., None] * c).reshape(-1)
            wA = (np.abs(a)[..., None] * c).reshape(-1)
            wC = (np.abs(a)[..., None] * (dl[..., None] + ep[..., None] * c)).reshape(-1)
            r = rows.reshape(-1)
            qm = np.broadcast_to(np.arange(rows.shape[0] * M).reshape(rows.shape[0], M, 1, 1, 1), rows.shape).reshape(-1)
            gq = gout[n, sl].reshape(-1, D)
            cnt[n] += np.bincount(r, weights=ok.reshape(-1).astype(np.float64), minlength=S * M + 1)
            for k, (wt, gg) in enumerate(((w, gq), (wA, np.abs(gq)), (wC, np.abs(gq)))):
                gv[k][n] += _scatter(r, qm, wt, gg, S * M + 1)
            if edge_rows is not None:
                wE = np.broadcast_to((np.abs(a) * dl)[..., None], edge_rows.shape).reshape(-1)
                gv[2][n] += _scatter(edge_rows.reshape(-1), qm, wE, np.abs(gq), S * M + 1)
    res = dict(out=Bounded(out[0].reshape(N, Lq, M * D), out[1].reshape(N, Lq, M * D), 4 * L * P + DEPTH,
                           out[2].reshape(N, Lq, M * D)))
    if gout is None:
        return res
    cut = [x[:, :S * M].reshape(N, S, M, D) for x in gv]
    n_gv = np.broadcast_to(cnt[:, :S * M].reshape(N, S, M, 1), (N, S, M, D)) + DEPTH
    if mask is not None:
        pad = np.asarray(mask, bool)[:, :, None, None]
        cut = [np.where(pad, 0.0, x) for x in cut]
    res["grad_value"] = Bounded(cut[0], cut[1], n_gv, cut[2])
    res["grad_attn"] = Bounded(ga[0], ga[1], 4 * D + DEPTH, ga[2])
    res["grad_loc"] = Bounded(gl[0], gl[1], 4 * D + DEPTH, gl[2], skip=np.broadcast_to(kink[..., None], gl[0].shape))
    return res


def _scatter(rows, qm, w, g, nrows):
    """sum over contributions i of w_i * g[qm_i, :] into rows[i] -> (nrows, D)."""
    import scipy.sparse as sp
    m = sp.csr_matrix((w, (rows, qm)), shape=(nrows, g.shape[0]))
    return np.asarray(m @ g)


def forward(value, shapes, loc, attn, **kw):
    return msda(value, shapes, loc, attn, **kw)["out"]


def backward(value, shapes, loc, attn, gout, **kw):
    r = msda(value, shapes, loc, attn, gout, **kw)
    return r["grad_value"], r["grad_loc"], r["grad_attn"]


def fused(value, shapes, ref, off, logits, gout=None, mask=None, exact=None):
    """The fused prologue + op + epilogue in fp64: dict with 'out' and, with gout, 'grad_value', 'grad_offsets', 'grad_logits'
    (and the intermediate 'grad_loc' / 'grad_attn' against the prologue's locations).  exact: as msda(), and only where the
    sample's offset is exactly 0 (the kernel forms ref + off * rcp(W): with off = 0 that is ref, whatever rcp gives)."""
    shapes, _ = _level_table(shapes)
    P = np.asarray(off).shape[4]
    if exact is not None:
        assert not (np.asarray(exact, bool) & (np.asarray(off) != 0).any(-1)).any(), "fused: exact needs a zero offset"
    with np.errstate(invalid="ignore", over="ignore"):      # (non-finite offsets: msda() skips those samples)
        pro = prologue(ref, off, logits, shapes, P)
    res = msda(value, shapes, pro["loc"], pro["attn"], gout, delta=pro["delta"], eps=pro["eps"], mask=mask, exact=exact)
    res["prologue"] = pro
    if gout is None:
        return res
    gl, ga = res["grad_loc"], res["grad_attn"]
    s = np.abs(pro["scale"])
    res["grad_offsets"] = Bounded(gl.val * pro["scale"], gl.A * s, gl.n + 3, gl.C * s, skip=gl.skip)
    N, Lq, M, L, P = ga.val.shape
    a = pro["attn"].reshape(N, Lq, M, L * P)
    ep = pro["eps"].reshape(a.shape)
    g = ga.val.reshape(a.shape)
    b = (ga.n * ga.A + ga.C).reshape(a.shape)             # the grad_attn bound / 2u (units of u / 2)
    dot = (a * g).sum(-1, keepdims=True)
    val = a * (g - dot)
    # (carried: 2u-bound of g_a through a (g_i - sum a_j g_j); eps on a_i and on the a_j inside the dot; rounding of the epilogue)
    carried = a * b + a * (a * b).sum(-1, keepdims=True)
    eps_part = ep * a * np.abs(g - dot) + a * (ep * a * np.abs(g)).sum(-1, keepdims=True)
    A = a * (np.abs(g) + (a * np.abs(g)).sum(-1, keepdims=True))
    # bound = 2u n A + 2 C: the carried part enters as C = carried (it already is a 2u-bound / 2u), eps as eps_part / 2
    n_ep = L * P + 4
    res["grad_logits"] = Bounded(val, A, n_ep, carried + eps_part / 2)
    return res


def check(route, what, got, ref, dtype=np.float32, geometry=None):
    """Assert |got - ref.val| <= ref.bound elementwise; returns the worst err / bound.  On failure the message names the route,
    the worst element's index, err / bound and (geometry(index) -> str) the samples behind it."""
    r = ref.ratio(got, dtype)
    worst = float(r.max()) if r.size else 0.0
    if not worst <= 1.0:
        idx = np.unravel_index(int(np.argmax(r)), r.shape)
        g = np.asarray(got, np.float64).reshape(ref.val.shape)[idx]
        nbad = int((r > 1.0).sum())
        msg = (f"{route} {what}: {nbad} element(s) out of bound, worst at {tuple(int(i) for i in idx)}: got {g!r} ref "
               f"{ref.val[idx]!r} err/bound {worst:.3g} (bound {ref.bound(dtype)[idx]:.3g}, A {ref.A[idx]:.3g}, "
               f"n {np.broadcast_to(ref.n, r.shape)[idx]:.0f}, C/u {ref.C[idx]:.3g})")
        if geometry is not None:
            msg += "; " + geometry(what, idx)
        raise AssertionError(msg)
    return worst
