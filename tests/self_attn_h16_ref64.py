"""The yardstick of the decoder self-attention's ``operand`` arithmetic (``ArithH16`` of csrc/self_attn.hip: fp16 / bf16 operands on the
16-bit MFMA): the float64 attention of the ROUNDED operands with a derived bound per element, and the kernel's operation order
in numpy fp32 (``emulate``).  Test helper (not a conftest); it imports from tests/self_attn_ref64.py and modifies nothing there.

The statement is that of self_attn_ref64 (s, p, o, dP, delta, dS, dQ, dK, dV) on ``q``, ``k``, ``v``, ``gout`` rounded to the
16-bit type with ``msda_h16_ref.round16``: the operands ARE 16-bit numbers, so nothing is lost on the way in.

Contract (include/semidetr_hip.h, semidetr_self_attn_forward_h16), in this order:
  1. s = (fp32 MFMA sum of the exact products q_d k_d) * scale, scale applied in fp32 to the score;
  2. running maximum, exp2, row sum l and lse = m + log l in fp32 on the UNROUNDED probabilities;
  3. P rounded once to the operand type for P V and P^T dO;
  4. dP = fp32 MFMA sum of the exact products dO_d v_d; delta in fp32 from dO and the saved 16-bit out;
  5. dS = p (dP - delta) in fp32, rounded once to the operand type for dS K and dS^T Q; scale on the fp32 accumulators;
  6. every result rounded once on the way out.

ASSUMPTION.  Neither the order nor the rounding mode of the fp32 additions inside a 16-bit MFMA is documented.  The bounds take
an MFMA chain over n products as the sum of n EXACT products (an 11-bit or 8-bit significand squared fits fp32) in any order
with a relative error of at most 2 u per addition (u = 2^-24); that covers truncation as well as round-to-nearest:
g2(n) = gamma(2 n).

Bounds, with u16 / s16 of tests/msda_h16_ref.py (half an ulp relative; half the subnormal spacing), n_i the open keys of row i,
n_j the open queries of key j, T key tiles, D = 32, and E, e, eps, rho, L, eta, c_exp as in self_attn_ref64:
  score     |s^ - s| <= E_ij = gamma(2 D + 2) scale sum_d |q_id| |k_jd|       (D additions at 2 u; scale's rounding; the product)
  weight    relative error of p_j: eps_ij = 2 e_i + c_exp u (1 + |s_ij - m_i|)                        (the fp32 bound's term)
  P16       |rn16(w^) - w^| <= u16 w^ + s16 per OPEN element, at the tile's running maximum; the later rescales (<= 1) and the
            division by l >= 1 only shrink it: u16 p_ij + s16 against p_ij.  A blocked element is an exact 0.
  out       B32 = W_id + gamma(2 n_i + (1 + c_exp) T + 2) (sum_j p |v| + |o|) + sum_j (u16 p_ij (1 + eps_ij) + s16) |v_jd|,
            then the rounding on the way out: B_out = B32 + u16 (|o| + B32) + s16.
  lse       L_i as in self_attn_ref64 with E above: the probabilities enter l unrounded.
  p (bwd)   eta_ij = E_ij + L_i + c_exp u (1 + |s_ij - lse_i|)
  dP        F_ij = gamma(2 D) sum_d |dO_id| |v_jd|
  delta     G_i = sum_d |dO_id| B_out_id + gamma(D + 1) sum_d |dO_id| |o_id|: the saved out carries its whole bound B_out, the
            16-bit rounding included
  dS        fp32: Z_ij = p_ij ((eta_ij + 2 u) |dP_ij - delta_i| + F_ij + G_i); rounded: Z16_ij = Z_ij + u16 (|dS_ij| + Z_ij) + s16
            on open elements
  dQ        scale (sum_j Z16_ij |k_jd| + gamma(2 n_i + 2) sum_j |dS_ij| |k_jd|), then the rounding on the way out
  dK        scale (sum_i Z16_ij |q_id| + gamma(2 n_j + 2) sum_i |dS_ij| |q_id|), then the rounding on the way out
  dV        sum_i (p_ij eta_ij + u16 p_ij (1 + eta_ij) + s16) |dO_id| + gamma(2 n_j) sum_i p_ij |dO_id|, then the rounding
The fp32-level terms (eps, eta, gamma) are first-order statements as in self_attn_ref64 (relative terms below 1e-2, SECOND =
1.01); every 16-bit term is carried exactly, none to first order.
"""
import functools

import numpy as np

import self_attn_cases as C
from msda_h16_ref import S16, U16, round16, widen16
from self_attn_ref64 import C_EXP, SECOND, TILE, TINY, U, gamma

DTYPES = ("fp16", "bf16")


def _head16(q, k, v, g, open_, scale, grads, dt):
    """One (image, head) on float64 copies of the rounded operands -> values and bounds (self_attn_ref64._head's shape)."""
    u16, s16 = U16[dt], S16[dt]
    Lq, D = q.shape
    Lk = k.shape[0]
    T = -(-Lk // TILE)
    aq, ak, av = np.abs(q), np.abs(k), np.abs(v)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        s = np.where(open_, scale * (q @ k.T), -np.inf)
        Es = gamma(2 * D + 2) * abs(scale) * (aq @ ak.T)
        n = open_.sum(1)
        dead = n == 0
        m = np.where(dead, 0.0, s.max(1))
        w = np.where(open_, np.exp(s - m[:, None]), 0.0)
        l = w.sum(1)
        p = w / np.where(dead, 1.0, l)[:, None]
        o = p @ v
        e = np.where(open_, Es, 0.0).max(1)
        x = np.where(open_, m[:, None] - s, 0.0)
        eps = np.where(open_, 2.0 * e[:, None] + C_EXP * U * (1.0 + x), 0.0)
        pe = p * eps
        w_a = pe @ av + pe.sum(1)[:, None] * np.abs(o)
        w_b = eps.max(1)[:, None] * np.sqrt(np.maximum(p @ (v * v) - o * o, 0.0))
        gN = gamma(2.0 * n + (1.0 + C_EXP) * T + 2.0)
        p16 = np.where(open_, u16 * p * (1.0 + eps) + s16, 0.0)
        b32 = SECOND * (np.minimum(w_a, w_b) + gN[:, None] * (p @ av + np.abs(o))) + p16 @ av + TINY
        b_out = widen16(b32, o, dt)
        res = {"out": np.where(dead[:, None], np.nan, o), "b_out": b_out, "rel": float(eps.max(initial=0.0))}
        ll = np.where(dead, 1.0, l)
        logl = np.log(ll)
        lse = m + logl
        rho = e + (p * C_EXP * U * (1.0 + x)).sum(1) + gamma(n + (1.0 + C_EXP) * T)
        Lb = rho + 6.0 * U * np.abs(logl) + U * np.abs(lse)
        res["lse"], res["b_lse"] = np.where(dead, -np.inf, lse), SECOND * Lb + TINY
        if not grads:
            return res
        ag = np.abs(g)
        gv = ag @ av.T
        dP = g @ v.T
        F = gamma(2 * D) * gv
        delta = (g * o).sum(1)
        G = (ag * b_out).sum(1) + gamma(D + 1) * (ag * np.abs(o)).sum(1)
        eta = np.where(open_, Es + Lb[:, None] + C_EXP * U * (1.0 + np.abs(np.where(open_, s, 0.0) - lse[:, None])), 0.0)
        dd = np.where(open_, dP - delta[:, None], 0.0)
        dS = p * dd
        aS = np.abs(dS)
        Z = SECOND * p * ((eta + 2.0 * U) * np.abs(dd) + F + G[:, None])
        Z16 = np.where(open_, Z + u16 * (aS + Z) + s16, 0.0)
        P16 = np.where(open_, SECOND * p * eta + u16 * p * (1.0 + eta) + s16, 0.0)
        nk = open_.sum(0)
        sc = abs(scale)
        dq, dk, dv = scale * (dS @ k), scale * (dS.T @ q), p.T @ g
        res.update(
            dq=dq, b_dq=widen16(sc * (Z16 @ ak + SECOND * gamma(2.0 * n + 2.0)[:, None] * (aS @ ak)) + TINY, dq, dt),
            dk=dk, b_dk=widen16(sc * (Z16.T @ aq + SECOND * gamma(2.0 * nk + 2.0)[:, None] * (aS.T @ aq)) + TINY, dk, dt),
            dv=dv, b_dv=widen16(P16.T @ ag + SECOND * gamma(2.0 * nk)[:, None] * (p.T @ ag) + TINY, dv, dt))
        res["rel"] = max(res["rel"], float(eta.max(initial=0.0)))
    return res


def rounded(problem, dtype16):
    """q, k, v, gout of a problem rounded to the 16-bit type, as float32 arrays (exact)."""
    return {n: round16(problem[n], dtype16) for n in ("q", "k", "v", "gout") if problem.get(n) is not None}


def ref64_h16(problem, dtype16, grads=True):
    """``problem`` as ``self_attn_ref64.ref64`` takes it.  -> float64 ``out`` (Lq, B, E; NaN in a fully blocked row), ``lse``
    (B, H, Lq; -inf there), ``dq``, ``dk``, ``dv`` of the operands rounded to ``dtype16`` ('fp16' / 'bf16') and their bounds
    ``b_out`` ... for the ``operand`` arithmetic (module docstring); ``rel``: the largest fp32-level relative error term."""
    r16 = rounded(problem, dtype16)
    q, k, v = (r16[n].astype(np.float64) for n in "qkv")
    (Lq, B, E), Lk, H = q.shape, k.shape[0], int(problem["heads"])
    D = E // H
    scale = float(D) ** -0.5 if problem.get("scale") is None else float(problem["scale"])
    mask = problem.get("mask")
    open_ = np.ones((Lq, Lk), bool) if mask is None else ~np.asarray(mask, bool)
    grads = grads and "gout" in r16
    g = r16["gout"].astype(np.float64) if grads else None
    names = ["out", "b_out"] + (["dq", "b_dq", "dk", "b_dk", "dv", "b_dv"] if grads else [])
    res = {n_: np.zeros((Lq if n_[-1] in "tq" else Lk, B, E)) for n_ in names}
    res["lse"], res["b_lse"], res["rel"] = np.zeros((B, H, Lq)), np.zeros((B, H, Lq)), 0.0
    for b in range(B):
        for h in range(H):
            sl = slice(h * D, (h + 1) * D)
            r = _head16(q[:, b, sl], k[:, b, sl], v[:, b, sl], g[:, b, sl] if grads else None, open_, scale, grads, dtype16)
            for n_ in names:
                res[n_][:, b, sl] = r[n_]
            res["lse"][b, h], res["b_lse"][b, h] = r["lse"], r["b_lse"]
            res["rel"] = max(res["rel"], r["rel"])
    return res


@functools.lru_cache(maxsize=None)
def reference(name, dtype16):
    """The statement of a case of tests/self_attn_cases.py with its bounds, computed once and shared; not to be modified."""
    p = C.cases()[name]
    return ref64_h16(p, dtype16, grads=not p["forward_only"])


def judge(got, ref):
    """-> {tensor: largest |got - ref| / bound over ALL its elements} for the tensors in ``got`` (``out``, ``lse``, ``dq``,
    ``dk``, ``dv``).  NaN (``out``) and -inf (``lse``) of a fully blocked row must be matched exactly; a NaN or inf on one side
    only, or left over from a fill, is inf."""
    rep = {}
    for name, val in got.items():
        want, bound = ref[name], ref["b_" + name]
        val = np.asarray(val, np.float64)
        assert val.shape == want.shape, (name, val.shape, want.shape)
        same = (np.isnan(want) & np.isnan(val)) | (np.isinf(want) & (val == want))
        with np.errstate(invalid="ignore"):
            ratio = np.abs(val - want) / bound
        ratio[same] = 0.0
        ratio[~same & ~(np.isfinite(val) & np.isfinite(want))] = np.inf
        rep[name] = float(ratio.max())
    return rep


def check(got, ref, name=""):
    """Every element of every tensor in ``got`` within its bound.  Returns the report of ``judge``."""
    assert ref["rel"] < 1e-2, f"{name}: a relative error term of {ref['rel']:.3g}: the first-order bounds do not apply"
    rep = judge(got, ref)
    bad = {k_: v_ for k_, v_ in rep.items() if not v_ <= 1.0}
    assert not bad, f"{name}: outside the bound (error / bound): {bad}"
    return rep


def table(name, rep):
    return f"{name:32s} " + " ".join(f"{k_}={v_:.3f}" for k_, v_ in rep.items())


def emulate(problem, dtype16, no_scale=False, mask=None, drop_last_tile=False, no_rescale=False, swap_dk_dv=False,
            round_scores=False, sum_rounded_p=False):
    """The kernels' operation order in numpy fp32 with ``round16`` at the contract's three rounding points (P, dS, the results):
    online softmax over key tiles of 32 in the forward, the saved lse in the backward.  The keyword arguments are the mutations
    of tests/test_self_attn_h16_ref.py (``mask``: another mask than the problem's)."""
    f = np.float32
    r16 = rounded(problem, dtype16)
    q, k, v = r16["q"], r16["k"], r16["v"]
    (Lq, B, E), Lk, H = q.shape, k.shape[0], int(problem["heads"])
    D = E // H
    scale = f(1.0) if no_scale else f(D ** -0.5 if problem.get("scale") is None else problem["scale"])
    mask = problem.get("mask") if mask is None else mask
    blocked = np.zeros((Lq, Lk), bool) if mask is None else np.asarray(mask, bool)
    grads = not problem.get("forward_only") and "gout" in r16
    rnd = lambda a: round16(a, dtype16)      # noqa: E731
    got = {"out": np.zeros((Lq, B, E), f), "lse": np.zeros((B, H, Lq), f)}
    if grads:
        got.update(dq=np.zeros((Lq, B, E), f), dk=np.zeros((Lk, B, E), f), dv=np.zeros((Lk, B, E), f))
    tiles = list(range(0, Lk, TILE))
    if drop_last_tile:
        tiles = tiles[:-1]
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        for b in range(B):
            for h in range(H):
                sl = slice(h * D, (h + 1) * D)
                qh, kh, vh = q[:, b, sl], k[:, b, sl], v[:, b, sl]
                score = lambda kk, bl: np.where(bl, f(-np.inf), rnd((qh @ kk.T) * scale) if round_scores else (qh @ kk.T) * scale)  # noqa: E731
                m, l, O = np.full(Lq, -np.inf, f), np.zeros(Lq, f), np.zeros((Lq, D), f)
                for t in tiles:
                    s = score(kh[t:t + TILE], blocked[:, t:t + TILE])
                    mn = np.maximum(m, s.max(1))
                    safe = np.where(np.isinf(mn), f(0), mn)
                    alpha = np.exp(m - safe)
                    pt = np.exp(s - safe[:, None])
                    p16 = rnd(pt)
                    l = l * alpha + (p16 if sum_rounded_p else pt).sum(1)
                    O = (O if no_rescale else O * alpha[:, None]) + p16 @ vh[t:t + TILE]
                    m = mn
                out = rnd(O / l[:, None])
                lse = m + np.log(l)
                got["out"][:, b, sl], got["lse"][b, h] = out, lse
                if not grads:
                    continue
                gh = r16["gout"][:, b, sl]
                delta = (gh * out).sum(1, dtype=f)
                pb = np.exp(score(kh, blocked) - lse[:, None])
                dS = pb * (gh @ vh.T - delta[:, None])
                dS16, P16 = rnd(dS), rnd(pb)
                got["dq"][:, b, sl] = rnd((dS16 @ kh) * scale)
                dk, dv = rnd((dS16.T @ qh) * scale), rnd(P16.T @ gh)
                got["dk"][:, b, sl], got["dv"][:, b, sl] = (dv, dk) if swap_dk_dv else (dk, dv)
    return got
