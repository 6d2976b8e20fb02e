"""The decoder self-attention core in plain float64, with a derived bound per element for an fp32 implementation.

    s_ij = scale * sum_d q_id k_jd   (blocked: -inf),   p_ij = softmax_j(s_ij),   o_id = sum_j p_ij v_jd
    dP_ij = sum_d dO_id v_jd,  delta_i = sum_d dO_id o_id,  dS_ij = p_ij (dP_ij - delta_i)
    dQ_id = scale sum_j dS_ij k_jd,  dK_jd = scale sum_i dS_ij q_id,  dV_jd = sum_i p_ij dO_id

per image and head on seq-first ``(L, B, H * D)`` arrays: what ``nn.MultiheadAttention`` computes between its two projections
(it agrees with torch's float64 module to 4e-16 with the dn mask; a fully blocked row is NaN in that row only).

Bounds (``check_self_attn``), from the operation order of csrc/self_attn.hip; u = 2^-24, gamma_n = n u / (1 - n u), n_i the open
keys of row i, n_j the open queries of key j, T = ceil(Lk / 32) key tiles.  They hold for any order of the sums, so torch's fp32
op on the CPU is inside them too.

  score     qs = fl(q * scale) with scale rounded to fp32 (2 roundings), then a fused-multiply-add chain over D terms:
            |s^ - s| <= E_ij = gamma_{D+2} scale sum_d |q_id| |k_jd|;  e_i = max over the open j of E_ij.
  weight    w_j = exp2(fl(fl(s^_j - m) * fl(log2 e))): the subtraction adds u |x| to the argument (x = s_j - m), the constant and
            the multiply 2 u |x|, v_exp_f32 is documented at 1 ulp = 2 u relative: 2 u + 3 u |x| <= c_exp u (1 + |x|), c_exp = 3.
            (v_exp_f32 may flush a result below 2^-126: TINY covers it.)  The rescale factors exp2((m - m') log2 e) of the later
            tiles carry the same kind of error; their arguments telescope to m_final - m_tile, so with x taken against the FINAL
            maximum the |x| part covers both, and their constant parts (c_exp u) and products (u) are T (1 + c_exp) roundings.
            Numerator and denominator of p_j = w_j / sum w each move by the score error: relative error of p_j
            eps_ij = 2 e_i + c_exp u (1 + |s_ij - m_i|).
  out       a perturbation eps_j of the weights moves o by sum_j p_j eps_j (v_j - o):
            |o^ - o| <= W_id + gamma_N (sum_j p_ij |v_jd| + |o_id|),  N = n_i + (1 + c_exp) T + 2 (sums, rescales, division),
            W_id = min( sum_j p_ij eps_ij (|v_jd| + |o_id|),  max_j eps_ij * sqrt(sum_j p_ij v_jd^2 - o_id^2) )
            (the second form is Jensen's bound of sum_j p_j |v_j - o|: a row with one open key has W = 0 and a bound of a few u).
  lse       lse^ = fl(m + logf(l^)): l^ has the relative error rho_i = e_i + sum_j p_ij c_exp u (1 + |s_ij - m_i|) +
            gamma_{n_i + (1 + c_exp) T}; logf within 3 ulp (the OpenCL limit); one rounding of the sum:
            |lse^ - lse| <= L_i = rho_i + 6 u |log l_i| + u |lse_i|.
  p (bwd)   p^ = exp2((s^ - lse^) log2 e): relative error eta_ij = E_ij + L_i + c_exp u (1 + |s_ij - lse_i|).
  dP        fma chain over D: |dP^ - dP| <= F_ij = gamma_D sum_d |dO_id| |v_jd|.
  delta     from the computed out: G_i = sum_d |dO_id| B_out_id + gamma_{D+1} sum_d |dO_id| |o_id|.  torch's softmax backward takes
            delta as sum_j p_j dP_j instead; its error is sum_j p_ij (eps_ij + gamma_{n_i+D+2}) sum_d |dO_id| |v_jd|.  The bound
            takes the larger of the two, so that both formulations are judged by one statement.
  dS        dS^ = p^ fl(dP^ - delta^):  |dS^ - dS| <= Z_ij = p_ij ((eta_ij + 2 u) |dP_ij - delta_i| + F_ij + G_i).
  dQ        scale (sum_j Z_ij |k_jd| + gamma_{n_i+2} sum_j |dS_ij| |k_jd|)     (a blocked key adds an exact zero)
  dK        scale (sum_i Z_ij |q_id| + gamma_{n_j+3} sum_i |dS_ij| |q_id|)     (qs carries 2 roundings)
  dV        sum_i p_ij eta_ij |dO_id| + gamma_{n_j+1} sum_i p_ij |dO_id|
All of these are first-order statements.  ``check_self_attn`` requires every relative error above to stay below 1e-2, so the
products of two of them are below 1 % of the bound, and multiplies the bounds by SECOND = 1.01.
"""
import numpy as np

U = 2.0 ** -24
C_EXP = 3.0
TILE = 32
SECOND = 1.01
TINY = 2.0 ** -100


def gamma(n):
    n = np.asarray(n, np.float64)
    return n * U / (1.0 - n * U)


def grad_pattern(shape, salt):
    """Deterministic fp32-exact pseudo-random values in [-2, 2): the upstream gradients of the cases (not stored)."""
    n = int(np.prod(shape))
    i = (np.arange(n, dtype=np.uint64) + np.uint64(salt)) * np.uint64(2654435761) % np.uint64(2 ** 32)
    return (((i >> np.uint64(16)).astype(np.float64) - 32768.0) / 16384.0).astype(np.float32).reshape(shape)


def _head(q, k, v, g, open_, scale, grads):
    """One (image, head): q (Lq, D), k, v (Lk, D), g (Lq, D) or None, open_ (Lq, Lk) bool -> values and bounds."""
    Lq, D = q.shape
    Lk = k.shape[0]
    T = -(-Lk // TILE)
    aq, ak, av = np.abs(q), np.abs(k), np.abs(v)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        s = np.where(open_, scale * (q @ k.T), -np.inf)
        Es = gamma(D + 2) * scale * (aq @ ak.T)
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
        gN = gamma(n + (1.0 + C_EXP) * T + 2.0)
        b_out = SECOND * (np.minimum(w_a, w_b) + gN[:, None] * (p @ av + np.abs(o))) + TINY
        res = {"out": np.where(dead[:, None], np.nan, o), "b_out": b_out, "rel": float(eps.max(initial=0.0))}
        if not grads:
            return res
        ag = np.abs(g)
        gv = ag @ av.T
        dP = g @ v.T
        F = gamma(D) * gv
        delta = (g * o).sum(1)
        G = np.maximum((ag * b_out).sum(1) + gamma(D + 1) * (ag * np.abs(o)).sum(1),
                       (p * (eps + gamma(n + D + 2.0)[:, None]) * gv).sum(1))
        ll = np.where(dead, 1.0, l)
        logl = np.log(ll)
        lse = m + logl
        rho = e + (p * C_EXP * U * (1.0 + x)).sum(1) + gamma(n + (1.0 + C_EXP) * T)
        Lb = rho + 6.0 * U * np.abs(logl) + U * np.abs(lse)
        eta = np.where(open_, Es + Lb[:, None] + C_EXP * U * (1.0 + np.abs(np.where(open_, s, 0.0) - lse[:, None])), 0.0)
        dd = np.where(open_, dP - delta[:, None], 0.0)
        dS = p * dd
        Z = p * ((eta + 2.0 * U) * np.abs(dd) + F + G[:, None])
        nk = open_.sum(0)
        aS = np.abs(dS)
        res.update(
            dq=scale * (dS @ k), b_dq=SECOND * scale * (Z @ ak + gamma(n + 2.0)[:, None] * (aS @ ak)) + TINY,
            dk=scale * (dS.T @ q), b_dk=SECOND * scale * (Z.T @ aq + gamma(nk + 3.0)[:, None] * (aS.T @ aq)) + TINY,
            dv=p.T @ g, b_dv=SECOND * ((p * eta).T @ ag + gamma(nk + 1.0)[:, None] * (p.T @ ag)) + TINY)
        res["rel"] = max(res["rel"], float(eta.max(initial=0.0)))
    return res


def ref64(problem, grads=True):
    """``problem``: q (Lq, B, E), k, v (Lk, B, E) float32 arrays, ``heads``, ``mask`` (Lq, Lk) bool or None (True = blocked),
    ``scale`` or None (D ** -0.5), ``gout`` (Lq, B, E) for the gradients.  -> dict of float64 arrays ``out`` (NaN in a fully
    blocked row), ``dq``, ``dk``, ``dv`` and their bounds ``b_out`` ...; ``rel``: the largest relative error term."""
    q, k, v = (np.asarray(problem[n], np.float64) for n in ("q", "k", "v"))
    (Lq, B, E), Lk, H = q.shape, k.shape[0], int(problem["heads"])
    D = E // H
    scale = float(D) ** -0.5 if problem.get("scale") is None else float(problem["scale"])
    mask = problem.get("mask")
    open_ = np.ones((Lq, Lk), bool) if mask is None else ~np.asarray(mask, bool)
    grads = grads and problem.get("gout") is not None
    g = np.asarray(problem["gout"], np.float64) if grads else None
    names = ["out", "b_out"] + (["dq", "b_dq", "dk", "b_dk", "dv", "b_dv"] if grads else [])
    res = {n_: np.zeros((Lq if n_[-1] in "tq" else Lk, B, E)) for n_ in names}
    res["rel"] = 0.0
    for b in range(B):
        for h in range(H):
            sl = slice(h * D, (h + 1) * D)
            r = _head(q[:, b, sl], k[:, b, sl], v[:, b, sl], g[:, b, sl] if grads else None, open_, scale, grads)
            for n_ in names:
                res[n_][:, b, sl] = r[n_]
            res["rel"] = max(res["rel"], r["rel"])
    return res


def judge_self_attn(problem, got, ref=None, dtype16=None):
    """-> {tensor: largest |got - ref| / bound over its elements (inf where a NaN is on one side only)} for the tensors in
    ``got`` (``out``, ``dq``, ``dk``, ``dv``), no element left out.  ``dtype16`` (``'fp16'`` / ``'bf16'``): the results were
    rounded once into that type, and every bound is widened to B + u16 (|ref| + B) + s16 (tests/msda_h16_ref.py)."""
    ref = ref or ref64(problem, grads=any(n in got for n in ("dq", "dk", "dv")))
    rep = {"rel": ref["rel"]}
    for name, val in got.items():
        want, bound = ref[name], ref["b_" + name]
        if dtype16 is not None:
            from msda_h16_ref import widen16
            with np.errstate(invalid="ignore"):
                bound = widen16(bound, want, dtype16)
        val = np.asarray(val, np.float64)
        assert val.shape == want.shape, (name, val.shape, want.shape)
        nan_w, nan_g = np.isnan(want), np.isnan(val)
        with np.errstate(invalid="ignore"):
            ratio = np.abs(val - want) / bound
        ratio[nan_w & nan_g] = 0.0
        ratio[nan_w ^ nan_g] = np.inf
        ratio[~np.isfinite(val) & ~nan_g] = np.inf
        rep[name] = float(ratio.max())
    return rep


def check_self_attn(problem, got, name="", ref=None, dtype16=None):
    """Every element of every tensor in ``got`` within its bound of the float64 statement (a fully blocked row: NaN on both
    sides).  Returns the report of ``judge_self_attn``."""
    rep = judge_self_attn(problem, got, ref, dtype16)
    assert rep["rel"] < 1e-2, f"{name}: a relative error term of {rep['rel']:.3g}: the first-order bounds do not apply"
    bad = {k_: v_ for k_, v_ in rep.items() if k_ != "rel" and not v_ <= 1.0}
    assert not bad, f"{name}: outside the bound (error / bound): {bad}"
    return rep


def table(name, rep):
    return f"{name:32s} " + " ".join(f"{k_}={v_:.3f}" for k_, v_ in rep.items() if k_ != "rel")
