"""Plain float64 statement of the cross-view consistency loss -- csrc/consis_loss.hip, forward and backward -- each value carried
as a (value, err) pair in the arithmetic of tests/assign_ref64.py, the checker that decides whether a result (from the GPU, from
the reference's float32 run, or from the fp32 numpy evaluation ``eval_f32`` below) is ADMISSIBLE against it, and mutants.

Test helper (not a conftest; imported by name like assign_ref64.py / loss_ref64.py).  Numpy only: no call into the library.

A ``problem`` is a dict: ``hs_v1`` / ``hs_v2`` lists of L float32 arrays (B, Q, D); ``bid`` (K,) float or int; ``idx`` (K,) int;
``weights`` (K,) float32 or None (= zeros, past the warm-up); ``pad_size``; ``scale`` (10); ``eps`` (1e-12); ``upstream`` (L,)
float32, the gradient flowing into each layer's loss.

What is stated (the kernel's expression order, csrc/consis_loss.hip):

    n = sqrtf(rowsum(x x)),  y = x / fmaxf(n, eps),  e = y1 - y2,  term_k = rowsum(e e) * w_k
    loss_l = (float)(sum_k term_lk [fp64] * (double)inv),  inv = scale / (float)(K D)
    coef_l = inv * upstream_l,  c = w_k * coef_l,  g = (2 c) e
    n1 >= eps:  grad = g / n1 - x1 * (((dot / n1) / n1) / n1),  dot = rowsum(x1 g);      n1 < eps:  grad = g / eps

Conventions: those of assign_ref64.py (u = 2^-24, one ulp = 2u per operation, ``sqrt_`` and ``div`` as given there, 2^-126 per
operation for a flushed subnormal, a bound that is not finite means "no statement", nothing scaled per test), plus:

  * reduction order and depth.  ``rowsum`` over the D elements of a row: lane j of the wave takes the float4 chunks j, j + 64,
    ... and adds (t0 + t1) + (t2 + t3) of each to its running sum, then the xor tree over 32, 16, 8, 4, 2, 1 lanes.  An element
    passes through ``consis_depth(D)`` = 2 + ceil(D / 256) + 6 additions (D = 256: 9), so the bound of a row sum is the sum of
    its elements' bounds + ((1 + 2u)^depth - 1) sum|t| + (D + 64) 2^-126.  A sum with at most one term that is not an exact zero
    is exact.  Over the rows the kernel adds the fp32 terms in fp64 (four rows per workgroup, the workgroups' slots by lanes and
    a tree): (K + 8) 2^-53 sum|term|, then one fp32 rounding of the product with inv.
  * parameters.  eps and scale are stated as the numbers themselves (1e-12, 10); the kernel holds the fp32 values the C ABI
    carries, and the difference is part of their error.
  * exact operations.  Two bitwise-identical rows give e = 0 exactly (the same expression of the same inputs); a product with
    an exact zero (weight 0, upstream 0) is an exact zero; sqrtf of an exact fp32 square is exact.  Such zeros carry no
    allowance: the gradient there must BE 0.
  * decisions.  The comparisons of a norm against eps are the only ones.  Intervals surely apart: decided.  Intervals that meet:
    fmaxf(n, eps) takes the larger error and the gradient admits the hull of both branches.  An exact tie (n an exact value equal
    to eps) follows torch's rule: >= passes, the n1 >= eps branch.
  * a pair with bid outside [0, B) or idx outside [0, pad_size) is not dereferenced: every layer's loss must be NaN, the pair
    has no gradient row, every other pair's row keeps its statement (K in the mean still counts the pair).
  * every element of the dense gradient outside the selected rows must be exactly zero, and hs_v2 receives no gradient.
"""
import numpy as np

from assign_ref64 import TINY, U, Inadmissible, _within, div, fmax, inp, mul, ratio, sqrt_, sub

F = np.float32
MUTANTS = ("no_eps_clamp", "mean_over_k", "weights_ignored", "no_scale", "h2_not_detached", "grad_doubled", "no_projection",
           "gate_gt", "unselected_nonzero")


def consis_depth(D):
    """additions an element of a row passes through: the chunk's pairwise adds, the lane's running sum, the xor tree"""
    chunks = D // 4
    return 2 + (chunks + 63) // 64 + 6


def scal(a, m):
    """times an exact power of two / selector: no rounding"""
    return a[0] * m, a[1] * np.abs(m)


def _param(c):
    """a parameter: the statement holds the number itself, the kernel the fp32 value the C ABI carries"""
    c = np.float64(c)
    return c, np.abs(np.float64(F(c)) - c)


def _sq(a):
    """x * x; exact where x is exact and the square is itself a normal fp32 number (correctly rounded: no rounding to charge)"""
    with np.errstate(all="ignore"):
        v, e = mul(a, a)
        exact = (a[1] == 0) & (v.astype(F).astype(np.float64) == v) & ((np.abs(v) >= TINY) | (v == 0))
    return v, np.where(exact, 0.0, e)


def _rowsum(t, D):
    v, e = t
    depth = consis_depth(D)
    s = v.sum(-1)
    nz = ((v != 0) | (e != 0)).sum(-1)
    rnd = ((1 + 2 * U) ** depth - 1) * np.abs(v).sum(-1) + (D + 64) * TINY
    return s, e.sum(-1) + np.where(nz <= 1, 0.0, rnd)


def _sqrt(a):
    """sqrt_ of assign_ref64, exact where the argument is exact and its root an fp32 number (IEEE sqrtf is correctly rounded)"""
    with np.errstate(all="ignore"):
        v, e = sqrt_(a)
        exact = (a[1] == 0) & (v.astype(F).astype(np.float64) == v) & (v * v == a[0])
    return v, np.where(exact, 0.0, e)


def valid_pairs(problem):
    bid, idx = np.asarray(problem["bid"], np.float64), np.asarray(problem["idx"], np.int64)
    B = problem["hs_v1"][0].shape[0]
    return (bid >= 0) & (bid < B) & (idx >= 0) & (idx < problem["pad_size"])


def _gather(problem):
    ok = valid_pairs(problem)
    b = np.where(ok, np.asarray(problem["bid"], np.float64), 0).astype(np.int64)
    q = np.where(ok, np.asarray(problem["idx"], np.int64), 0)
    x1 = np.stack([np.asarray(h, F)[b, q] for h in problem["hs_v1"]])          # (L, K, D)
    x2 = np.stack([np.asarray(h, F)[b, q] for h in problem["hs_v2"]])
    return ok, b, q, x1, x2


def _weights(problem, K):
    w = problem.get("weights")
    return np.zeros(K, F) if w is None else np.asarray(w, F).reshape(-1)


def statement(problem):
    """-> dict(loss=(v, e) (L,), grad=(v, e) (L, K, D) rows of the selected pairs, valid (K,), b, q, open (L, K))"""
    with np.errstate(all="ignore"):
        ok, b, q, x1f, x2f = _gather(problem)
        L, K, D = x1f.shape
        x1, x2 = inp(x1f), inp(x2f)
        eps = _param(problem.get("eps", 1e-12))
        n1, n2 = _sqrt(_rowsum(_sq(x1), D)), _sqrt(_rowsum(_sq(x2), D))
        d1, d2 = fmax(n1, eps), fmax(n2, eps)
        col = lambda a: (a[0][..., None], a[1][..., None])      # noqa: E731
        e = sub(div(x1, col(d1)), div(x2, col(d2)))
        same = (x1f == x2f).all(-1, keepdims=True)
        e = np.where(same, 0.0, e[0]), np.where(same, 0.0, e[1])
        w = inp(_weights(problem, K))
        term = mul(_rowsum(mul(e, e), D), w)
        tv, te = np.where(ok, term[0], 0.0), np.where(ok, term[1], 0.0)
        total = tv.sum(-1), te.sum(-1) + (K + 8) * 2.0 ** -53 * np.abs(tv).sum(-1)
        kd = float(K) * D
        inv = div(_param(problem.get("scale", 10.0)), (np.float64(kd), np.abs(np.float64(F(kd)) - kd)))
        loss = mul(total, inv)
        if not ok.all():
            loss = np.full(L, np.nan), np.zeros(L)
        # backward
        coef = mul(inv, inp(np.asarray(problem["upstream"], F).reshape(L)))
        c = mul((w[0][None, :], w[1][None, :]), (coef[0][:, None], coef[1][:, None]))
        g = mul(col(scal(c, 2.0)), e)
        dot = _rowsum(mul(x1, g), D)
        t = div(div(div(dot, n1), n1), n1)
        ga = sub(div(g, col(n1)), mul(x1, col(t)))
        gb = div(g, eps)
        tie = (n1[1] == 0) & (eps[1] == 0) & (n1[0] == eps[0])
        above = ((n1[0] - eps[0] > n1[1] + eps[1]) | tie)[..., None]
        below = (eps[0] - n1[0] > n1[1] + eps[1])[..., None]
        lo = np.minimum(ga[0] - ga[1], gb[0] - gb[1])
        hi = np.maximum(ga[0] + ga[1], gb[0] + gb[1])
        hull = 0.5 * (hi + lo), np.where(np.isfinite(hi - lo), 0.5 * (hi - lo), np.inf)
        gv = np.where(above, ga[0], np.where(below, gb[0], hull[0]))
        ge = np.where(above, ga[1], np.where(below, gb[1], hull[1]))
        ge = np.where(np.isfinite(gv), ge, np.inf)
        gv = np.where(np.isfinite(gv), gv, 0.0)
    return dict(loss=loss, grad=(gv, ge), valid=ok, b=b, q=q, open=~(above | below)[..., 0])


def check_consis(problem, losses, grads, grad_v2=None, name="consis", stmt=None):
    """Raise ``Inadmissible`` unless ``losses`` (L,) and the dense gradients ``grads`` (L arrays (B, Q, D)) are admissible.
    -> dict(loss_ratio, grad_ratio, no_statement): the largest |diff| / bound and the number of elements without one."""
    s = stmt or statement(problem)
    losses = np.asarray(losses, np.float64).reshape(-1)
    L = len(problem["hs_v1"])
    if losses.shape != (L,):
        raise Inadmissible(f"{name}: {losses.shape} losses for {L} layers")
    if not s["valid"].all():
        if not np.isnan(losses).all():
            raise Inadmissible(f"{name}: a pair outside the pad must make every loss NaN, got {losses!r}")
    else:
        _within(f"{name}.loss", losses, s["loss"])
    if grad_v2 is not None and any(np.any(np.asarray(g) != 0) for g in grad_v2):
        raise Inadmissible(f"{name}: hs_v2 is detached but received a gradient")
    ok, b, q = s["valid"], s["b"][s["valid"]], s["q"][s["valid"]]
    rows = np.stack([np.asarray(g, np.float64)[b, q] for g in grads])              # (L, K_valid, D)
    want = s["grad"][0][:, ok], s["grad"][1][:, ok]
    _within(f"{name}.grad", rows, want)
    for l, g in enumerate(grads):
        rest = np.array(g, np.float64)
        rest[b, q] = 0.0
        bad = ~(rest == 0)                                                          # NaN is not zero
        if bad.any():
            i = tuple(int(x) for x in np.argwhere(bad)[0])
            raise Inadmissible(f"{name}.grad[{l}]{list(i)}: {np.asarray(g)[i]!r} outside the selected rows, must be exactly 0")
    return dict(loss_ratio=0.0 if not ok.all() else ratio(losses, s["loss"]), grad_ratio=ratio(rows, want),
                no_statement=int((~np.isfinite(want[1])).sum() + (0 if not ok.all() else (~np.isfinite(s["loss"][1])).sum())))


# ------------------------------------------------------------------------------------------------------------------
# fp32 evaluation in the kernel's order, and mutants
# ------------------------------------------------------------------------------------------------------------------
def _rowsum32(t):
    """the wave's row sum of csrc/consis_loss.hip in float32: t (..., D) -> (...)"""
    D = t.shape[-1]
    C = D // 4
    t4 = t.reshape(t.shape[:-1] + (C, 4))
    s = (t4[..., 0] + t4[..., 1]) + (t4[..., 2] + t4[..., 3])
    per = (C + 63) // 64
    pad = np.zeros(s.shape[:-1] + (per * 64,), F)
    pad[..., :C] = s
    pad = pad.reshape(s.shape[:-1] + (per, 64))
    acc = np.zeros(s.shape[:-1] + (64,), F)
    for i in range(per):
        acc = acc + pad[..., i, :]
    lanes = np.arange(64)
    for sft in (32, 16, 8, 4, 2, 1):
        acc = acc + acc[..., lanes ^ sft]
    return acc[..., 0]


def _layersum64(terms):
    """the fp64 sum over rows: four rows per workgroup, the slots by lanes (stride 64) and the xor tree: (L, K) -> (L,)"""
    L, K = terms.shape
    nb = (K + 3) // 4
    t = np.zeros((L, nb * 4))
    t[:, :K] = terms
    t = t.reshape(L, nb, 4)
    part = ((t[..., 0] + t[..., 1]) + t[..., 2]) + t[..., 3]
    per = (nb + 63) // 64
    pad = np.zeros((L, per * 64))
    pad[:, :nb] = part
    pad = pad.reshape(L, per, 64)
    acc = np.zeros((L, 64))
    for i in range(per):
        acc = acc + pad[:, i, :]
    lanes = np.arange(64)
    for sft in (32, 16, 8, 4, 2, 1):
        acc = acc + acc[:, lanes ^ sft]
    return acc[:, 0]


def eval_f32(problem, mutant=None):
    """The kernels' arithmetic in numpy float32 -> (losses (L,) float32, [dense gradient (B, Q, D) float32] * L, grad_v2 or None)."""
    assert mutant is None or mutant in MUTANTS, mutant
    with np.errstate(all="ignore"):
        ok, b, q, x1, x2 = _gather(problem)
        L, K, D = x1.shape
        B, Q, _ = problem["hs_v1"][0].shape
        eps = F(problem.get("eps", 1e-12))
        scale = F(1.0 if mutant == "no_scale" else problem.get("scale", 10.0))
        w = np.ones(K, F) if mutant == "weights_ignored" else _weights(problem, K)
        n1, n2 = np.sqrt(_rowsum32(x1 * x1)), np.sqrt(_rowsum32(x2 * x2))
        clamp = (lambda n: n) if mutant == "no_eps_clamp" else (lambda n: np.maximum(n, eps))
        d1, d2 = clamp(n1)[..., None], clamp(n2)[..., None]
        e = x1 / d1 - x2 / d2
        term = (_rowsum32(e * e) * w).astype(np.float64)
        term = np.where(ok, term, np.nan)
        inv = scale / F(K if mutant == "mean_over_k" else float(K) * D)
        losses = (_layersum64(term) * np.float64(inv)).astype(F)
        coef = inv * np.asarray(problem["upstream"], F).reshape(L, 1)
        c2 = F(2.0) * (w[None, :] * coef)
        g = c2[..., None] * e
        dot = _rowsum32(x1 * g)
        nn = n1[..., None]
        t = (((dot / n1) / n1) / n1)[..., None]
        ga = g / nn if mutant == "no_projection" else g / nn - x1 * t
        gate = (nn > eps) if mutant == "gate_gt" else (nn >= eps)
        if mutant == "no_eps_clamp":
            gate = np.ones_like(gate)
        rows = np.where(gate, ga, g / eps).astype(F)
        if mutant == "grad_doubled":
            rows = rows * F(2.0)
        grads = []
        for l in range(L):
            dense = np.zeros((B, Q, D), F)
            dense[b[ok], q[ok]] = rows[l][ok]
            if mutant == "unselected_nonzero":
                dense[B - 1, Q - 1, D - 1] = F(1e-20)
            grads.append(dense)
        grad_v2 = None
        if mutant == "h2_not_detached":
            grad_v2 = []
            for l in range(L):
                dense = np.zeros((B, Q, D), F)
                dense[b[ok], q[ok]] = (-g[l] / d2[l])[ok]
                grad_v2.append(dense)
    return losses, grads, grad_v2


def table(case, rep):
    return f"{case:28s} loss {rep['loss_ratio']:6.3f}  grad {rep['grad_ratio']:6.3f} of the bound; {rep['no_statement']} without a statement"
