"""Plain float64 statement of csrc/pyramid_inputs.hip -- the level masks, the HW sine position rows with the level row, the valid
ratios, the encoder's reference points and the gradient of ``level_embed`` -- with ``pos`` and the gradient carried as (value,
err) pairs in the arithmetic of tests/assign_ref64.py, and the checker that decides whether a result (from the GPU, from
torch's fp32 evaluation of tests/pyramid_inputs_torch_restated.py, or from the recorded fixture) is ADMISSIBLE against it.

Test helper (not a conftest; imported by name like ref_points_ref64.py).  Numpy only.

Conventions: those of ref_points_ref64.py / assign_ref64.py (u = 2^-24; each of + - * / is charged one rounding, 2u |result| plus
2^-126; a bound that is not finite means "no statement"; nothing scaled per test), and:

  * the counts are exact integers; ``offset``, ``eps`` and ``scale`` are the fp32 numbers the C ABI carries; the two ``dim_t``
    tables are the fp32 tables the kernel is handed: exact.
  * y = ((cnt + offset) / (tot + eps)) * scale: four roundings; arg = y / dim_t[c]: one more.  The argument's error goes through
    with |d sin|, |d cos| <= 1; ``sinf`` / ``cosf``: ``SINCOS_ULPS`` = 2 ulp of the result, as in ref_points_ref64.py.
  * + level_embed[l][c] (exact: a number of its dtype): one rounding.  16-bit ``pos``: half an ulp of the format on top.
  * the gradient of ``level_embed[l][c]`` is a sum of n = N * h * w exact terms: any order of fp32 additions stays within
    (n - 1) * 2u * sum |term|; then the rounding to the dtype of ``level_embed``.
  * masks, valid ratios, reference points and the index tensors are fp32 / integer results of exact operands through correctly
    rounded operations: judged BIT FOR BIT against ``evaluate`` below (numpy's fp32 + - * / are the same IEEE operations).  A
    non-finite reference point must be non-finite of the same class (NaN, +inf, -inf).

``evaluate(case, dim_ty, dim_tx, mutant)`` is the op in numpy fp32, operation by operation; with a ``mutant`` it is the op with
one defect, which ``check`` has to reject on at least one case (tests/test_pyramid_inputs_ref.py).
"""
import numpy as np

from assign_ref64 import TINY, U, Inadmissible, add, bound, div, mul
from ref_points_ref64 import SINCOS_ULPS, exact, ratio, stored, ulp, within

F = np.float32
BLOCK, C = 128, 256
MUTANTS = ("sin_cos_swapped", "halves_swapped", "exclusive_counts", "eps_missing", "normalised_by_h", "wrong_level_row",
           "temperatures_swapped", "nearest_rounds", "ratios_from_whole_mask", "ratios_hw_order")


def dim_t(temperature, num_feats=BLOCK):
    """the table in float64 rounded to fp32: tests that have no torch table at hand (the statement takes whatever it is given)"""
    k = np.arange(num_feats)
    return (np.float64(temperature) ** (2 * (k // 2) / num_feats)).astype(F)


def nearest_src(d, in_size, out_size, mutant=None):
    """the fp32 nearest rule: min(int(floorf(d * (float(in) / out))), in - 1)"""
    p = F(d) * (F(in_size) / F(out_size))
    return min(int(np.rint(p) if mutant == "nearest_rounds" else np.floor(p)), in_size - 1)


def masks_of(case, mutant=None):
    """the level masks of a case: given, or from the image sizes by the nearest rule; [(N, h, w) bool]"""
    if case["masks"] is not None:
        return [np.asarray(m) != 0 for m in case["masks"]]
    (ih, iw), out = case["input"], []
    for h, w in case["shapes"]:
        si = np.array([nearest_src(i, ih, h, mutant) for i in range(h)])
        sj = np.array([nearest_src(j, iw, w, mutant) for j in range(w)])
        out.append(np.stack([(si[:, None] >= img_h) | (sj[None, :] >= img_w) for img_h, img_w in case["img_shapes"]]))
    return out


def counts(mask, mutant=None):
    """(cnt_y, tot_y, cnt_x, tot_x) of one (N, h, w) mask as int64, the totals broadcast to (N, h, w)"""
    valid = (~mask).astype(np.int64)
    cy, cx = valid.cumsum(1), valid.cumsum(2)
    ty, tx = np.broadcast_to(cy[:, -1:, :], cy.shape), np.broadcast_to(cx[:, :, -1:], cx.shape)
    if mutant == "exclusive_counts":
        cy, cx = cy - valid, cx - valid
    if mutant == "normalised_by_h":
        ty, tx = np.full_like(cy, mask.shape[1]), np.full_like(cx, mask.shape[2])
    return cy, ty, cx, tx


def _tables(case, dim_ty, dim_tx, mutant):
    return (dim_tx, dim_ty) if mutant == "temperatures_swapped" else (dim_ty, dim_tx)


def _level_row(case, lvl, mutant):
    le = case["level_embed"]
    if le is None:
        return None
    return le[(lvl + 1) % len(le)] if mutant == "wrong_level_row" else le[lvl]


def valid_ratios(masks, mutant=None, rule="reciprocal"):
    """(N, L, 2) fp32, [w, h]: bit for bit what the op stores.  ``rule``: how a count is divided by the level's side.  Stock torch
    divides a tensor by a Python number on the GPU by multiplying with the number's fp32 reciprocal ("reciprocal": the op's rule,
    it runs where the model runs) and on the CPU by an IEEE division ("divide": what a CPU run of the stock chain and the
    recorded fixture hold); the two differ by an ulp for some counts (5 / 12)."""
    out = []
    for m in masks:
        _, h, w = m.shape
        rows, cols = (~m[:, :, 0]).sum(1), (~m[:, 0, :]).sum(1)
        if mutant == "ratios_from_whole_mask":
            rows, cols = (~m).any(2).sum(1), (~m).any(1).sum(1)
        pair = [cols.astype(F) * (F(1) / F(w)), rows.astype(F) * (F(1) / F(h))] if rule == "reciprocal" else \
            [cols.astype(F) / F(w), rows.astype(F) / F(h)]
        out.append(np.stack(pair[::-1] if mutant == "ratios_hw_order" else pair, -1))
    return np.stack(out, 1).astype(F)


def reference_points(shapes, vr):
    """(N, S, L, 2) fp32 from the fp32 valid ratios, operation by operation"""
    vr = np.asarray(vr, F)
    with np.errstate(all="ignore"):
        per_level = []
        for lvl, (h, w) in enumerate(shapes):
            ii, jj = np.meshgrid(np.arange(h, dtype=F) + F(0.5), np.arange(w, dtype=F) + F(0.5), indexing="ij")
            ys = ii.reshape(-1)[None] / (vr[:, None, lvl, 1] * F(h))
            xs = jj.reshape(-1)[None] / (vr[:, None, lvl, 0] * F(w))
            per_level.append(np.stack((xs, ys), -1))
        pts = np.concatenate(per_level, 1).astype(F)
        return (pts[:, :, None] * vr[:, None]).astype(F)


def index_tensors(shapes):
    sh = np.asarray(shapes, np.int64).reshape(-1, 2)
    return sh, np.concatenate([[0], np.cumsum(sh[:, 0] * sh[:, 1])[:-1]]).astype(np.int64)


def evaluate(case, dim_ty, dim_tx, mutant=None, rule="reciprocal"):
    """The op in numpy fp32, one operation at a time -> the dict ``check`` reads (``pos`` and ``grad`` as fp32 arrays holding the
    values of their dtypes)."""
    from pyramid_inputs_cases import round_to
    enc, masks = case["enc"], masks_of(case, mutant)
    ty, tx = _tables(case, np.asarray(dim_ty, F), np.asarray(dim_tx, F), mutant)
    off, eps, scale = F(enc.get("offset", 0.0)), F(enc.get("eps", 1e-6)), F(enc.get("scale", 2 * np.pi))
    if mutant == "eps_missing":
        eps = F(0)
    even = np.arange(BLOCK) % 2 == (1 if mutant == "sin_cos_swapped" else 0)
    rows, grads = [], []
    n = masks[0].shape[0]
    with np.errstate(all="ignore"):
        for lvl, m in enumerate(masks):
            cy, tot_y, cx, tot_x = counts(m, mutant)
            y, x = cy.astype(F), cx.astype(F)
            if enc.get("normalize", False):
                y = ((y + off) / (tot_y.astype(F) + eps)) * scale
                x = ((x + off) / (tot_x.astype(F) + eps)) * scale
            ay, ax = y[..., None] / ty, x[..., None] / tx
            py, px = np.where(even, np.sin(ay), np.cos(ay)).astype(F), np.where(even, np.sin(ax), np.cos(ax)).astype(F)
            pos = np.concatenate((px, py) if mutant == "halves_swapped" else (py, px), -1).reshape(n, -1, C)
            row = _level_row(case, lvl, mutant)
            rows.append(pos if row is None else (pos + row.astype(F)).astype(F))
    vr = valid_ratios(masks, mutant, rule)
    sh, starts = index_tensors(case["shapes"])
    out = {"pos": round_to(np.concatenate(rows, 1), case["dtype"]), "mask_flatten": np.concatenate([m.reshape(n, -1) for m in masks], 1),
           "valid_ratios": vr, "reference_points": reference_points(case["shapes"], vr), "spatial_shapes": sh,
           "level_start_index": starts}
    if case["level_embed"] is not None:
        at = 0
        for h, w in case["shapes"]:
            grads.append(case["g"][:, at:at + h * w].astype(np.float64).sum((0, 1)))
            at += h * w
        out["grad"] = round_to(np.stack(grads).astype(F), case["le_dtype"])
    return out


def pos(case, dim_ty, dim_tx):
    """the (value, err) pair of ``pos`` (N, S, 256) as stored in the case's dtype"""
    enc, masks = case["enc"], masks_of(case)
    off, eps, scale = (exact(float(F(enc.get(k, d)))) for k, d in (("offset", 0.0), ("eps", 1e-6), ("scale", 2 * np.pi)))
    even = np.arange(BLOCK) % 2 == 0
    n, vals, errs = masks[0].shape[0], [], []
    with np.errstate(all="ignore"):
        for lvl, m in enumerate(masks):
            cy, tot_y, cx, tot_x = counts(m)
            halves = []
            for cnt, tot, table in ((cy, tot_y, dim_ty), (cx, tot_x, dim_tx)):
                coord = exact(cnt)
                if enc.get("normalize", False):
                    coord = mul(div(add(coord, off), add(exact(tot), eps)), scale)
                arg = div((coord[0][..., None], coord[1][..., None]), exact(np.asarray(table, np.float64)))
                v = np.where(even, np.sin(arg[0]), np.cos(arg[0]))
                halves.append((v, arg[1] + SINCOS_ULPS * ulp(v)))
            v = np.concatenate([halves[0][0], halves[1][0]], -1).reshape(n, -1, C)
            e = np.concatenate([halves[0][1], halves[1][1]], -1).reshape(n, -1, C)
            if case["level_embed"] is not None:
                v, e = add((v, e), exact(case["level_embed"][lvl]))
            vals.append(v)
            errs.append(e)
    return stored((np.concatenate(vals, 1), np.concatenate(errs, 1)), case["dtype"])


def grad(case):
    """the (value, err) pair of the gradient of ``level_embed`` (L, 256) as stored in its dtype"""
    vals, errs, at = [], [], 0
    for h, w in case["shapes"]:
        t = case["g"][:, at:at + h * w].astype(np.float64)
        at += h * w
        terms = t.shape[0] * t.shape[1]
        vals.append(t.sum((0, 1)))
        errs.append((terms - 1) * 2 * U * np.abs(t).sum((0, 1)) + TINY)
    return stored((np.stack(vals), np.stack(errs)), case["le_dtype"])


def same_bits(name, got, want):
    """Raise unless the two arrays are equal element for element, non-finite values of the same class"""
    got, want = np.asarray(got), np.asarray(want)
    if got.shape != want.shape:
        raise Inadmissible(f"{name}: shape {got.shape}, expected {want.shape}")
    if want.dtype.kind == "f":
        got = got.astype(want.dtype)
        with np.errstate(all="ignore"):
            bad = ~((got == want) | (np.isnan(got) & np.isnan(want)))
    else:
        bad = got.astype(np.int64) != want.astype(np.int64)
    if bad.any():
        i = tuple(int(x) for x in np.argwhere(bad)[0])
        raise Inadmissible(f"{name}{list(i)}: got {got[i]!r}, expected {want[i]!r} ({int(bad.sum())} elements differ)")


BITWISE = ("mask_flatten", "valid_ratios", "reference_points", "spatial_shapes", "level_start_index")


def check(case, got, dim_ty, dim_tx, name="", rule="reciprocal"):
    """Every result of a case in ``got`` (float / bool / integer arrays in the logical shapes; keys that are absent are not
    judged) against the statement.  Returns ``{key: worst |diff| / bound}`` for ``pos`` and ``grad``."""
    want = evaluate(case, dim_ty, dim_tx, rule=rule)
    out = {}
    for key in BITWISE:
        if key in got:
            same_bits(f"{name} {key}", got[key], want[key])
    if "pos" in got:
        a = pos(case, dim_ty, dim_tx)
        within(f"{name} pos", got["pos"], a)
        out["pos"] = ratio(got["pos"], a)
    if "grad" in got and case["level_embed"] is not None:
        a = grad(case)
        within(f"{name} grad", got["grad"], a)
        out["grad"] = ratio(got["grad"], a)
    return out


def table(name, ratios):
    return f"  {name:24s} " + "  ".join(f"{k} {v:.3f}" for k, v in ratios.items())
