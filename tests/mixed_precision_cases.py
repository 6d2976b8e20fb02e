"""Inputs of the mixed-precision tests of the transformer mirrors (tests/test_mixed_precision_ref.py on the CPU,
tests/test_gpu_mixed_precision.py on the GPU): ``add_norm``, ``self_attn`` and ``query_select`` under ``torch.autocast`` and as
``.half()`` modules.  Test helper (not a conftest); numpy, and torch on the CPU for the rounding.

Every 16-bit operand is a float32 array that holds 16-bit values exactly (``round16`` of tests/msda_h16_ref.py), so the float64
statements see exactly what the GPU sees and their bounds need no input term: a result that leaves in fp32 keeps the fp32
bound B of add_norm_ref64 / self_attn_ref64 / query_select_ref64, one that leaves in 16 bits gets B + u16 (|ref| + B) + s16.

Contexts: ``autocast_bf16`` / ``autocast_fp16`` (fp32 parameters, fp32 residual stream, 16-bit branch outputs) and
``half_module`` (autocast disabled, everything fp16), as in tests/test_gpu_msda_h16.py.
"""
import functools

import numpy as np

import add_norm_cases as AC
import add_norm_ref64 as AR
import query_select_ref64 as QR
import self_attn_cases as SC
import self_attn_ref64 as SR
from msda_h16_ref import MAX16, round16

F = np.float32
CONTEXTS = ("autocast_bf16", "autocast_fp16", "half_module")
DTYPE16 = {"autocast_bf16": "bf16", "autocast_fp16": "fp16", "half_module": "fp16"}


def autocast(context):
    """the torch context manager of a context name"""
    import torch
    if context == "half_module":
        return torch.autocast("cuda", enabled=False)
    return torch.autocast("cuda", dtype=torch.bfloat16 if context == "autocast_bf16" else torch.float16)


# ------------------------------------------------------------------------------------------------------------------
# 1. add_layer_norm: which operand is 16-bit
# ------------------------------------------------------------------------------------------------------------------
#           name            residual  pos      where it occurs
COMBOS = {"res32":         ("f32",    None),   # encoder norm1, decoder norm1 / norm3
          "res32_pos32":   ("f32",    "f32"),  # encoder norm2 with the next layer's query
          "res32_pos16":   ("f32",    "h16"),  # decoder forward_sa with the MLP's query_pos
          "bare":          (None,     None),   # an adopted enc_output_norm
          "res16":         ("h16",    None),   # LayerNorm.forward on two 16-bit operands
          "res16_pos16":   ("h16",    "h16")}  # a .half() layer with pos
AUTOCAST_COMBOS = ("res32", "res32_pos32", "res32_pos16", "bare", "res16")
HALF_COMBOS = ("res16", "res16_pos16", "bare")
BASES = ("r65_transposed", "r2051_contiguous")


def add_norm_names():
    return [(b, c, ctx) for ctx in CONTEXTS for c in (HALF_COMBOS if ctx == "half_module" else AUTOCAST_COMBOS) for b in BASES]


@functools.lru_cache(maxsize=None)
def add_norm_case(base, combo, context):
    """The case ``base`` of add_norm_cases with ``x`` (the branch) rounded to the context's 16-bit type and ``residual`` /
    ``pos`` as ``combo`` says.  ``half_module``: weight, bias and the upstream gradients are 16-bit numbers too.  The case
    carries ``kinds``: operand -> 'f32' | 'h16' | None."""
    dt = DTYPE16[context]
    src = AC.cases()[base]
    res_kind, pos_kind = COMBOS[combo]
    half = context == "half_module"
    assert not half or "f32" not in (res_kind, pos_kind)
    rng = np.random.default_rng(700 + len(base) + len(combo))
    r16 = lambda a: round16(a, dt)
    as_kind = lambda a, kind: None if kind is None else (r16(a) if kind == "h16" else np.array(a, F))
    gy = src["gy"] if src["gy"] is not None else rng.standard_normal(src["x"].shape).astype(F)
    gq = (src["gq"] if src["gq"] is not None else rng.standard_normal(src["x"].shape).astype(F)) if pos_kind else None
    case = dict(name=f"{base}/{combo}/{context}", shape=src["shape"], layout=src["layout"], eps=src["eps"], dtype16=dt,
                x=r16(src["x"]), residual=as_kind(src["residual"], res_kind), pos=as_kind(src["pos"], pos_kind),
                weight=r16(src["weight"]) if half else src["weight"], bias=r16(src["bias"]) if half else src["bias"],
                gy=r16(gy) if half else gy, gq=(r16(gq) if half else gq) if gq is not None else None,
                kinds=dict(x="h16", residual=res_kind, pos=pos_kind, weight="h16" if half else "f32",
                           bias="h16" if half else "f32"), context=context)
    # The special rows.  Row 0 (equal values) survives the rounding.  Row 1 -- mean 4096, spread 1e-2 -- rounds to the constant
    # 4096 in either 16-bit type; the statement says nothing about a row whose variance interval reaches zero, and dweight sums
    # over all rows.  So the spread moves to where the formats can hold it: into the residual (4096 + 1e-2 z is formed in fp32
    # by the kernel: the same cancellation), or, without a residual, to 64 z, a multiple of the 16-bit spacing at 4096.
    rows = case["x"].reshape(-1, 256)
    if case["residual"] is not None:
        case["residual"].reshape(-1, 256)[1] = as_kind(1e-2 * rng.standard_normal(256), res_kind)
    else:
        rows[1] = r16(4096.0 + 64.0 * rng.standard_normal(256))
    assert (rows[0] == F(1.375)).all() and np.abs(rows[1] - 4096.0).max() < 512.0
    for v in case.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return case


@functools.lru_cache(maxsize=None)
def add_norm_reference(base, combo, context):
    return AR.ref64(add_norm_case(base, combo, context))


def derived_dtypes(case):
    """{result: 'f32' | 'h16'} as the issue derives them from torch's rules (the GPU test asserts stock torch agrees).  Under
    enabled CUDA autocast ``layer_norm`` is on the fp32 list: ``y`` is fp32, and so is ``y + pos``.  With autocast disabled both
    are the promotion of their operands.  A gradient has its leaf's dtype; ``dx`` is x's, ``dx_res`` the residual's."""
    k = case["kinds"]
    if case["context"] == "half_module":
        y = "f32" if k["residual"] == "f32" else "h16"
        q = None if k["pos"] is None else ("f32" if "f32" in (y, k["pos"]) else "h16")
    else:
        y, q = "f32", (None if k["pos"] is None else "f32")
    return dict(y=y, q=q, dx=k["x"], dx_res=k["residual"], dpos=k["pos"], dweight=k["weight"], dbias=k["bias"])


def judged_dtypes(kinds, dt):
    """{output of check_add_norm: 'fp16' | 'bf16'} for the results that left in 16 bits"""
    return {n: dt for n, kind in kinds.items() if kind == "h16"}


def rounded_once(case, mutant=None):
    """add_norm_ref64.eval_f32 of the case, each result rounded once into its derived dtype; or one of the two mutants:
    ``stream_narrowed`` -- a ``y`` (and the ``q`` made from it) that should leave in fp32 passed through the 16-bit type;
    ``rounded_twice`` -- ``q = round16(round16(y) + pos)`` where the contract rounds the fp32 ``y + pos`` once.
    -> (got, changed): ``changed`` names the results the mutant changed (empty without one)."""
    dt, want = case["dtype16"], derived_dtypes(case)
    raw = AR.eval_f32(case)
    raw["dx_res"] = raw["dx"]
    assert mutant in (None, "stream_narrowed", "rounded_twice"), mutant
    good = {n: (round16(v, dt) if want[n] == "h16" else np.asarray(v, F)) for n, v in raw.items() if want.get(n) is not None}
    got = dict(good)
    if mutant == "stream_narrowed" and want["y"] == "f32":
        got["y"] = round16(raw["y"], dt)
        if want["q"] is not None:
            got["q"] = (got["y"] + case["pos"].reshape(-1, 256)).astype(F)
    elif mutant == "rounded_twice" and want["q"] == "h16":
        got["q"] = round16(round16(raw["y"], dt) + case["pos"].reshape(-1, 256), dt)
    got["kinds"] = {n: want[n] for n in good}
    return got, [n for n in good if got[n].tobytes() != good[n].tobytes()]


def check_add_norm16(case, got, ref, name=None):
    """``got``: any of y, q, dx, dx_res, dweight, dbias as float arrays plus ``kinds``: {result: 'f32' | 'h16'} saying how each
    left.  Every element within B (fp32) or B + u16 (|ref| + B) + s16 (16-bit).  -> {result: worst err / bound}"""
    name = name or case["name"]
    kinds = got["kinds"]
    rep = {}
    for n, v in got.items():
        if n == "kinds":
            continue
        stated = "dx" if n == "dx_res" else n
        rep[n] = AR.check_add_norm(case, {stated: v}, f"{name} [{n} as {kinds[n]}]", ref,
                                   judged_dtypes({stated: kinds[n]}, case["dtype16"]))[stated]
    return rep


# ------------------------------------------------------------------------------------------------------------------
# 2. masked_attention on 16-bit operands
# ------------------------------------------------------------------------------------------------------------------
ATTN_CASES = ("dn_edges_in_tiles", "lq_ne_lk", "L33_B3_masked", "large_scores")
DTYPES = ("fp16", "bf16")


@functools.lru_cache(maxsize=None)
def attn_case(name, dt):
    """the self_attn case with q, k, v and gout rounded to the 16-bit type (a packed case: the rounding of one (L, B, 3E)
    buffer is the rounding of its three parts)"""
    p = dict(SC.cases()[name])
    for n in ("q", "k", "v", "gout"):
        p[n] = round16(p[n], dt)
        p[n].setflags(write=False)
    return p


@functools.lru_cache(maxsize=None)
def attn_reference(name, dt):
    return SR.ref64(attn_case(name, dt))


def attn_reach(name, dt):
    """{result: max (|ref| + B)}: what a result can be at most before its rounding (the fp16 range condition)"""
    r = attn_reference(name, dt)
    return {n: float(np.nanmax(np.abs(r[n]) + r["b_" + n])) for n in ("out", "dq", "dk", "dv")}


# ------------------------------------------------------------------------------------------------------------------
# 3. select_queries on 16-bit logits: ties under load
# ------------------------------------------------------------------------------------------------------------------
SMALL4 = [(9, 13), (5, 7), (3, 4), (2, 2)]                    # the pyramid of tests/test_region_grid_host.py, S = 168
SEL_N, SEL_C, SEL_D = 2, 8, 256
BAND = [(1.0, 1.0), (0.7, 0.8)]                                # image 1 is padded below 70 % of the rows, right of 80 % of the columns


def band_mask(shapes, fracs):
    rows = []
    for fh, fw in fracs:
        parts = []
        for H, W in shapes:
            m = np.ones((H, W), bool)
            m[:int(np.ceil(H * fh)), :int(np.ceil(W * fw))] = False
            parts.append(m.reshape(-1))
        rows.append(np.concatenate(parts))
    return np.stack(rows)


def tie_stats(keys, k):
    """keys (N, S) -> per image (straddle, tied): whether the keys at ranks k - 1 and k (0-based, key descending) are equal, and
    how many of the first k ranks share their key with a neighbouring rank"""
    out = []
    for row in np.asarray(keys, np.float64):
        s = -np.sort(-row)
        same = s[1:] == s[:-1]
        tied = np.zeros(len(s), bool)
        tied[1:] |= same
        tied[:-1] |= same
        out.append((bool(s[k - 1] == s[k]), int(tied[:k].sum())))
    return out


@functools.lru_cache(maxsize=None)
def select_case(dt):
    """N(0, 2) logits rounded to the 16-bit type on the SMALL4 pyramid; padded and invalid tokens carry one and the same row
    (what a zeroed ``output_memory`` row gives: the head's bias), as in the model.  ``k`` is the smallest k >= 16 at which some
    image has a tie across rank k and more than k / 4 tied ranks in its top k; tests/test_mixed_precision_ref.py asserts both."""
    rng = np.random.default_rng(31)
    mask = band_mask(SMALL4, BAND)
    p = QR.proposals(mask, SMALL4)
    S = mask.shape[1]
    logits = (rng.standard_normal((SEL_N, S, SEL_C)) * np.sqrt(2.0)).astype(F)
    logits[~p["valid"]] = np.linspace(-2.0, 1.5, SEL_C, dtype=F)
    logits = round16(logits, dt)
    keys = QR.keys_of(logits)
    k = next((k for k in range(16, S) if any(st and tied > k / 4 for st, tied in tie_stats(keys, k))), None)
    memory = rng.standard_normal((SEL_N, S, SEL_D)).astype(F)
    reg = (rng.standard_normal((SEL_N, S, 4)) * 0.5).astype(F)
    return dict(mask=mask, shapes=SMALL4, p=p, logits=logits, keys=keys, k=k, memory=memory, reg=reg, dtype16=dt)


def select_numpy(keys, k):
    """the first k of (key descending, token ascending) in plain numpy on finite keys: a stable sort of the negated keys"""
    keys = np.asarray(keys, np.float64)
    return np.stack([np.argsort(-row, kind="stable")[:k] for row in keys]).astype(np.int64)


__all__ = ["MAX16", "round16"]
