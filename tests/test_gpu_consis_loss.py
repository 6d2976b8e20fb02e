"""GPU: semi_detr_amd.consistency_loss (csrc/consis_loss.hip) against the float64 statement tests/consis_ref64.py: every loss and
every element of every dense gradient through ``check_consis`` (the zeros outside the selected rows must be exactly zero), on the
cases of tests/consis_cases.py and of the fixture recorded from the reference.  Before each call NaN-filled buffers of the
gradient's size are freed into the caching allocator, so an element the backward does not write shows.

torch.autograd.gradcheck is not used: it would run the kernel in fp32 against finite differences, which is what the float64
statement with its derived bounds replaces."""
import math
import os

import numpy as np
import pytest
import torch

import consis_cases as C
import consis_ref64 as R
import consis_torch_restated as T

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"


def _poison(shape):
    junk = [torch.full(shape, float("nan"), dtype=torch.float32, device=DEV) for _ in range(2)]
    del junk


def _grad(leaf):
    """a leaf whose loss is unused has no gradient under torch (the restatement); the Function writes its zeros"""
    return leaf.grad if leaf.grad is not None else torch.zeros_like(leaf)


def _inputs(case, mode):
    """-> (leaves that receive the gradient, hs_v1, hs_v2, function leaf gradients -> list of (B, Q, D) arrays)"""
    b1 = [torch.from_numpy(b).to(DEV) for b in case["buf_v1"]]
    b2 = [torch.from_numpy(b).to(DEV) for b in case["buf_v2"]]
    if mode == "views":                                  # as the reference builds them: (Q, B, D) buffers, transposed
        leaves = [b.requires_grad_(True) for b in b1]
        return leaves, [b.transpose(0, 1) for b in leaves], [b.transpose(0, 1) for b in b2], \
            lambda: [_grad(b).transpose(0, 1).cpu().numpy() for b in leaves]
    if mode == "contiguous":
        leaves = [b.transpose(0, 1).contiguous().requires_grad_(True) for b in b1]
        return leaves, leaves, [b.transpose(0, 1).contiguous() for b in b2], lambda: [_grad(b).cpu().numpy() for b in leaves]
    assert mode == "stacked"
    leaf = torch.stack([b.transpose(0, 1) for b in b1]).requires_grad_(True)
    return [leaf], leaf, torch.stack([b.transpose(0, 1) for b in b2]), lambda: list(leaf.grad.cpu().numpy())


def _meta(case, bid_dtype=torch.float32):
    return {"pad_size_1": case["pad_size"], "known_bid_1": torch.from_numpy(case["bid"]).to(DEV).to(bid_dtype),
            "map_known_indice_1": torch.from_numpy(case["idx"]).to(DEV),
            "loss_weights": torch.from_numpy(case["weights"]).to(DEV).reshape(-1, 1)}


def run(case, mode="views", bid_dtype=torch.float32, warm_up=True, fn=None):
    """losses (L,) and dense gradients of sum_l upstream_l loss_l (a layer with upstream 0 is left out of the sum: unused)"""
    import semi_detr_amd as s
    fn = fn or s.consistency_loss
    leaves, hs1, hs2, grads = _inputs(case, mode)
    Q, B, D = case["buf_v1"][0].shape
    _poison((len(case["buf_v1"]), B, Q, D))
    kw = {} if fn is not s.consistency_loss else {"eps": case["eps"]}
    out = fn(hs1, hs2, _meta(case, bid_dtype), warm_up=warm_up, scale=case["scale"], **kw)
    assert list(out) == [f"consis_loss.d{l}" for l in range(len(case["buf_v1"]))]
    assert all(v.dim() == 0 and v.dtype == torch.float32 for v in out.values())
    total = sum(float(c) * out[f"consis_loss.d{l}"] for l, c in enumerate(case["upstream"]) if c != 0)
    total.backward()
    return torch.stack(list(out.values())).detach().cpu().numpy(), grads()


def checked(case, name, **kw):
    p = C.problem(case)
    if not kw.get("warm_up", True):
        p["weights"] = None
    losses, grads = run(case, **kw)
    rep = R.check_consis(p, losses, grads, name=name)
    print(R.table(name, rep))
    return losses, grads, rep


def _same(a, b):
    return a[0].tobytes() == b[0].tobytes() and all(x.tobytes() == y.tobytes() for x, y in zip(a[1], b[1]))


def test_ordinary_case_views_contiguous_and_stacked_agree_bitwise():
    case = C.ordinary()
    res = {}
    for mode in ("views", "contiguous", "stacked"):
        losses, grads, rep = checked(case, "ordinary " + mode, mode=mode)
        assert rep["no_statement"] == 0
        assert not np.any(grads[4])                       # the unused layer
        res[mode] = (losses, grads)
    assert _same(res["views"], res["contiguous"]) and _same(res["views"], res["stacked"])
    again = run(case)                                     # determinism: bit-identical, forward and backward
    assert _same(res["views"], again)


@pytest.mark.parametrize("name", sorted(C.FIXTURE_CASES))
def test_fixture_cases_from_the_reference(name):
    z = np.load(os.path.join(ROOT, "tests", "golden", "consis_loss.npz"))
    case = C.FIXTURE_CASES[name]()
    stored = z[f"{name}.buf_v1"]
    case["buf_v1"] = [stored[l].copy() for l in range(stored.shape[0])]
    stored = z[f"{name}.buf_v2"]
    case["buf_v2"] = [stored[l].copy() for l in range(stored.shape[0])]
    for k in ("bid", "idx", "weights", "upstream"):
        case[k] = z[f"{name}.{k}"]
    losses, grads, rep = checked(case, "fixture " + name)
    assert rep["no_statement"] == 0
    # and directly against the reference's float64 numbers, within the same bounds
    s = R.statement(C.problem(case))
    assert np.all(np.abs(losses - z[f"{name}.loss64"]) <= s["loss"][1] + 1e-12 * np.abs(z[f"{name}.loss64"]))
    b, q = case["bid"].astype(np.int64), case["idx"]
    rows = np.stack([g[b, q] for g in grads])
    want = z[f"{name}.grad64"]
    assert np.all(np.abs(rows - want) <= s["grad"][1] + 1e-12 * np.abs(want).max(-1, keepdims=True))


@pytest.mark.parametrize("build", [C.k1, C.k_odd, C.k1500, C.d64, C.d36, C.d1024], ids=lambda f: f.__name__)
def test_sizes_and_widths(build):
    """K = 1; K = 15 (no multiple of the four rows of a workgroup); K = 1500 (375 partial slots per layer: the multi-workgroup
    reduce); D = 64, D = 36 (the tail of the row loop) and D = 1024 (several chunks per lane) on the generic path"""
    losses, grads, rep = checked(build(), build.__name__)
    assert rep["no_statement"] == 0 and np.isfinite(losses).all()


def test_known_bid_fp32_and_int64_agree_bitwise():
    case = C.k_odd()
    a = run(case, bid_dtype=torch.float32)
    b = run(case, bid_dtype=torch.int64)
    assert _same(a, b)
    R.check_consis(C.problem(case), *b)


def test_weights():
    case = C.image_weight_zero()
    losses, grads, rep = checked(case, "image weight 0")
    for g in grads:
        assert not np.any(g[1]) and np.any(g[0])          # image 1's rows: exactly zero
    # past the warm-up: every weight zero
    case = C.ordinary()
    losses, grads, rep = checked(case, "warm_up=False", warm_up=False)
    assert losses.tobytes() == np.zeros_like(losses).tobytes()
    assert all(not np.any(g) and not np.isnan(g).any() for g in grads)


def test_identical_views_give_exact_zeros():
    losses, grads, rep = checked(C.identical_views(), "identical views")
    assert not np.any(losses) and all(not np.any(g) for g in grads)


def test_rows_below_the_eps_clamp():
    case = C.below_eps()
    s = R.statement(C.problem(case))
    assert not s["open"].any()                            # a zero row, norm 1e-13, squares that flush: all decided
    losses, grads, rep = checked(case, "below eps")
    assert rep["no_statement"] == 0 and np.isfinite(losses).all()
    g = grads[0]
    assert np.abs(g[0, 0]).max() > 1e6                    # g / eps: large, finite
    assert np.isfinite(g).all()


def test_exact_tie_takes_the_ge_branch():
    case = C.exact_tie()
    losses, grads, rep = checked(case, "exact tie")
    assert rep["no_statement"] == 0
    assert grads[0][0, 1, 7] == 0                         # the projection cancels the one non-zero element; g / eps would not


def test_out_of_range_pair_is_guarded():
    case = C.out_of_range()                               # idx in [pad_size, Q): inside the tensor
    losses, grads, rep = checked(case, "out of range")
    assert np.isnan(losses).all()
    assert not np.any(grads[0][0, case["pad_size"] + 2])   # the pair's own row: past the pad, zeros
    torch.cuda.synchronize()                              # the call succeeded


def test_k_zero_gives_nan_losses_and_zero_gradients():
    import semi_detr_amd as s
    hs1 = [torch.randn(2, 6, 64, device=DEV, requires_grad=True) for _ in range(2)]
    hs2 = [torch.randn(2, 6, 64, device=DEV) for _ in range(2)]
    meta = {"pad_size_1": 5, "known_bid_1": torch.zeros(0, device=DEV), "map_known_indice_1": torch.zeros(0, dtype=torch.int64, device=DEV),
            "loss_weights": torch.zeros(0, 1, device=DEV)}
    out = s.consistency_loss(hs1, hs2, meta)
    assert all(torch.isnan(v) for v in out.values())
    sum(out.values()).backward()
    assert all(h.grad is not None and not h.grad.any() for h in hs1)


def test_agreement_with_the_torch_restatement():
    """Both sides against each other within the SUM of their bounds.  The kernel's bound is the statement's.  The restatement
    runs the same fp32 expression per element with torch's reductions: its row sums are trees of no more depth than the
    statement's, and its mean over K D elements is an fp32 tree of at most ceil(log2(K D)) + 4 roundings (four elements per
    thread) where the kernel adds in fp64, so its loss gets that many more ulps of |loss|."""
    case = C.ordinary()
    p = C.problem(case)
    s = R.statement(p)
    mine = run(case)
    theirs = run(case, fn=T.consistency_loss)
    R.check_consis(p, *mine, name="kernel", stmt=s)
    K, D = len(case["bid"]), case["buf_v1"][0].shape[2]
    extra = (math.ceil(math.log2(K * D)) + 4) * 2 * R.U * np.abs(s["loss"][0])
    assert np.all(np.abs(mine[0] - theirs[0]) <= 2 * s["loss"][1] + extra)
    b, q = case["bid"].astype(np.int64), case["idx"]
    for l in range(len(mine[1])):
        assert np.all(np.abs(mine[1][l][b, q] - theirs[1][l][b, q]) <= 2 * s["grad"][1][l])
        rest = theirs[1][l].copy()
        rest[b, q] = 0
        assert not np.any(rest)
