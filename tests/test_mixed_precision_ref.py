"""CPU: the judges of the mixed-precision tests (tests/mixed_precision_cases.py; GPU side: tests/test_gpu_mixed_precision.py).

* the 16-bit-widened bounds of add_norm_ref64 accept the honest fp32 evaluation of every mixed case, rounded once into the
  dtype each result leaves in, and reject the two ways a mirror can get the dtype handling wrong: an fp32 residual stream
  passed through the 16-bit type, and a ``q`` rounded twice;
* the logits of the selection case really tie where the test says they do;
* the plain numpy selection is the total order of query_select_ref64.topk;
* no fp16 attention case comes near the range of fp16, so overflow can excuse nothing.
"""
import numpy as np
import pytest

import add_norm_ref64 as AR
import mixed_precision_cases as M
import query_select_ref64 as QR
from msda_h16_ref import MAX16, S16, U16

NAMES = M.add_norm_names()
IDS = ["/".join(n) for n in NAMES]


@pytest.mark.parametrize("base,combo,context", NAMES, ids=IDS)
def test_fp32_evaluation_rounded_once_is_admissible(base, combo, context):
    case = M.add_norm_case(base, combo, context)
    got, changed = M.rounded_once(case)
    assert not changed and set(got["kinds"]) >= {"y", "dx", "dweight", "dbias"}
    ref = M.add_norm_reference(base, combo, context)
    assert all(np.isfinite(ref[n][1]).all() for n in ("dweight", "dbias")), "a row without a statement leaves dweight unjudged"
    rep = M.check_add_norm16(case, got, ref)
    print(AR.table(case["name"], rep))
    want = M.derived_dtypes(case)
    if context != "half_module":
        assert want["y"] == "f32" and want["q"] in (None, "f32") and want["dx"] == "h16"
        assert (want["dx_res"] == "f32") == (M.COMBOS[combo][0] == "f32")


@pytest.mark.parametrize("mutant", ["stream_narrowed", "rounded_twice"])
@pytest.mark.parametrize("base,combo,context", NAMES, ids=IDS)
def test_mutants_are_rejected_with_case_and_element_named(base, combo, context, mutant):
    case = M.add_norm_case(base, combo, context)
    got, changed = M.rounded_once(case, mutant)
    want = M.derived_dtypes(case)
    if mutant == "stream_narrowed":                   # differs wherever y is to leave in fp32: every autocast case
        assert ("y" in changed) == (want["y"] == "f32") and (context == "half_module" or "y" in changed)
    else:                                             # differs wherever q leaves in 16 bits: the .half() layer with pos
        assert changed == (["q"] if want["q"] == "h16" else [])
    ref = M.add_norm_reference(base, combo, context)
    for n in changed:
        with pytest.raises(AR.Inadmissible, match=rf"{base}/{combo}/{context} \[{n} as {want[n]}\]: {n}\[\d+, \d+\]: got"):
            M.check_add_norm16(case, {n: got[n], "kinds": got["kinds"]}, ref)


def test_both_mutants_are_exercised():
    hit = {m: sum(bool(M.rounded_once(M.add_norm_case(*n), m)[1]) for n in NAMES) for m in ("stream_narrowed", "rounded_twice")}
    assert hit["stream_narrowed"] == sum(n[2] != "half_module" for n in NAMES) and hit["rounded_twice"] == len(M.BASES)


def test_default_judges_are_unchanged():
    a = (np.array([1.0, -2.0]), np.array([1e-6, 2e-6]))
    assert AR.widen16(a, None) is a and QR.widen16(a[1], a[0], None) is a[1]
    w = AR.widen16(a, "bf16")[1]
    assert np.array_equal(w, a[1] + U16["bf16"] * (np.abs(a[0]) + a[1]) + S16["bf16"])
    assert np.array_equal(QR.widen16(a[1], a[0], "fp16"), a[1] + U16["fp16"] * (np.abs(a[0]) + a[1]) + S16["fp16"])


@pytest.mark.parametrize("dt", M.DTYPES)
def test_selection_case_ties_across_rank_k_and_inside_the_top_k(dt):
    c = M.select_case(dt)
    k = c["k"]
    assert k is not None and 16 <= k < c["keys"].shape[1]
    stats = M.tie_stats(c["keys"], k)
    print(f"{dt}: k = {k}, (tie across rank k, tied ranks in the top k) per image = {stats}, "
          f"distinct keys per image = {[len(np.unique(r)) for r in c['keys']]}")
    assert any(straddle and tied > k / 4 for straddle, tied in stats)
    assert np.array_equal(c["logits"], M.round16(c["logits"], dt)) and np.isfinite(c["keys"]).all()
    # the tie matters: the token at rank k has the key of the one at rank k - 1, so only the token order decides
    idx = QR.topk(c["keys"], k + 1)
    n = next(i for i, (straddle, tied) in enumerate(stats) if straddle and tied > k / 4)
    assert c["keys"][n, idx[n, k - 1]] == c["keys"][n, idx[n, k]] and idx[n, k - 1] < idx[n, k]


@pytest.mark.parametrize("dt", M.DTYPES)
def test_numpy_selection_is_the_statements_total_order(dt):
    c = M.select_case(dt)
    for k in (1, c["k"], c["keys"].shape[1]):
        assert np.array_equal(M.select_numpy(c["keys"], k), QR.topk(c["keys"], k))
    assert not np.array_equal(M.select_numpy(c["keys"], c["k"]), QR.topk(c["keys"], c["k"], "ties_high"))


@pytest.mark.parametrize("name", M.ATTN_CASES)
def test_no_fp16_attention_result_can_reach_the_range_of_fp16(name):
    reach = M.attn_reach(name, "fp16")
    print(name, {k: f"{v:.4g}" for k, v in reach.items()})
    assert all(v < MAX16["fp16"] for v in reach.values()), reach
    p = M.attn_case(name, "fp16")
    assert all(np.isfinite(p[n]).all() and np.abs(p[n]).max() < MAX16["fp16"] for n in ("q", "k", "v", "gout"))
