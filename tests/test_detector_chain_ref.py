"""CPU: the judges of the detector chain (tests/detector_chain_cases.py) before the GPU uses them.

  1. ``msda_torch_restated``'s core against the float64 statement with its fp64 bounds, and the restated module against the
     fixture the reference's own module produced (the tolerances tests/test_gpu_module.py uses for it).
  2. The conditions the committed seeds must meet: the lattice margin of the ``init`` encoder samples on the ``window``
     pyramid, the cap on the share of samples the kink judgement leaves out, a top-k without ties.
  3. The handoff mistakes of ``MUTANTS``, each run as the "side" in fp32: every one breaks the rule on a judged tensor.

Run with -s for the figures.
"""
import functools

import numpy as np
import pytest
import torch

import detector_chain_cases as C
import msda_ref64 as R
import msda_torch_restated as MT
from test_gpu_add_norm import FACTOR
from test_gpu_msda_bounds import _spec, make_case

TINY = [(5, 7), (3, 4)]
OP_CASES = {
    "points_offmap": _spec(TINY, 2, Lq=30, M=2, D=4, spread="offmap", seed=301),
    "points_mask": _spec(TINY, 2, Lq=30, M=2, D=4, io="fused", mask="band", spread=2.0, seed=302),
    "boxes_mask": _spec(TINY, 2, Lq=30, M=2, D=4, io="fused", ref_dim=4, mask="band", spread="offmap", seed=303),
    "encoder_points": _spec(TINY, 2, M=2, D=4, io="fused", spread=1.0, seed=304),
}


def _leaf(a):
    return torch.from_numpy(np.asarray(a, np.float64)).requires_grad_(True)


@pytest.mark.parametrize("name", list(OP_CASES))
def test_restated_op_against_the_float64_statement(name):
    s = OP_CASES[name]
    c = make_case(s)
    shapes = torch.from_numpy(c["shapes"])
    starts = torch.cat([shapes.new_zeros(1), (shapes[:, 0] * shapes[:, 1]).cumsum(0)[:-1]])
    value = _leaf(c["value"])
    masked = value if c["mask"] is None else value.masked_fill(torch.from_numpy(c["mask"])[..., None, None], 0.0)
    gout = torch.from_numpy(c["gout"].astype(np.float64))
    if s["io"] == "fused":
        ref, off, logits = torch.from_numpy(c["ref"].astype(np.float64)), _leaf(c["off"]), _leaf(c["logits"])
        loc = MT.locations_of(ref, off, shapes, s["P"])
        attn = torch.softmax(logits, -1).view(off.shape[:5])
        want = R.fused(c["value"], c["shapes"], c["ref"], c["off"], c["logits"], c["gout"], mask=c["mask"])
        leaves = {"grad_value": value, "grad_offsets": off, "grad_logits": logits}
    else:
        loc, attn = _leaf(c["loc"]), _leaf(c["attn"])
        want = R.msda(c["value"], c["shapes"], c["loc"], c["attn"], c["gout"])
        leaves = {"grad_value": value, "grad_loc": loc, "grad_attn": attn}
    out = MT.core(masked, shapes, starts, loc, attn)
    out.backward(gout)
    worst = {"out": R.check(name, "out", out.detach().numpy(), want["out"], np.float64)}
    for what, leaf in leaves.items():
        worst[what] = R.check(name, what, leaf.grad.numpy(), want[what], np.float64)
    if c["mask"] is not None:
        assert (value.grad.numpy()[c["mask"]] == 0.0).all()
    print(f"\n{name}: worst err / fp64 bound " + ", ".join(f"{k} {v:.3f}" for k, v in worst.items()))


def _pack(t):
    a = t.detach().numpy().reshape(-1)
    return a if a.size <= 4096 else a[::5]


@pytest.mark.parametrize("case", ["enc_ref2", "enc_ref2_mask", "dec_ref4", "dec_ref4_mask"])
def test_restated_module_against_the_reference_fixture(case):
    from conftest import Golden
    from oracle.gen_golden import MODULE_D32_CASES, module_d32_inputs
    g = Golden("msda_module_d32.npz")[case]
    name, refdim, use_mask, encoder = next(c for c in MODULE_D32_CASES if c[0] == case)
    levels, sd, query, src, ref, mask, gout = module_d32_inputs(name, refdim, use_mask, encoder)
    m = MT.MSDeformAttn(256, 4, 8, 4)
    m.load_state_dict(sd, strict=True)
    shapes = torch.as_tensor(levels, dtype=torch.long)
    starts = torch.cat([shapes.new_zeros(1), (shapes[:, 0] * shapes[:, 1]).cumsum(0)[:-1]])
    q, s_, r = [t.clone().requires_grad_(True) for t in (query, src, ref)]
    out = m(q, r, s_, shapes, starts, mask)
    out.backward(gout)
    np.testing.assert_allclose(out.detach().numpy(), g["out"], rtol=1e-4, atol=2e-5)

    def close(got, key, rel=2e-4):
        want = g[key]
        np.testing.assert_allclose(_pack(got), want, rtol=1e-3, atol=rel * np.abs(want).max(), err_msg=key)
    close(q.grad, "g_query")
    close(s_.grad, "g_src")
    close(r.grad, "g_ref")
    for k, p in m.named_parameters():
        close(p.grad, "g_" + k)


def test_restated_module_has_the_product_modules_keys_and_initialisation():
    """the keys are compared on the CPU without the native library: the product's module is not constructed here"""
    m = MT.MSDeformAttn(256, 4, 8, 4)
    assert list(m.state_dict()) == ["sampling_offsets.weight", "sampling_offsets.bias", "attention_weights.weight",
                                    "attention_weights.bias", "value_proj.weight", "value_proj.bias", "output_proj.weight",
                                    "output_proj.bias"]
    bias = m.sampling_offsets.bias.detach().view(8, 4, 4, 2)
    assert torch.equal(bias[0, :, :, 0], torch.arange(1.0, 5.0).expand(4, 4)) and (bias[0, :, :, 1] == 0).all()
    assert float(bias.abs().max(-1)[0].sub(torch.arange(1.0, 5.0)).abs().max()) < 1e-6
    assert not m.sampling_offsets.weight.any() and not m.attention_weights.weight.any()


# ------------------------------------------------------------------------------------------------------------------ the chain
@functools.lru_cache(maxsize=None)
def _sides(pyramid, state):
    """the stock fp32 chain and the float64 chain on the CPU, computed once and left unchanged"""
    model, inp = C.build_model(state), C.inputs(pyramid)
    stock = C.run_side(model, C.stock_forward, inp)
    f64 = C.run_side(C.in_float64(model), C.stock_forward, inp, exact=True, idx=stock["idx"])
    return model, inp, stock, f64


def test_offset_biases_are_exact_in_both_16_bit_types():
    for state in C.STATES:
        for _, att in C.attentions(C.build_model(state)):
            b = att.sampling_offsets.bias.detach()
            assert torch.equal(b.bfloat16().float(), b) and torch.equal(b.half().float(), b)
            assert float(b.abs().max()) <= 3.0 and not (b == b.round()).any()


@pytest.mark.parametrize("state", C.STATES)
@pytest.mark.parametrize("pyramid", list(C.PYRAMIDS))
def test_chain_conditions(pyramid, state):
    model, inp, stock, f64 = _sides(pyramid, state)
    rows = C.rule_report(stock, stock, f64, f64)
    assert all(scale > 0 for _, _, scale in rows), "the fp32 chain differs from the float64 chain in every judged tensor"
    # top-k: the first K + 1 keys are KEY_GAP apart, in fp32 and in float64, so two fp32 sides select the same tokens
    gaps = [C.topk_gap(dict(s["fwd"])["logits"]) for s in (stock, f64)]
    assert min(gaps) > C.KEY_GAP, gaps
    assert dict(stock["fwd"])["logits"].sub(dict(f64["fwd"])["logits"]).abs().max() < C.KEY_GAP / 10
    assert len(set(stock["idx"][0].tolist())) == C.K
    if state == "init":
        shares = C.left_out_shares(stock, f64)
        assert max(shares.values()) <= C.LEFT_OUT_CAP, shares
        if pyramid == "window":
            margin = C.lattice_margin(f64["taps"])
            assert margin >= C.MARGIN - 1e-9, margin
            print(f"\n{pyramid} {state}: lattice margin of the encoder samples {margin:.6f} px")
        print(f"\n{pyramid} {state}: left-out share per call " + ", ".join(f"{k} {v:.2e}" for k, v in shares.items()))
    print(f"\n{pyramid} {state}: smallest top-k key gap fp32 {gaps[0]:.3e}, f64 {gaps[1]:.3e}; worst |fp32 - f64| "
          + ", ".join(f"{n} {scale:.2e}" for n, _, scale in rows))


def test_stock_chain_passes_its_own_rule_from_another_summation_order():
    """The rule is satisfiable: the fp32 chain evaluated with the batch reversed (other GEMM rows, the same arithmetic) stays
    within FACTOR of the fp32 chain's own error."""
    model, inp, stock, f64 = _sides("patch", "init")
    flipped = dict(inp, feats=[t.flip(0) for t in inp["feats"]], pos=inp["pos"].flip(0), pad=inp["pad"].flip(0), vr=inp["vr"].flip(0),
                   seeds=[s.flip(1) if s.dim() == 4 else s.flip(0) for s in inp["seeds"]])
    side = C.run_side(model, C.stock_forward, flipped)
    unflip = lambda n, t: t if t is None or n.startswith("grad ") and not n.startswith(("grad feats", "grad pos")) else \
        t.flip(1) if n == "boxes" else t.flip(0)
    for which in ("fwd", "grads"):
        side[which] = [(n, unflip(n, t)) for n, t in side[which]]
    assert torch.equal(side["idx"].flip(0), stock["idx"])
    for which in ("fwd", "grads"):
        rows = C.rule_report(side, stock, f64, f64, which, skip=C.offset_gradient_names(model) if which == "grads" else ())
        assert not C.broken(rows, FACTOR), [r for r in rows if r[0] in C.broken(rows, FACTOR)]


@pytest.mark.parametrize("mutant", C.MUTANTS)
def test_mutant_breaks_the_rule(mutant):
    """patch pyramid (its valid ratios differ between the levels), ``init`` state (its gradients are judged)"""
    model, inp, stock, f64 = _sides("patch", "init")
    side = C.run_side(model, C.stock_forward, inp, mutant=mutant)
    f64_side = f64 if torch.equal(side["idx"], stock["idx"]) else \
        C.run_side(C.in_float64(model), C.stock_forward, inp, exact=True, idx=side["idx"])
    bad = C.broken(C.rule_report(side, stock, f64_side, f64, "fwd"), FACTOR)
    bad += C.broken(C.rule_report(side, stock, f64_side, f64, "grads", skip=C.offset_gradient_names(model)), FACTOR)
    print(f"\n{mutant}: {len(bad)} tensors break the rule, first {bad[:3]}")
    assert bad, f"{mutant} passes the rule on every judged tensor"
