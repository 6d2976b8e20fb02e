"""CPU: the float64 statement of the two-stage query selection (tests/query_select_ref64.py) against the fixtures the
reference's own functions produced (tests/golden/query_select.npz, tools/gen_query_select_golden.py), its fp32 bounds against
the reference's float32 run, mutants, and the C-ABI surface."""
import numpy as np
import pytest

import query_select_ref64 as R
from conftest import Golden

G = Golden("query_select.npz")
NAMES = G.names()
CASES = {n: G[n] for n in NAMES}
SELECT = [n for n in NAMES if "logits" in CASES[n]]


def diff(a, b):
    """|a - b| with equal infinities and NaN against NaN counting as 0."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    with np.errstate(invalid="ignore"):
        return np.where((a == b) | (np.isnan(a) & np.isnan(b)), 0.0, np.abs(a - b))


def shapes_of(c):
    return [tuple(int(v) for v in r) for r in c["shapes"]]


def statement(c, mutant=None):
    """The statement's view of a case with given head outputs -> dict of everything the fixture records."""
    mask = c["mask"].astype(bool)
    p = R.proposals(mask, shapes_of(c), mutant)
    k = int(c["k"])
    logits = c["logits"].astype(np.float32)
    keys = R.keys_of(logits, mutant)
    idx = R.topk(keys, k, mutant)
    outmem = R.masked_memory(c["memory"], p["valid"])
    coord = c["reg"].astype(np.float64) + p["prop"]
    g = R.gather(idx, coord, p["prop"], p["bound"], outmem, mutant)
    return dict(p=p, keys=keys, idx=idx, outmem=outmem, coord=coord, g=g, k=k)


def test_cases_cover_what_the_issue_lists():
    lv = {len(CASES[n]["shapes"]) for n in NAMES}
    assert {1, 4, 5} <= lv
    assert any((CASES[n]["shapes"][:, 1] == 1).any() for n in NAMES)
    assert any(not CASES[n]["mask"].any() for n in NAMES) and any(int(CASES[n]["k"]) == CASES[n]["mask"].shape[1] for n in NAMES)
    assert {CASES[n]["logits"].shape[2] for n in SELECT} >= {1, 20, 80}
    assert any(np.isnan(CASES[n]["logits"]).any() for n in SELECT)
    c = CASES["h50_no_mask"]                     # the 0.5 / 50 boundary: row 0 is invalid, row 1 is not
    v = np.isfinite(c["prop32"][0, :, 0]).reshape(50, 84)
    assert not v[0].any() and v[1, 1:-1].all()
    c = CASES["k_gt_valid"]
    assert (np.isfinite(c["prop32"][..., 0]).sum(1) < int(c["k"])).all()
    c = CASES["masked_level"]
    assert c["mask"][1, 36:].all()


@pytest.mark.parametrize("name", NAMES)
def test_valid_flags_equal_the_fp32_run_exactly_and_values_lie_within_bounds(name):
    c = CASES[name]
    p = R.proposals(c["mask"].astype(bool), shapes_of(c))
    ref_valid = ~np.isinf(c["prop32"]).all(-1)
    assert np.array_equal(p["valid"], ref_valid)
    assert np.array_equal(np.isinf(c["prop32"]), np.isinf(p["prop"])) and np.array_equal(np.isinf(c["prop64"]), np.isinf(p["prop"]))
    fin = np.isfinite(p["prop"])
    assert np.abs(p["prop"][fin] - c["prop64"][fin]).max(initial=0) <= 1e-13
    err = np.abs(c["prop32"].astype(np.float64)[fin] - p["prop"][fin])
    assert (err <= p["bound"][fin]).all(), (err / p["bound"][fin]).max()
    assert np.array_equal(R.masked_memory(c["memory"], p["valid"]), c["outmem32"])


@pytest.mark.parametrize("name", SELECT)
def test_selection_rule_values_and_gradients(name):
    c = CASES[name]
    s = statement(c)
    keys, idx, k = s["keys"], s["idx"], s["k"]
    n = np.arange(idx.shape[0])[:, None]
    # the reference's top-k VALUES exactly (NaN == NaN), its index SET outside tied keys
    assert np.array_equal(keys[n, idx].astype(np.float32), c["topv32"], equal_nan=True)
    uniq = R.unique_key_slots(keys, idx)
    assert np.array_equal(idx[uniq], c["topi32"][uniq]) and np.array_equal(idx[uniq], c["topi64"][uniq])
    g = s["g"]
    u3 = uniq[..., None]
    assert np.where(u3, diff(g["refpoint"], c["dec_ref64"][:, -k:]), 0).max() <= 1e-12
    assert np.array_equal(np.where(u3, g["tgt"], 0), np.where(u3, c["hs_enc32"], 0))
    assert np.where(u3, diff(g["ref_enc"], c["ref_enc64"]), 0).max() <= 1e-15
    assert np.where(u3, diff(g["init_box"], c["init64"]), 0).max() <= 1e-15
    # the reference's float32 run within the derived bounds
    assert (np.where(u3, diff(c["init32"], g["init_box"]), 0) <= g["init_bound"]).all()
    ref32 = R.sigmoid(c["dec_ref32"][:, -k:].astype(np.float64))
    assert (np.where(u3, diff(c["ref_enc32"], ref32), 0) <= 4 * R.U * ref32 + R.TINY).all()
    if "dn_ref" in c:
        assert np.array_equal(c["dec_ref32"][:, :-k], c["dn_ref"]) and np.array_equal(c["dec_tgt32"][:, :-k], c["dn_tgt"])
    assert np.array_equal(c["dec_tgt32"][:, -k:], np.broadcast_to(c["tgt_embed"], c["dec_tgt32"][:, -k:].shape))
    # gradients: where every selected key is unique the fixture's float64 gradients are the statement's
    if uniq.all():
        S = keys.shape[1]
        g1, g2 = R.grad_pattern(g["tgt"].shape, 1), R.grad_pattern(g["ref_enc"].shape, 2)
        gc, _, gm = R.gather_backward(idx, S, g["ref_enc"], None, g1, g2)
        assert diff(gc, c["g_reg"]).max() <= 1e-14
        assert np.array_equal(np.where(s["p"]["valid"][..., None], gm, 0).astype(np.float64), c["g_memory"])


def _disagrees(mutant):
    for name in SELECT:
        c = CASES[name]
        s = statement(c, mutant)
        if mutant in ("ge", "no_half", "swap_wh", "extents", "linear_scale", "fill_zero"):
            if not np.array_equal(s["p"]["valid"], ~np.isinf(c["prop32"]).all(-1)):
                return True
            fin = np.isfinite(c["prop64"])
            if not np.array_equal(np.isinf(s["p"]["prop"]), ~fin) or np.abs(s["p"]["prop"][fin] - c["prop64"][fin]).max() > 1e-9:
                return True
        else:
            n = np.arange(s["idx"].shape[0])[:, None]
            good = statement(c)
            uniq = R.unique_key_slots(good["keys"], good["idx"])
            if not np.array_equal(s["keys"][n, s["idx"]].astype(np.float32), c["topv32"], equal_nan=True):
                return True
            if mutant == "ties_high" and not np.array_equal(s["idx"], good["idx"]):
                return True
            if np.where(uniq[..., None], diff(s["g"]["init_box"], c["init64"]), 0).max() > 1e-9:
                return True
    return False


@pytest.mark.parametrize("mutant", R.MUTANTS)
def test_mutants_are_rejected(mutant):
    assert _disagrees(mutant), mutant


def test_unmutated_statement_is_not_rejected():
    assert not _disagrees(None)


def test_torch_restatement_reproduces_the_fixture():
    """The probe's baseline is the reference's op sequence; it is checked here so that it is not this project's code."""
    import torch
    import query_select_torch_restated as T
    for name in SELECT:
        c = CASES[name]
        mem = torch.from_numpy(c["memory"])
        om, prop = T.gen_proposals(mem, torch.from_numpy(c["mask"].astype(bool)), torch.from_numpy(c["shapes"]))
        assert np.array_equal(om.numpy(), c["outmem32"]) and np.array_equal(prop.numpy(), c["prop32"])
        lg = torch.from_numpy(c["logits"].astype(np.float32))
        coord = torch.from_numpy(c["reg"].astype(np.float32)) + prop
        idx, ref, init, tgt, ref_enc = T.select(lg, coord, prop, om, int(c["k"]))
        uniq = R.unique_key_slots(R.keys_of(c["logits"]), idx.numpy())
        assert np.array_equal(idx.numpy()[uniq], c["topi32"][uniq])
        u3 = uniq[..., None]
        assert np.array_equal(np.where(u3, init.numpy(), 0), np.where(u3, c["init32"], 0))
        assert np.array_equal(np.where(u3, tgt.numpy(), 0), np.where(u3, c["hs_enc32"], 0))
        assert np.array_equal(np.where(u3, ref_enc.numpy(), 0), np.where(u3, c["ref_enc32"], 0), equal_nan=True)


def test_cabi_surface_and_argument_errors():
    import semi_detr_amd
    names = ["semidetr_qsel_proposals_f32", "semidetr_qsel_proposals_backward_f32", "semidetr_qsel_topk_workspace_bytes",
             "semidetr_qsel_topk_f32", "semidetr_qsel_gather_f32", "semidetr_qsel_gather_backward_f32"]
    assert set(names) <= set(semi_detr_amd._lib.SIGNATURES)
    lib = semi_detr_amd._lib.lib()
    assert lib.semidetr_abi_version() == 7
    assert lib.semidetr_qsel_proposals_f32(None, None, None, None, None, 1, 1, 1, 1, None, None, None) == -1
    assert b"null pointer" in lib.semidetr_last_error()
    assert lib.semidetr_qsel_topk_workspace_bytes(4, 22223) == 4 * 22223 * 4 and lib.semidetr_qsel_topk_workspace_bytes(0, 5) == 0
    one = 16                                            # non-null, never dereferenced: the checks below fail on the host
    assert lib.semidetr_qsel_topk_f32(None, one, 2, 100, 80, 101, one, 800, one, one) == -1 and b"out of range" in lib.semidetr_last_error()
    assert lib.semidetr_qsel_topk_f32(None, one, 1, 9000, 80, 5000, one, 36000, one, one) == -2      # SEMIDETR_E_TOOLARGE
    assert lib.semidetr_qsel_topk_f32(None, one, 2, 100, 80, 10, one, 8, one, one) == -1 and b"workspace" in lib.semidetr_last_error()
    import ctypes
    sh = (ctypes.c_int64 * 2)(3, 4)
    rc = lib.semidetr_qsel_proposals_f32(None, one, one, ctypes.cast(sh, ctypes.c_void_p), None, 1, 1, 13, 4, one, one, one)
    assert rc == -1 and b"hold 12 tokens" in lib.semidetr_last_error()
    assert lib.semidetr_qsel_proposals_f32(None, one, one, None, None, 1, 1, 12, 4, one, one, one) == -1
    assert lib.semidetr_qsel_proposals_f32(None, one, one, ctypes.cast(sh, ctypes.c_void_p), None, 9, 1, 12, 4, one, one, one) == -1
    assert lib.semidetr_qsel_gather_backward_f32(None, one, None, None, one, None, 1, 12, 3, 4, one, one) == -1
    assert lib.semidetr_qsel_gather_f32(None, one, one, one, one, 8192, 5000, 4096, 4, one, one, one, one) == -2      # N * k >= 2^24
    import torch
    from semi_detr_amd import query_select as Q
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        Q.gen_encoder_output_proposals(torch.zeros(1, 12, 4), torch.zeros(1, 12, dtype=torch.bool), [(3, 4)])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        Q.select_queries(torch.zeros(1, 12, 2), torch.zeros(1, 12, 4), torch.zeros(1, 12, 4), torch.zeros(1, 12, 4), 3)
    with pytest.raises(NotImplementedError, match="transformer.py:1317"):
        Q.gen_encoder_output_proposals(torch.zeros(1, 12, 4), torch.zeros(1, 12, dtype=torch.bool), [(3, 4)], torch.zeros(2))
    from semi_detr_amd import registry
    done, skipped = registry.bind_query_select()
    assert sorted(done + skipped) == ["DINOTransformer.two_stage_queries", "gen_encoder_output_proposals"]
