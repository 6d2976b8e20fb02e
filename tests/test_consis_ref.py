"""CPU: the float64 statement of the consistency loss (tests/consis_ref64.py) against the fixture recorded from the reference's
own loop (tests/golden/consis_loss.npz, tools/gen_consis_golden.py), the admissibility of the fp32 evaluations, the mutants, the
host-side argument checks of the C ABI and the mirror's refusal of CPU tensors.  No GPU."""
import ctypes
import os

import numpy as np
import pytest
import torch

import consis_cases as C
import consis_ref64 as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def golden():
    z = np.load(os.path.join(ROOT, "tests", "golden", "consis_loss.npz"))
    return {k: z[k] for k in z.files}


def _fixture_case(golden, name):
    """the case rebuilt from the STORED inputs (and equal to what consis_cases builds today)"""
    case = C.FIXTURE_CASES[name]()
    for k in ("buf_v1", "buf_v2"):
        stored = golden[f"{name}.{k}"]
        np.testing.assert_array_equal(stored, np.stack(case[k]))
        case[k] = [stored[l] for l in range(stored.shape[0])]
    for k in ("bid", "idx", "weights", "upstream"):
        np.testing.assert_array_equal(golden[f"{name}.{k}"], case[k])
    assert int(golden[f"{name}.pad_size"]) == case["pad_size"]
    return case


def _dense(case, rows):
    """dense gradients from the fixture's selected rows (the rest is zero: its checksum is asserted)"""
    Q, B, D = case["buf_v1"][0].shape
    b, q = case["bid"].astype(np.int64), case["idx"]
    out = []
    for l in range(rows.shape[0]):
        d = np.zeros((B, Q, D), rows.dtype)
        d[b, q] = rows[l]
        out.append(d)
    return out


@pytest.mark.parametrize("name", sorted(C.FIXTURE_CASES))
def test_statement_agrees_with_the_reference_in_float64(golden, name):
    case = _fixture_case(golden, name)
    s = R.statement(C.problem(case))
    want_l, want_g = golden[f"{name}.loss64"], golden[f"{name}.grad64"]
    assert want_l.dtype == np.float64 and want_g.dtype == np.float64
    assert np.all(np.abs(s["loss"][0] - want_l) <= 1e-12 * np.abs(want_l).max())
    top = np.abs(want_g).max(-1, keepdims=True)
    assert np.all(np.abs(s["grad"][0] - want_g) <= 1e-12 * top)
    assert np.all(golden[f"{name}.rest64"] == 0) and np.all(golden[f"{name}.rest32"] == 0)
    assert golden[f"{name}.grad_v2_abs"] == 0                       # the other view is detached


@pytest.mark.parametrize("name", sorted(C.FIXTURE_CASES))
def test_fp32_evaluations_are_admissible(golden, name):
    case = _fixture_case(golden, name)
    p = C.problem(case)
    s = R.statement(p)
    losses, grads, g2 = R.eval_f32(p)
    rep = R.check_consis(p, losses, grads, g2, name=name, stmt=s)
    print(R.table(name + " eval_f32", rep))
    assert rep["no_statement"] == 0
    rep = R.check_consis(p, golden[f"{name}.loss32"], _dense(case, golden[f"{name}.grad32"]), name=name, stmt=s)
    print(R.table(name + " reference fp32", rep))
    assert rep["no_statement"] == 0


def test_column_weights_of_the_reference(golden):
    """The reference multiplies the (K, D) squared differences by ``loss_weights.unsqueeze(-1)``.  With a (K,) vector that is the
    per-row weight stated here.  With the (K, 1) column that prepare_unsup_cdn produces it broadcasts to (K, K, D) and the loss is
    mean(w) x the unweighted mean: equal for uniform weights, different for mixed ones (tools/gen_consis_golden.py)."""
    name = "uniform_weights"
    np.testing.assert_allclose(golden[f"{name}.loss64_column"], golden[f"{name}.loss64"], rtol=1e-14)
    np.testing.assert_allclose(golden[f"{name}.grad64_column"], golden[f"{name}.grad64"], rtol=1e-12, atol=0)
    name = "image_weight_zero"
    case = _fixture_case(golden, name)
    w = case["weights"]
    assert 0 < w.mean() < 1
    ones = R.statement(C.problem(case, weights=np.ones_like(w)))
    np.testing.assert_allclose(golden[f"{name}.loss64_column"], w.astype(np.float64).mean() * ones["loss"][0], rtol=1e-12)
    assert not np.allclose(golden[f"{name}.loss64_column"], golden[f"{name}.loss64"], rtol=1e-3)


def _ordinary_with_zero_row():
    case = C.ordinary()
    for buf in case["buf_v1"]:
        buf[1, 0, :] = 0                                 # (b 0, q 1): selected
    return case


def test_ordinary_case_has_a_statement_everywhere_and_rejects_the_mutants():
    case = C.ordinary()
    p = C.problem(case)
    s = R.statement(p)
    assert not s["open"].any() and s["valid"].all()
    assert np.isfinite(s["loss"][1]).all() and np.isfinite(s["grad"][1]).all()
    rep = R.check_consis(p, *R.eval_f32(p), stmt=s)
    assert rep["no_statement"] == 0 and rep["loss_ratio"] <= 1 and rep["grad_ratio"] <= 1
    assert np.all(s["grad"][0][4] == 0) and np.all(s["grad"][1][4] == 0)      # the unused layer: an exact zero
    for mutant in R.MUTANTS:
        if mutant in ("no_eps_clamp", "gate_gt"):
            continue                                     # bit-identical on rows far above eps: their cases follow
        with pytest.raises(R.Inadmissible):
            R.check_consis(p, *R.eval_f32(p, mutant=mutant), stmt=s)
    # the clamp: the ordinary case with one selected row of hs_v1 zeroed (0 / 0 without it)
    case = _ordinary_with_zero_row()
    p = C.problem(case)
    s = R.statement(p)
    assert not s["open"].any()
    assert R.check_consis(p, *R.eval_f32(p), stmt=s)["no_statement"] == 0
    with pytest.raises(R.Inadmissible):
        R.check_consis(p, *R.eval_f32(p, mutant="no_eps_clamp"), stmt=s)


def test_exact_tie_follows_torch_and_rejects_the_strict_gate():
    case = C.exact_tie()
    p = C.problem(case)
    s = R.statement(p)
    assert not s["open"].any()                          # the tie is exact: decided, no hull
    rep = R.check_consis(p, *R.eval_f32(p), stmt=s)
    assert rep["no_statement"] == 0
    with pytest.raises(R.Inadmissible):
        R.check_consis(p, *R.eval_f32(p, mutant="gate_gt"), stmt=s)
    # torch itself, in float64 on the same numbers, takes the >= branch
    x1 = torch.from_numpy(np.stack(p["hs_v1"])).double().requires_grad_(True)
    x2 = torch.from_numpy(np.stack(p["hs_v2"])).double()
    b, q = torch.from_numpy(case["bid"]).long(), torch.from_numpy(case["idx"])
    y1 = torch.nn.functional.normalize(x1[0][b, q], dim=-1, eps=case["eps"])
    y2 = torch.nn.functional.normalize(x2[0][b, q], dim=-1, eps=case["eps"])
    loss = 10 * ((y1 - y2) ** 2 * torch.from_numpy(case["weights"]).double()[:, None]).mean() * float(case["upstream"][0])
    loss.backward()
    got = x1.grad[0][b, q].numpy()
    top = np.abs(got).max(-1, keepdims=True)
    assert np.all(np.abs(s["grad"][0][0] - got) <= 1e-12 * top)


def test_rows_below_the_clamp_are_decided_and_an_open_gate_admits_both_branches():
    case = C.below_eps()
    p = C.problem(case)
    s = R.statement(p)
    assert not s["open"].any()
    assert R.check_consis(p, *R.eval_f32(p), stmt=s)["no_statement"] == 0
    # a norm within its own rounding of eps: the gate is open, either branch is admissible
    case = C.exact_tie()
    case["eps"] = 1e-12
    row = np.zeros(256, np.float32)
    row[:4] = np.float32(0.5e-12)                        # norm = 1e-12 up to rounding, fp32(1e-12) != 1e-12
    case["buf_v1"][0][1, 0, :] = row
    p = C.problem(case)
    s = R.statement(p)
    assert s["open"].sum() == 1
    for mutant in (None, "gate_gt"):
        R.check_consis(p, *R.eval_f32(p, mutant=mutant), stmt=s)


def test_out_of_range_pair_makes_the_losses_nan():
    case = C.out_of_range()
    p = C.problem(case)
    losses, grads, g2 = R.eval_f32(p)
    assert np.isnan(losses).all()
    R.check_consis(p, losses, grads, g2)
    with pytest.raises(R.Inadmissible):
        R.check_consis(p, np.zeros_like(losses), grads, g2)


def test_reduction_depth():
    assert R.consis_depth(256) == 9 and R.consis_depth(36) == 9 and R.consis_depth(1024) == 12
    for case in (C.d36(), C.d1024(), C.k1500()):
        p = C.problem(case)
        assert R.check_consis(p, *R.eval_f32(p))["no_statement"] == 0


class _Layer(ctypes.Structure):
    _fields_ = [("v1", ctypes.c_void_p), ("v2", ctypes.c_void_p), ("v1_stride", ctypes.c_int64 * 2),
                ("v2_stride", ctypes.c_int64 * 2), ("grad_v1", ctypes.c_void_p)]


def test_c_abi_rejects_bad_arguments_without_a_gpu():
    import semi_detr_amd
    from semi_detr_amd import consis_loss as M
    assert {"semidetr_consis_loss_workspace_bytes", "semidetr_consis_loss_forward_f32",
            "semidetr_consis_loss_backward_f32"} <= set(semi_detr_amd._lib.SIGNATURES)
    assert ctypes.sizeof(M._Layer) == ctypes.sizeof(_Layer) == 56
    lib = semi_detr_amd._lib.lib()
    fwd, bwd = lib.semidetr_consis_loss_forward_f32, lib.semidetr_consis_loss_backward_f32

    def params(L=2, B=2, Q=8, D=256, pad=5, K=4):
        p = M._Params()
        p.num_layers, p.batch, p.num_query, p.dim, p.pad_size, p.num_known = L, B, Q, D, pad, K
        p.scale, p.eps = 10.0, 1e-12
        p.known_bid = p.map_known_indice = 64                  # never dereferenced on the host
        for l in range(min(L, M.MAX_LAYERS)):
            p.layer[l].v1 = p.layer[l].v2 = 64
            p.layer[l].v1_stride[0], p.layer[l].v1_stride[1] = Q * D, D
            p.layer[l].v2_stride[0], p.layer[l].v2_stride[1] = Q * D, D
        return p

    def rejected(rc, text):
        assert rc == -1 and text in lib.semidetr_last_error(), (rc, lib.semidetr_last_error())

    rejected(fwd(None, None, 64, 1 << 20, 64), b"null pointer")
    rejected(bwd(None, None, 64, 1 << 20, 64), b"null pointer")
    rejected(fwd(None, ctypes.byref(params(D=38)), 64, 1 << 20, 64), b"not a multiple of 4")
    rejected(fwd(None, ctypes.byref(params(L=17)), 64, 1 << 20, 64), b"17 layers")
    rejected(fwd(None, ctypes.byref(params(pad=9)), 64, 1 << 20, 64), b"pad_size 9")
    rejected(fwd(None, ctypes.byref(params()), None, 1 << 20, 64), b"workspace")
    rejected(fwd(None, ctypes.byref(params()), 64, 8, 64), b"workspace")
    rejected(fwd(None, ctypes.byref(params()), 64, 1 << 20, None), b"null pointer")
    p = params()
    p.known_bid = None
    rejected(fwd(None, ctypes.byref(p), 64, 1 << 20, 64), b"null pointer")
    p = params()
    p.layer[1].v2 = None
    rejected(fwd(None, ctypes.byref(p), 64, 1 << 20, 64), b"layer 1: null pointer")
    p = params()
    p.layer[0].v1_stride[1] = 258                              # rows would not start 16-byte aligned
    rejected(fwd(None, ctypes.byref(p), 64, 1 << 20, 64), b"16-byte aligned")
    rejected(bwd(None, ctypes.byref(params()), 64, 1 << 20, 64), b"grad_v1")        # backward without gradient buffers
    p = params()
    for l in range(2):
        p.layer[l].grad_v1 = 64
    rejected(bwd(None, ctypes.byref(p), 64, 1 << 20, None), b"null pointer")
    need = lib.semidetr_consis_loss_workspace_bytes(6, 1500, 4, 300)
    assert need == 6 * 375 * 8 + 4 * 300 * 4
    assert lib.semidetr_consis_loss_workspace_bytes(17, 10, 2, 5) == 0
    assert lib.semidetr_abi_version() == 7


def test_mirror_has_no_cpu_fallback_and_checks_shapes():
    import semi_detr_amd as s
    assert s.consistency_loss is s.consis_loss.consistency_loss
    assert issubclass(s.ConsistencyLossFunction, torch.autograd.Function)
    hs = [torch.zeros(2, 8, 256) for _ in range(3)]
    meta = {"pad_size_1": 5, "known_bid_1": torch.zeros(4), "map_known_indice_1": torch.zeros(4, dtype=torch.int64),
            "loss_weights": torch.ones(4, 1)}
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        s.consistency_loss(hs, hs, meta)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        s.consistency_loss(torch.stack(hs), torch.stack(hs), meta, warm_up=False)


def test_kernels_use_no_scratch_and_no_float_atomics():
    from test_cabi_host import _code_object_kernels
    meta = _code_object_kernels(os.path.join(ROOT, "semi-detr_amd", "csrc", "libsemidetr_hip.so"))
    mine = {n: k for n, k in meta.items() if n.startswith("consis_")}
    assert len(mine) == 5, sorted(mine)                   # forward and backward for D = 256 and generic, the finalize
    for n, k in mine.items():
        assert not k[".vgpr_spill_count"] and not k[".sgpr_spill_count"] and not k[".private_segment_fixed_size"], n
    src = open(os.path.join(ROOT, "semi-detr_amd", "csrc", "consis_loss.hip")).read()
    assert "atomic" not in src.split("#include", 1)[1]
