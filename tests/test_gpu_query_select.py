"""The two-stage query selection on the MI355X (csrc/query_select.hip) against the reference's fixtures
(tests/golden/query_select.npz) and the float64 statement with its fp32 bounds (tests/query_select_ref64.py), through the
public Python functions and through the C ABI."""
import ctypes
import types

import numpy as np
import pytest
import torch

import query_select_ref64 as R
from test_query_select_ref import CASES, SELECT, diff, shapes_of

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
FULL4 = [(100, 167), (50, 84), (25, 42), (13, 21)]                 # S = 22 223
FULL5 = [(100, 167), (50, 84), (25, 42), (13, 21), (7, 11)]        # the COCO-Full five-level pyramid


def _np(t):
    return t.detach().cpu().numpy()


def _dev(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a))
    return (t if dtype is None else t.to(dtype)).to(DEV)


def _report(what, err, bound):
    worst = float((err[bound > 0] / bound[bound > 0]).max(initial=0.0))
    print(f"[query_select] {what}: worst err / bound = {worst:.3f}")
    assert (err <= bound).all(), (what, worst)


def check_proposals(name, mask, shapes, memory, shapes_arg):
    """gen_encoder_output_proposals forward + backward against the statement.  Returns the device outputs."""
    import semi_detr_amd as s
    p = R.proposals(mask, shapes)
    mem = _dev(memory).requires_grad_(True)
    om, prop = s.gen_encoder_output_proposals(mem, _dev(mask), shapes_arg)
    assert om.dtype == prop.dtype == torch.float32 and not prop.requires_grad
    got = _np(prop).astype(np.float64)
    assert np.array_equal(np.isinf(got) & (got > 0), np.isinf(p["prop"]))                   # the flags, exactly
    fin = np.isfinite(p["prop"])
    _report(f"{name} logits", np.abs(got[fin] - p["prop"][fin]), p["bound"][fin])
    assert _np(om).tobytes() == R.masked_memory(memory, p["valid"]).tobytes()
    g = R.grad_pattern(memory.shape, 3)
    grads = []
    for _ in range(2):
        mem.grad = None
        om2, _ = s.gen_encoder_output_proposals(mem, _dev(mask), shapes_arg)
        om2.backward(_dev(g))
        grads.append(_np(mem.grad).copy())
    assert grads[0].tobytes() == grads[1].tobytes() == R.masked_memory(g, p["valid"]).tobytes()
    return p, om.detach(), prop.detach()


def check_select(name, logits, reg, p, om, prop, k):
    """select_queries forward + backward against the statement (fp64 from the same fp32 inputs)."""
    import semi_detr_amd as s
    N, S = logits.shape[:2]
    coord = (_dev(reg) + prop).requires_grad_(True)
    outmem = om.clone().requires_grad_(True)
    lg = _dev(logits)
    idx, ref, init, tgt, ref_enc = s.select_queries(lg, coord, prop, outmem, k)
    assert idx.dtype == torch.int64 and idx.shape == (N, k)
    keys = R.keys_of(logits)
    want = R.topk(keys, k)
    assert np.array_equal(_np(idx), want)                                                  # the total order, exactly
    coord_np, om_np = _np(coord), _np(om)
    g = R.gather(want, coord_np, _np(prop).astype(np.float64), p["bound"] * 0, om_np)      # from the device's fp32 inputs
    assert _np(ref).tobytes() == coord_np[np.arange(N)[:, None], want].tobytes()
    assert _np(tgt).tobytes() == om_np[np.arange(N)[:, None], want].tobytes()
    _report(f"{name} ref_enc", diff(_np(ref_enc), g["ref_enc"]), g["ref_bound"])
    _report(f"{name} init_box", diff(_np(init), g["init_box"]), g["init_bound"])
    gs = R.gather(want, coord_np, p["prop"], p["bound"], om_np)                            # and against the exact anchors
    _report(f"{name} init_box vs fp64 anchors", diff(_np(init), gs["init_box"]), gs["init_bound"])
    g1, g2, g3 = R.grad_pattern(tgt.shape, 1), R.grad_pattern(ref_enc.shape, 2), R.grad_pattern(ref.shape, 5)
    runs = []
    for _ in range(2):
        coord.grad = outmem.grad = None
        _, ref2, _, tgt2, enc2 = s.select_queries(lg, coord, prop, outmem, k)
        ((tgt2 * _dev(g1)).sum() + (enc2 * _dev(g2)).sum() + (ref2 * _dev(g3)).sum()).backward()
        runs.append((_np(coord.grad).copy(), _np(outmem.grad).copy()))
    assert runs[0][0].tobytes() == runs[1][0].tobytes() and runs[0][1].tobytes() == runs[1][1].tobytes()
    gc, bound, gm = R.gather_backward(want, S, g["ref_enc"], g3, g1, g2)
    assert runs[0][1].tobytes() == gm.tobytes()                                            # copies and zeros
    _report(f"{name} grad coord", diff(runs[0][0], gc), bound)
    return want


@pytest.mark.parametrize("name", SELECT)
def test_fixture_cases(name):
    c = CASES[name]
    mask, shapes = c["mask"].astype(bool), shapes_of(c)
    for shapes_arg in (_dev(c["shapes"]), shapes):                     # the reference's device tensor, and a host list
        p, om, prop = check_proposals(name, mask, shapes, c["memory"], shapes_arg)
    ref_valid = ~np.isinf(c["prop32"]).all(-1)
    assert np.array_equal(p["valid"], ref_valid)
    k = int(c["k"])
    idx = check_select(name, c["logits"].astype(np.float32), c["reg"].astype(np.float32), p, om, prop, k)
    uniq = R.unique_key_slots(R.keys_of(c["logits"]), idx)
    assert np.array_equal(idx[uniq], c["topi32"][uniq])                 # the reference's choice wherever the keys decide


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


FRACS = [(1.0, 1.0), (0.75, 0.9), (1.0, 0.62), (0.55, 1.0)]


@pytest.mark.parametrize("shapes,B", [(FULL4, 1), (FULL4, 4), (FULL5, 1), (FULL5, 4)])
def test_full_size_seeded(shapes, B):
    rng = np.random.default_rng(100 + B + len(shapes))
    mask = band_mask(shapes, FRACS[:B] if B > 1 else FRACS[1:2])
    S = mask.shape[1]
    memory = rng.standard_normal((B, S, 256)).astype(np.float32)
    name = f"full L{len(shapes)} B{B}"
    p, om, prop = check_proposals(name, mask, shapes, memory, _dev(np.asarray(shapes, np.int64)))
    logits = rng.standard_normal((B, S, 80)).astype(np.float32)
    logits[~p["valid"]] = np.linspace(-2, 1.5, 80, dtype=np.float32)  # what a zeroed row gives: the head's bias
    reg = (rng.standard_normal((B, S, 4)) * 0.5).astype(np.float32)
    check_select(name, logits, reg, p, om, prop, 900)


@pytest.mark.parametrize("D", [6, 1, 10])
def test_channel_counts_that_are_no_multiple_of_four(D):
    """The element-wise paths of the four copying kernels (the 16-byte paths need D % 4 == 0)."""
    rng = np.random.default_rng(40 + D)
    shapes = [(7, 9), (4, 5), (2, 3)]
    mask = band_mask(shapes, [(1.0, 1.0), (0.6, 0.8), (0.9, 0.5)])
    B, S = mask.shape
    memory = rng.standard_normal((B, S, D)).astype(np.float32)
    p, om, prop = check_proposals(f"D={D}", mask, shapes, memory, shapes)
    logits = rng.standard_normal((B, S, 20)).astype(np.float32)
    reg = (rng.standard_normal((B, S, 4)) * 0.5).astype(np.float32)
    check_select(f"D={D}", logits, reg, p, om, prop, 25)


def test_cabi_inverse_map_and_large_s_path():
    """Straight through the C ABI: the inverse map (every element written), k == 1, and an S whose keys do not fit LDS
    (the workspace path of the select kernel)."""
    import semi_detr_amd
    lib = semi_detr_amd._lib.lib()
    rng = np.random.default_rng(5)
    P = ctypes.c_void_p
    for N, S, C, k in ((2, 300, 20, 1), (2, 300, 7, 300), (2, 50000, 4, 900), (1, 22223, 80, 4096)):
        logits = rng.integers(-50, 50, (N, S, C)).astype(np.float32) / 4        # many exact ties
        lg = _dev(logits)
        nbytes = lib.semidetr_qsel_topk_workspace_bytes(N, S)
        ws = torch.empty(nbytes, dtype=torch.uint8, device=DEV)
        idx = torch.full((N, k), -7, dtype=torch.int64, device=DEV)
        inv = torch.full((N, S), -7, dtype=torch.int32, device=DEV)
        rc = lib.semidetr_qsel_topk_f32(P(torch.cuda.current_stream().cuda_stream), P(lg.data_ptr()), N, S, C, k,
                                        P(ws.data_ptr()), nbytes, P(idx.data_ptr()), P(inv.data_ptr()))
        assert rc == 0, lib.semidetr_last_error()
        want = R.topk(R.keys_of(logits), k)
        assert np.array_equal(_np(idx), want) and np.array_equal(_np(inv), R.inverse_map(want, S))


def test_graph_capture_and_replay():
    import semi_detr_amd as s
    c = CASES["four_levels"]
    mask, shapes, k = _dev(c["mask"].astype(bool)), _dev(c["shapes"]), int(c["k"])
    mem, lg, reg = _dev(c["memory"]), _dev(c["logits"].astype(np.float32)), _dev(c["reg"].astype(np.float32))

    def step():
        om, prop = s.gen_encoder_output_proposals(mem, mask, shapes)
        return (om, prop) + tuple(s.select_queries(lg, reg + prop, prop, om, k))
    eager = [_np(t).copy() for t in step()]
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        step()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        outs = step()
    for _ in range(2):
        for t in outs:
            t.zero_() if t.dtype != torch.int64 else t.fill_(-1)
        graph.replay()
        torch.cuda.synchronize()
        for a, b in zip(eager, outs):
            assert a.tobytes() == _np(b).tobytes()


def test_graph_capture_and_replay_of_the_backwards():
    import semi_detr_amd as s
    c = CASES["four_levels"]
    mask, shapes, k = _dev(c["mask"].astype(bool)), _dev(c["shapes"]), int(c["k"])
    mem = _dev(c["memory"]).requires_grad_(True)
    lg, reg = _dev(c["logits"].astype(np.float32)), _dev(c["reg"].astype(np.float32))
    D = mem.shape[2]
    g1, g2 = _dev(R.grad_pattern((mem.shape[0], k, D), 1)), _dev(R.grad_pattern((mem.shape[0], k, 4), 2))

    def step():
        om, prop = s.gen_encoder_output_proposals(mem, mask, shapes)
        coord = (reg + prop).requires_grad_(True)
        _, _, _, tgt, enc = s.select_queries(lg, coord, prop, om, k)
        return torch.autograd.grad([tgt, enc], [mem, coord], [g1, g2])
    eager = [_np(t).copy() for t in step()]
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        step()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        outs = step()
    for _ in range(2):
        for t in outs:
            t.fill_(7.0)
        graph.replay()
        torch.cuda.synchronize()
        for a, b in zip(eager, outs):
            assert a.tobytes() == _np(b).tobytes()


def forward_key_gap(c):
    """Smallest gap between neighbours among the k + 1 largest float64 keys of the ``forward`` case."""
    p = R.proposals(c["mask"].astype(bool), shapes_of(c))
    x = R.masked_memory(c["memory"], p["valid"]).astype(np.float64) @ c["w_out"].T.astype(np.float64) + c["b_out"]
    x = (x - x.mean(-1, keepdims=True)) / np.sqrt(x.var(-1, keepdims=True) + 1e-5) * c["ln_w"] + c["ln_b"]
    keys = (x @ c["w_cls"].T.astype(np.float64) + c["b_cls"]).max(-1)
    top = -np.sort(-keys, 1)[:, :int(c["k"]) + 1]
    return float(np.abs(np.diff(top, axis=1)).min())


def test_two_stage_queries_binding_hands_the_decoder_the_reference_tensors():
    """The helper on a stand-in transformer with the fixture's seeded enc_output / LayerNorm / heads against what the
    reference's forward handed its decoder and returned.  The GEMMs run in fp32 on the GPU and in float64 in the fixture, so
    the check first establishes from the float64 keys that no decision is within reach of that difference."""
    from semi_detr_amd import query_select as Q
    from torch import nn
    c = CASES["forward"]
    D, k = c["memory"].shape[2], int(c["k"])

    def lin(w, b):
        m = nn.Linear(w.shape[1], w.shape[0]).to(DEV)
        m.weight.data, m.bias.data = _dev(w), _dev(b)
        return m
    norm = nn.LayerNorm(D).to(DEV)
    norm.weight.data, norm.bias.data = _dev(c["ln_w"]), _dev(c["ln_b"])
    emb = nn.Embedding(k, D).to(DEV)
    emb.weight.data = _dev(c["tgt_embed"])
    self = types.SimpleNamespace(two_stage_type="standard", enc_output=lin(c["w_out"], c["b_out"]), enc_output_norm=norm,
                                 num_queries=k, embed_init_tgt=True, tgt_embed=emb, d_model=D)
    self.two_stage_queries = types.MethodType(Q.two_stage_queries, self)
    mem = _dev(c["memory"]).requires_grad_(True)
    ref, tgt, hs_enc, ref_enc, init = self.two_stage_queries(mem, _dev(c["mask"].astype(bool)), _dev(c["shapes"]),
                                                             lin(c["w_cls"], c["b_cls"]), lin(c["w_reg"], c["b_reg"]),
                                                             _dev(c["dn_ref"]), _dev(c["dn_tgt"]))
    # the float64 keys of the k + 1 best tokens are apart by far more than the fp32 GEMMs' error: no decision is open
    assert forward_key_gap(c) > 1e-3 and np.array_equal(c["topi32"], c["topi64"])
    assert np.array_equal(_np(tgt), c["dec_tgt32"]) and tgt.shape == c["dec_tgt64"].shape
    # two 16-term fp32 dot products (gamma_16 = 16 u of sum |x||w| < 64) and a LayerNorm on O(1) numbers stay below 1e-4;
    # a wrong row would differ by O(1)
    tol = 1e-4
    assert np.array_equal(_np(ref[:, :-k]), c["dn_ref"]) and not ref.requires_grad
    assert diff(_np(ref[:, -k:]), c["dec_ref64"][:, -k:]).max() <= tol * 8
    assert diff(_np(hs_enc[0]), c["hs_enc64"]).max() <= tol and hs_enc.shape == (1,) + c["hs_enc64"].shape
    assert diff(_np(ref_enc[0]), c["ref_enc64"]).max() <= tol and diff(_np(init), c["init64"]).max() <= tol
    assert hs_enc.requires_grad and ref_enc.requires_grad and not init.requires_grad
    (hs_enc.sum() + ref_enc.sum()).backward()
    assert mem.grad is not None and np.isfinite(_np(mem.grad)).all()
    valid = ~np.isinf(c["prop32"]).all(-1)
    assert not _np(mem.grad)[~valid].any()


def test_errors():
    import semi_detr_amd as s
    z = torch.zeros(1, 12, 4, device=DEV)
    with pytest.raises(RuntimeError, match="selected index k out of range"):
        s.select_queries(z, z, z, z, 13)
    with pytest.raises(RuntimeError, match="hold 11 tokens"):
        s.gen_encoder_output_proposals(z, torch.zeros(1, 12, dtype=torch.bool, device=DEV), [(11, 1)])
