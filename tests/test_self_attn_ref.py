"""CPU: the float64 statement of the decoder self-attention (tests/self_attn_ref64.py) against the fixture recorded from the
reference's ``forward_sa`` (tests/golden/self_attn.npz, tools/gen_self_attn_golden.py); torch's own fp32 op inside the derived
bounds on every case of tests/self_attn_cases.py; the mutations the bounds must catch; and the host side of the feature: the
C ABI's new symbols, the module's constructor contract, ``convert_self_attention`` and ``bind_decoder_self_attention``."""
import ctypes
import sys
import types

import numpy as np
import pytest
import torch
from torch import nn

import self_attn_cases as C
import self_attn_ref64 as R


# ---------------------------------------------------------------------------------------------------------------------------
# the statement against the reference
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def golden():
    from conftest import Golden
    return Golden("self_attn.npz")


@pytest.mark.parametrize("name", ["plain", "dn_mask", "two_images"])
def test_ref64_is_what_the_reference_computes(golden, name):
    c = golden[name]
    f = lambda n: c[n].astype(np.float64)      # noqa: E731
    E = c["tgt"].shape[2]
    W, b, Wo, bo = f("in_proj_weight"), f("in_proj_bias"), f("out_w"), f("out_b")
    x = f("tgt") + f("pos")
    q, k, v = x @ W[:E].T + b[:E], x @ W[E:2 * E].T + b[E:2 * E], f("tgt") @ W[2 * E:].T + b[2 * E:]
    gout = c["g_tgt2"] @ Wo
    mask = c["mask"].astype(bool) if "mask" in c else None
    r = R.ref64(dict(q=q, k=k, v=v, heads=int(c["heads"]), mask=mask, scale=None, gout=gout))
    tgt2 = r["out"] @ Wo.T + bo
    assert np.abs(tgt2 - c["tgt2"]).max() < 1e-12
    mu = (f("tgt") + tgt2).mean(-1, keepdims=True)
    var = (f("tgt") + tgt2).var(-1, keepdims=True)
    assert np.abs((f("tgt") + tgt2 - mu) / np.sqrt(var + 1e-5) * f("ln_w") + f("ln_b") - c["out"]).max() < 1e-12
    g_pos = r["dq"] @ W[:E] + r["dk"] @ W[E:2 * E]
    assert np.abs(g_pos - c["g_pos"]).max() < 1e-12
    assert np.abs(g_pos + r["dv"] @ W[2 * E:] + c["g_tgt2"] - c["g_tgt"]).max() < 1e-12      # + the residual branch
    g_bias = np.concatenate([r[n].sum((0, 1)) for n in ("dq", "dk", "dv")])
    assert np.abs(g_bias - c["g_in_proj_bias"]).max() < 1e-11


def test_fully_blocked_row_is_nan_in_that_row_only():
    p = C.cases()["blocked_row"]
    out = C.reference("blocked_row")["out"]
    assert np.isnan(out[40]).all() and not np.isnan(np.delete(out, 40, axis=0)).any()
    q, k, v = (torch.from_numpy(p[n]).double() for n in "qkv")
    mha = nn.MultiheadAttention(256, 8).double()
    with torch.no_grad():
        mha.in_proj_weight.copy_(torch.eye(256).repeat(3, 1))
        mha.in_proj_bias.zero_()
        mha.out_proj.weight.copy_(torch.eye(256))
        mha.out_proj.bias.zero_()
        want = mha(q, k, v, attn_mask=torch.from_numpy(p["mask"]))[0].numpy()
    assert np.isnan(want[40]).all()
    assert np.nanmax(np.abs(want - out)) < 1e-13


# ---------------------------------------------------------------------------------------------------------------------------
# fp32 implementations on the CPU against the bounds
# ---------------------------------------------------------------------------------------------------------------------------
def torch_fp32(p, scale=None, mask="own", swap_kv_grads=False):
    """The op as torch computes it in fp32 on the CPU (bmm, masked_fill, softmax, bmm), with the mutations of the tests."""
    q, k, v = (torch.from_numpy(p[n]).requires_grad_(True) for n in "qkv")
    (Lq, B, E), Lk, H = q.shape, k.shape[0], p["heads"]
    D = E // H
    if scale is None:
        scale = D ** -0.5 if p["scale"] is None else p["scale"]
    mask = p["mask"] if isinstance(mask, str) else mask
    qh, kh, vh = ((t * f).reshape(-1, B * H, D).transpose(0, 1) for t, f in ((q, scale), (k, 1.0), (v, 1.0)))
    s = torch.bmm(qh, kh.transpose(1, 2))
    if mask is not None:
        s = s.masked_fill(torch.from_numpy(mask), float("-inf"))
    out = torch.bmm(torch.softmax(s, -1), vh).transpose(0, 1).reshape(Lq, B, E)
    got = {"out": out.detach().numpy()}
    if not p["forward_only"]:
        out.backward(torch.from_numpy(p["gout"]))
        got.update(dq=q.grad.numpy(), dk=k.grad.numpy(), dv=v.grad.numpy())
        if swap_kv_grads:
            got["dk"], got["dv"] = got["dv"], got["dk"]
    return got


def online_fp32(p, rescale=True, drop_last_tile=False):
    """The forward as an online softmax over key tiles of 32 in numpy fp32 (the kernel's scheme), with two mutations."""
    f = np.float32
    q, k, v = p["q"], p["k"], p["v"]
    (Lq, B, E), Lk, H = q.shape, k.shape[0], p["heads"]
    D = E // H
    scale = f(D ** -0.5 if p["scale"] is None else p["scale"])
    out = np.zeros((Lq, B, E), f)
    tiles = list(range(0, Lk, R.TILE))
    if drop_last_tile:
        tiles = tiles[:-1]
    for b in range(B):
        for h in range(H):
            sl = slice(h * D, (h + 1) * D)
            qs = q[:, b, sl] * scale
            m, l, O = np.full(Lq, -np.inf, f), np.zeros(Lq, f), np.zeros((Lq, D), f)
            for t in tiles:
                s = qs @ k[t:t + R.TILE, b, sl].T
                if p["mask"] is not None:
                    s = np.where(p["mask"][:, t:t + R.TILE], f(-np.inf), s)
                mn = np.maximum(m, s.max(1))
                safe = np.where(np.isinf(mn), f(0), mn)
                alpha = np.exp(m - safe)
                pt = np.exp(s - safe[:, None])
                l = l * alpha + pt.sum(1)
                O = (O * alpha[:, None] if rescale else O) + pt @ v[t:t + R.TILE, b, sl]
                m = mn
            with np.errstate(invalid="ignore", divide="ignore"):
                out[:, b, sl] = O / l[:, None]
    return {"out": out}


@pytest.mark.parametrize("name", C.names())
def test_torch_fp32_on_the_cpu_is_within_the_bounds(name):
    p = C.cases()[name]
    rep = R.check_self_attn(p, torch_fp32(p), name, C.reference(name))
    print(R.table(name, rep))


@pytest.mark.parametrize("name", ["L129_B1", "dn_skipped_tiles", "random_095", "large_scores", "blocked_row"])
def test_online_softmax_in_fp32_is_within_the_bounds(name):
    R.check_self_attn(C.cases()[name], online_fp32(C.cases()[name]), name, C.reference(name))


def test_one_open_key_gives_that_row_of_v_within_a_few_u():
    p, ref = C.cases()["one_open_key"], C.reference("one_open_key")
    j = np.argmin(p["mask"], axis=1)
    assert np.array_equal(ref["out"], p["v"][j].astype(np.float64))
    assert (ref["b_out"] <= 64 * R.U * (np.abs(ref["out"]) + 1e-30) + 2 * R.TINY).all()


def _caught(name, got):
    with pytest.raises(AssertionError, match="outside the bound"):
        R.check_self_attn(C.cases()[name], got, name, C.reference(name))


def test_the_bounds_catch_the_mutations():
    c = C.cases()
    _caught("L33_B1", torch_fp32(c["L33_B1"], scale=1.0))                                       # scale omitted
    shifted = np.roll(c["dn_edges_in_tiles"]["mask"], 1, axis=0)
    _caught("dn_edges_in_tiles", torch_fp32(c["dn_edges_in_tiles"], mask=shifted))              # mask shifted by one row
    _caught("L65_B1", online_fp32(c["L65_B1"], drop_last_tile=True))                            # the last key tile dropped
    _caught("L129_B1", online_fp32(c["L129_B1"], rescale=False))                                # no rescale after a new maximum
    _caught("lq_ne_lk_wide", torch_fp32(c["lq_ne_lk_wide"], swap_kv_grads=True))                # dK and dV swapped


# ---------------------------------------------------------------------------------------------------------------------------
# the host side
# ---------------------------------------------------------------------------------------------------------------------------
NEW = ("semidetr_self_attn_workspace_bytes", "semidetr_self_attn_forward_f32", "semidetr_self_attn_backward_f32")


def test_new_symbols_are_declared_exported_and_in_the_signature_table():
    import semi_detr_amd
    lib = semi_detr_amd._lib.lib()
    for n in NEW:                                # declared by the header: tests/test_cabi_mirror.py
        assert n in semi_detr_amd._lib.SIGNATURES and hasattr(lib, n)
    assert lib.semidetr_abi_version() == 7
    assert lib.semidetr_self_attn_workspace_bytes(2, 8, 100, 70) == 2 * 8 * 100 * 4 + 4 * 3
    assert lib.semidetr_self_attn_workspace_bytes(0, 8, 100, 70) == 0


def test_host_side_refusals_of_the_library_need_no_gpu():
    import semi_detr_amd
    from semi_detr_amd import self_attn
    lib = semi_detr_amd._lib.lib()
    assert lib.semidetr_self_attn_forward_f32(None, None, None, 0) == -1 and b"null pointer" in lib.semidetr_last_error()
    p = self_attn._Params()
    p.batch, p.heads, p.head_dim, p.len_q, p.len_k, p.scale = 1, 4, 64, 8, 8, 0.125
    assert lib.semidetr_self_attn_forward_f32(None, ctypes.byref(p), None, 0) == -1
    assert b"head dimension 64" in lib.semidetr_last_error()
    p.head_dim = 32
    assert lib.semidetr_self_attn_backward_f32(None, ctypes.byref(p), None, 0) == -1 and b"null pointer" in lib.semidetr_last_error()


def test_constructor_contract_and_refusals():
    import semi_detr_amd as s
    ref = nn.MultiheadAttention(256, 8, dropout=0.0)
    m = s.MultiheadAttention(256, 8, dropout=0.0)
    assert [(k, tuple(v.shape)) for k, v in m.state_dict().items()] == [(k, tuple(v.shape)) for k, v in ref.state_dict().items()]
    m.load_state_dict(ref.state_dict(), strict=True)
    assert float(m.in_proj_bias.detach().abs().max()) == 0.0 and float(m.out_proj.bias.detach().abs().max()) == 0.0
    fresh = s.MultiheadAttention(64, 2)
    limit = (6.0 / (64 + 3 * 64)) ** 0.5                                   # xavier_uniform_ of the (3E, E) weight
    assert float(fresh.in_proj_weight.detach().abs().max()) <= limit and float(fresh.in_proj_weight.detach().std()) > 0.4 * limit
    nobias = s.MultiheadAttention(64, 2, bias=False)
    assert nobias.in_proj_bias is None and nobias.out_proj.bias is None
    for kw in (dict(batch_first=True), dict(add_bias_kv=True), dict(add_zero_attn=True), dict(kdim=32)):
        with pytest.raises(NotImplementedError):
            s.MultiheadAttention(256, 8, **kw)
    with pytest.raises(NotImplementedError, match="head dimension"):
        s.MultiheadAttention(256, 4)
    x = torch.zeros(5, 1, 256)
    with pytest.raises(NotImplementedError, match="key_padding_mask"):
        m(x, x, x, key_padding_mask=torch.zeros(1, 5, dtype=torch.bool))
    with pytest.raises(NotImplementedError, match="dropout"):
        s.MultiheadAttention(256, 8, dropout=0.1)(x, x, x)
    with pytest.raises(NotImplementedError, match="float masks"):
        s.masked_attention(x, x, x, 8, attn_mask=torch.zeros(5, 5))
    with pytest.raises(NotImplementedError, match="per-head"):
        s.masked_attention(x, x, x, 8, attn_mask=torch.zeros(8, 5, 5, dtype=torch.bool))
    with pytest.raises(NotImplementedError, match="head dimension"):
        s.masked_attention(x, x, x, 4)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        s.masked_attention(x, x, x, 8)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        m(x, x, x)
    assert s.MultiheadAttention(256, 8, dropout=0.1).eval().dropout == 0.1       # dropout is refused in training mode only


class _FakeLayer(nn.Module):
    def __init__(self, d_model=256, n_heads=8, dropout=0.0):
        super().__init__()
        self.self_attn = nn.MultiheadAttention(d_model, n_heads, dropout=dropout)
        self.norm2 = nn.LayerNorm(d_model)


def test_convert_self_attention_adopts_the_parameter_objects():
    import semi_detr_amd as s
    tree = nn.Module()
    tree.layers = nn.ModuleList([_FakeLayer(), _FakeLayer(), _FakeLayer(dropout=0.1), _FakeLayer(256, 4)])
    tree.layers[1].eval()
    before = dict(tree.named_parameters())
    keys = list(tree.state_dict())
    opt = torch.optim.AdamW(tree.parameters())
    assert s.convert_self_attention(tree) == 2
    kinds = [type(l.self_attn) for l in tree.layers]
    assert kinds == [s.MultiheadAttention, s.MultiheadAttention, nn.MultiheadAttention, nn.MultiheadAttention]
    after = dict(tree.named_parameters())
    assert list(after) == list(before) and all(after[k] is before[k] for k in before)
    assert list(tree.state_dict()) == keys
    assert all(a is b for a, b in zip(opt.param_groups[0]["params"], tree.parameters()))
    assert tree.layers[0].self_attn.training and not tree.layers[1].self_attn.training
    assert s.convert_self_attention(tree) == 0


def test_bind_decoder_self_attention_on_a_fake_detr_od(monkeypatch):
    import semi_detr_amd as s
    from semi_detr_amd import registry
    for n in [k for k in sys.modules if k == "detr_od" or k.startswith("detr_od.")]:
        monkeypatch.delitem(sys.modules, n)
    monkeypatch.setitem(sys.modules, "detr_od", None)                       # import detr_od -> ImportError
    assert registry.bind_decoder_self_attention() == ([], ["DINOTransformerDecoderLayer.self_attn"])
    fake = types.ModuleType("detr_od.models.utils.transformer")

    class DINOTransformerDecoderLayer(_FakeLayer):
        pass
    fake.DINOTransformerDecoderLayer = DINOTransformerDecoderLayer
    monkeypatch.setitem(sys.modules, "detr_od.models.utils.transformer", fake)
    assert type(DINOTransformerDecoderLayer().self_attn) is nn.MultiheadAttention
    assert registry.bind_decoder_self_attention() == (["DINOTransformerDecoderLayer.self_attn"], [])
    init = DINOTransformerDecoderLayer.__init__
    assert registry.bind_decoder_self_attention()[0] and DINOTransformerDecoderLayer.__init__ is init      # bound once
    layer = DINOTransformerDecoderLayer(256, 8)
    assert type(layer.self_attn) is s.MultiheadAttention
    assert list(layer.state_dict()) == list(_FakeLayer().state_dict())
    assert type(DINOTransformerDecoderLayer(256, 4).self_attn) is nn.MultiheadAttention                    # left as it is
