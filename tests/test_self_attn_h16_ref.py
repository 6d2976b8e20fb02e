"""CPU: the yardstick of the self-attention's ``operand`` arithmetic (tests/self_attn_h16_ref64.py) and the host side of the
feature.  The contract's operation order in numpy fp32 (``emulate``) is inside the derived bounds on every case of
tests/self_attn_cases.py in both 16-bit types with nothing excluded; mutations of it leave them; the library exports the two
entry points and refuses bad blocks before any launch; the Python interface carries ``arithmetic``."""
import copy
import ctypes
import pickle

import numpy as np
import pytest
import torch
from torch import nn

import self_attn_cases as C
import self_attn_h16_ref64 as R16
from msda_h16_ref import MAX16

NEW = ("semidetr_self_attn_forward_h16", "semidetr_self_attn_backward_h16")


@pytest.mark.parametrize("dtype16", R16.DTYPES)
def test_the_contract_in_numpy_is_within_the_bounds_on_every_case(dtype16):
    worst = {}
    for name in C.names():
        ref = R16.reference(name, dtype16)
        rep = R16.check(R16.emulate(C.cases()[name], dtype16), ref, f"{name} {dtype16}")
        for k, v in rep.items():
            worst[k] = max(worst.get(k, 0.0), v)
        # the bounds say nothing once a value can leave the type's range: no case gets near it
        assert all(np.nanmax(np.abs(ref[n]) + ref["b_" + n]) < 0.5 * MAX16[dtype16] for n in ("out", "dq", "dk", "dv") if n in ref)
    print(R16.table(f"emulate {dtype16}: worst error / bound", worst))
    assert set(worst) == {"out", "lse", "dq", "dk", "dv"}


def _leaves(name, dtype16, **mutation):
    try:
        R16.check(R16.emulate(C.cases()[name], dtype16, **mutation), R16.reference(name, dtype16), name)
    except AssertionError as e:
        assert "outside the bound" in str(e)
        return True
    return False


# mutation -> the cases it is tried on (it must leave the bounds on at least one of them, in each dtype)
MUTATIONS = {
    "scale omitted": (dict(no_scale=True), ("L33_B1",)),
    "mask shifted by one row": (dict(mask="shifted"), ("dn_edges_in_tiles",)),
    "last key tile dropped": (dict(drop_last_tile=True), ("L65_B1",)),
    "no rescale after a new maximum": (dict(no_rescale=True), ("L129_B1",)),
    "dk and dv swapped": (dict(swap_dk_dv=True), ("lq_ne_lk_wide",)),
    "scores rounded to 16 bits before the softmax": (dict(round_scores=True), ("large_scores", "L257_B3_masked", "L129_B1")),
    "P rounded before the row sum, the sum over the rounded values": (dict(sum_rounded_p=True),
                                                                       ("L257_B3_masked", "L129_B1", "dn_skipped_tiles")),
}


@pytest.mark.parametrize("dtype16", R16.DTYPES)
@pytest.mark.parametrize("what", list(MUTATIONS))
def test_the_bounds_catch_the_mutations(what, dtype16):
    mutation, names = MUTATIONS[what]
    caught = []
    for name in names:
        m = dict(mutation)
        if m.get("mask") == "shifted":
            m["mask"] = np.roll(C.cases()[name]["mask"], 1, axis=0)
        caught.append(_leaves(name, dtype16, **m))
    assert any(caught), f"{what} ({dtype16}) stays inside the bounds on {names}"


def test_new_symbols_are_declared_exported_and_in_the_signature_table():
    import semi_detr_amd
    lib = semi_detr_amd._lib.lib()
    for n in NEW:
        assert n in semi_detr_amd._lib.SIGNATURES and hasattr(lib, n)
    assert semi_detr_amd._lib.STRUCTS["semidetr_self_attn_h16"] is semi_detr_amd._lib.SelfAttnH16
    assert lib.semidetr_abi_version() == 7


def _block(dev_ptr=0x1000, fp32=False):
    """A parameter block that passes every host check but points nowhere (it is never launched: a refusal comes first)."""
    from semi_detr_amd import _lib
    p = _lib.SelfAttn() if fp32 else _lib.SelfAttnH16()
    p.batch, p.heads, p.head_dim, p.len_q, p.len_k, p.scale = 1, 8, 32, 8, 8, 0.125
    if not fp32:
        p.type = _lib.ROW_TYPES["SEMIDETR_ROW_BF16"]
    for n in ("q", "k", "v", "out", "lse", "grad_out", "grad_q", "grad_k", "grad_v"):
        setattr(p, n, dev_ptr)
    for n in ("q_stride", "k_stride", "v_stride", "gq_stride", "gk_stride", "gv_stride"):
        getattr(p, n)[0], getattr(p, n)[1] = 256, 256
    return p


def test_host_side_refusals_of_the_library_need_no_gpu():
    import semi_detr_amd
    lib = semi_detr_amd._lib.lib()
    fwd, bwd = lib.semidetr_self_attn_forward_h16, lib.semidetr_self_attn_backward_h16

    def refused(fn, p, text):
        assert fn(None, ctypes.byref(p), None, 0) == -1, text
        assert text.encode() in lib.semidetr_last_error(), (text, lib.semidetr_last_error())
    assert fwd(None, None, None, 0) == -1 and b"null pointer" in lib.semidetr_last_error()
    # a block that is refused for its missing workspace only: every other check lets it through
    refused(fwd, _block(), "workspace")
    refused(bwd, _block(), "workspace")
    for code in (0, 3, -1):                                   # SEMIDETR_ROW_F32 and unknown codes
        p = _block()
        p.type = code
        refused(fwd, p, f"element type {code}")
        refused(bwd, p, f"element type {code}")
    p = _block()
    p.head_dim, p.heads = 64, 4
    refused(fwd, p, "head dimension 64")
    p = _block(0x1004)                                        # rows 4 bytes into an 8-byte line
    refused(fwd, p, "8-byte aligned")
    p = _block()
    p.k_stride[0] = 258                                       # a leading stride that is no multiple of 4 elements
    refused(fwd, p, "8-byte aligned")
    p = _block()
    p.grad_k = 0x1002
    refused(bwd, p, "gradient rows must be 8-byte aligned")
    for n in ("q", "k", "v", "out", "lse"):
        p = _block()
        setattr(p, n, None)
        refused(fwd, p, "null pointer")
        refused(bwd, p, "null pointer")
    p = _block()
    p.grad_out = None
    refused(bwd, p, "grad_out")
    p = _block()
    p.grad_q = p.grad_k = p.grad_v = None
    refused(bwd, p, "no gradient asked for")


def test_host_side_refusals_of_the_fp32_pair_need_no_gpu():
    """The fp32 entry points go through the same host check on their widened block, with their own messages."""
    import semi_detr_amd
    lib = semi_detr_amd._lib.lib()
    fwd, bwd = lib.semidetr_self_attn_forward_f32, lib.semidetr_self_attn_backward_f32

    def refused(fn, p, text):
        assert fn(None, ctypes.byref(p), None, 0) == -1, text
        assert text.encode() in lib.semidetr_last_error(), (text, lib.semidetr_last_error())
        assert b"self_attn_h16" not in lib.semidetr_last_error()
    assert fwd(None, None, None, 0) == -1 and b"self_attn: null pointer (parameter block)" in lib.semidetr_last_error()
    # a block that is refused for its missing workspace only: every other check lets it through
    refused(fwd, _block(fp32=True), "self_attn: workspace null, misaligned or smaller than semidetr_self_attn_workspace_bytes()")
    refused(bwd, _block(fp32=True), "self_attn: workspace null, misaligned or smaller than semidetr_self_attn_workspace_bytes()")
    p = _block(fp32=True)
    p.head_dim, p.heads = 64, 4
    refused(fwd, p, "self_attn: head dimension 64 (only 32 is built)")
    refused(bwd, p, "self_attn: head dimension 64 (only 32 is built)")
    p = _block(0x1008, fp32=True)                             # rows 8 bytes into a 16-byte line: the 16-bit pair takes them
    refused(fwd, p, "self_attn: rows must be 16-byte aligned (base and strides) with non-negative strides")
    p = _block(fp32=True)
    p.k_stride[0] = 258                                       # a leading stride that is no multiple of 4 elements
    refused(fwd, p, "self_attn: rows must be 16-byte aligned (base and strides) with non-negative strides")
    p = _block(fp32=True)
    p.grad_k = 0x1008
    refused(bwd, p, "self_attn backward: gradient rows must be 16-byte aligned (base and strides)")
    for n in ("q", "k", "v", "out", "lse"):
        p = _block(fp32=True)
        setattr(p, n, None)
        refused(fwd, p, "self_attn: null pointer (q / k / v / out / lse)")
        refused(bwd, p, "self_attn: null pointer (q / k / v / out / lse)")
    p = _block(fp32=True)
    p.grad_out = None
    refused(bwd, p, "self_attn backward: null or misaligned grad_out")
    p = _block(fp32=True)
    p.grad_q = p.grad_k = p.grad_v = None
    refused(bwd, p, "self_attn backward: no gradient asked for")


def test_arithmetic_is_checked_before_any_device_work():
    import semi_detr_amd as s
    x = torch.zeros(5, 1, 256, dtype=torch.float16)          # CPU tensors: anything that reached the device path would raise
    with pytest.raises(ValueError, match="arithmetic"):      # RuntimeError("no CPU fallback") instead
        s.masked_attention(x, x, x, 8, arithmetic="nonsense")
    with pytest.raises(ValueError, match="one dtype"):
        s.masked_attention(x, x.float(), x, 8, arithmetic="operand")
    with pytest.raises(ValueError, match="one dtype"):
        s.masked_attention(x, x, x.bfloat16(), 8, arithmetic="operand")
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        s.masked_attention(x, x, x, 8, arithmetic="operand")
    with pytest.raises(ValueError, match="arithmetic"):
        s.MultiheadAttention(256, 8, arithmetic="fp64")
    with pytest.raises(ValueError, match="arithmetic"):
        s.convert_self_attention(nn.Module(), arithmetic="half")


def test_arithmetic_survives_adopt_deepcopy_and_pickling_and_adds_no_state():
    import semi_detr_amd as s
    ref = nn.MultiheadAttention(256, 8)
    assert s.MultiheadAttention(256, 8).arithmetic == "fp32" and s.MultiheadAttention.adopt(ref).arithmetic == "fp32"
    m = s.MultiheadAttention.adopt(ref, arithmetic="operand")
    assert m.arithmetic == "operand" and m.in_proj_weight is ref.in_proj_weight
    assert copy.deepcopy(m).arithmetic == "operand"
    again = pickle.loads(pickle.dumps(m))
    assert again.arithmetic == "operand" and torch.equal(again.in_proj_weight, m.in_proj_weight)
    old = pickle.loads(pickle.dumps(s.MultiheadAttention(64, 2)))
    del old.__dict__["arithmetic"]                           # an instance pickled before the attribute existed
    assert pickle.loads(pickle.dumps(old)).arithmetic == "fp32"
    assert list(m.state_dict()) == list(ref.state_dict())
    assert [n for n, _ in m.named_buffers()] == [] and [n for n, _ in m.named_parameters()] == [n for n, _ in ref.named_parameters()]
    tree = nn.Module()
    tree.a, tree.b = nn.MultiheadAttention(256, 8), nn.MultiheadAttention(64, 2)
    keys = list(tree.state_dict())
    assert s.convert_self_attention(tree, arithmetic="operand") == 2
    assert tree.a.arithmetic == tree.b.arithmetic == "operand" and list(tree.state_dict()) == keys
    tree.load_state_dict(nn.ModuleDict(dict(a=nn.MultiheadAttention(256, 8), b=nn.MultiheadAttention(64, 2))).state_dict(), strict=True)
