"""CPU: the host surface of the mixed-type add + LayerNorm entry points (``semidetr_add_norm_forward_mixed`` /
``semidetr_add_norm_backward_mixed``, include/semidetr_hip.h) that needs no GPU: the exported symbols, the type codes against the
header, every argument error of the host-side validation from hand-built blocks on host memory (the technique of
tests/test_add_norm_ref.py::test_argument_errors_need_no_gpu), and the stride / alignment logic of ``_lib.rows_native`` on CPU
tensors.  The block's layout and the signatures are checked by tests/test_cabi_mirror.py."""
import ctypes
import os
import re

import pytest
import torch

SYMBOLS = ("semidetr_add_norm_forward_mixed", "semidetr_add_norm_backward_mixed")
HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "semidetr_hip.h")


def test_library_exports_the_two_symbols_and_the_type_codes_are_the_headers():
    import semi_detr_amd
    L = semi_detr_amd._lib
    lib = L.lib()
    for n in SYMBOLS:
        assert hasattr(lib, n) and n in L.SIGNATURES
        assert L.SIGNATURES[n] == (ctypes.c_int, [ctypes.c_void_p, ctypes.POINTER(L.AddNormMixed), ctypes.c_void_p, ctypes.c_size_t])
    assert L.STRUCTS["semidetr_add_norm_mixed"] is L.AddNormMixed
    assert lib.semidetr_abi_version() == 7
    macros = {n: int(v) for n, v in re.findall(r"^#define\s+(SEMIDETR_ROW_\w+)\s+(\d+)\s*$", open(HEADER).read(), flags=re.M)}
    assert macros == L.ROW_TYPES and sorted(macros.values()) == [0, 1, 2]
    assert [L.row_type(d) for d in (torch.float32, torch.float16, torch.bfloat16)] == \
        [macros["SEMIDETR_ROW_F32"], macros["SEMIDETR_ROW_FP16"], macros["SEMIDETR_ROW_BF16"]]
    with pytest.raises(TypeError):
        L.row_type(torch.float64)


def _harness():
    import semi_detr_amd
    L = semi_detr_amd._lib
    lib = L.lib()
    buf = (ctypes.c_float * 4096)()
    base = (ctypes.addressof(buf) + 15) & ~15
    F32, FP16, BF16 = (L.ROW_TYPES["SEMIDETR_ROW_" + n] for n in ("F32", "FP16", "BF16"))

    def block(**kw):
        p = L.AddNormMixed()
        p.rows0, p.rows1, p.dim, p.eps = 1, 2, 256, 1e-5
        for n in ("x", "weight", "bias", "y", "mean", "rstd", "grad_x", "gy"):
            setattr(p, n, base)
        p.x_stride[0], p.x_stride[1], p.gy_stride[0], p.gy_stride[1] = 512, 256, 512, 256
        for k, v in kw.items():
            if k.endswith("_stride"):
                getattr(p, k)[0], getattr(p, k)[1] = v
            else:
                setattr(p, k, v)
        return ctypes.byref(p)

    def err(rc, text):
        assert rc == -1 and text in lib.semidetr_last_error(), (rc, lib.semidetr_last_error())
    return lib, base, block, err, (F32, FP16, BF16)


def test_argument_errors_need_no_gpu():
    lib, base, block, err, (F32, FP16, BF16) = _harness()
    fwd, bwd = lib.semidetr_add_norm_forward_mixed, lib.semidetr_add_norm_backward_mixed
    # today's checks
    err(fwd(None, None, None, 0), b"null pointer")
    err(fwd(None, block(x=None), None, 0), b"null pointer")
    err(fwd(None, block(dim=128), None, 0), b"row width 128")
    err(fwd(None, block(rows1=0), None, 0), b"bad sizes")
    err(fwd(None, block(eps=float("nan")), None, 0), b"eps is NaN")
    err(fwd(None, block(y=None), None, 0), b"bias / y")
    err(bwd(None, block(gy=None), None, 0), b"gy and gq")
    err(bwd(None, block(grad_weight=base), base, 2047), b"workspace")
    assert fwd(None, block(rows0=1 << 16, rows1=1 << 15), None, 0) == -2 and b"too large" in lib.semidetr_last_error()
    assert bwd(None, block(rows0=1 << 16, rows1=1 << 15), None, 0) == -2
    # an unknown type code, of an operand and of a result, forward and backward
    err(fwd(None, block(x_type=3), None, 0), b"unknown type code 3 of x")
    err(fwd(None, block(y_type=-1), None, 0), b"unknown type code -1 of y")
    err(fwd(None, block(residual=base, residual_type=7), None, 0), b"unknown type code 7 of residual")
    err(bwd(None, block(gy_type=9), None, 0), b"unknown type code 9 of gy")
    err(bwd(None, block(grad_x_type=4), None, 0), b"unknown type code 4 of grad_x")
    # alignment per type: fp32 rows 16 bytes, 16-bit rows 8 bytes, strides multiples of 4 elements
    err(fwd(None, block(x=base + 4), None, 0), b"rows of x must be 16-byte aligned")
    err(fwd(None, block(x=base + 8), None, 0), b"rows of x must be 16-byte aligned")
    err(fwd(None, block(x_stride=(258, 256)), None, 0), b"rows of x must be 16-byte aligned")
    err(fwd(None, block(x_stride=(-512, 256)), None, 0), b"rows of x")
    err(fwd(None, block(y=base + 8), None, 0), b"rows of y must be 16-byte aligned")
    for code in (FP16, BF16):
        err(fwd(None, block(x=base + 4, x_type=code), None, 0), b"rows of x must be 8-byte aligned")
        err(fwd(None, block(x=base + 2, x_type=code), None, 0), b"rows of x must be 8-byte aligned")
        err(fwd(None, block(x_type=code, x_stride=(514, 256)), None, 0), b"rows of x must be 8-byte aligned")
        err(fwd(None, block(y=base + 4, y_type=code), None, 0), b"rows of y must be 8-byte aligned")
        err(bwd(None, block(gy=base + 4, gy_type=code), None, 0), b"rows of gy must be 8-byte aligned")
        err(bwd(None, block(grad_x=base + 12, grad_x_type=code), None, 0), b"rows of grad_x must be 8-byte aligned")
        err(bwd(None, block(gq=base, gq_stride=(512, 256), grad_pos=base + 2, grad_pos_type=code), None, 0),
            b"rows of grad_pos must be 8-byte aligned")
    # pointers that come together
    err(fwd(None, block(pos=base), None, 0), b"q and pos")
    err(fwd(None, block(q=base), None, 0), b"q and pos")
    err(bwd(None, block(grad_x=None), None, 0), b"grad_x and grad_residual")
    err(bwd(None, block(grad_residual=base), None, 0), b"grad_residual without residual")
    err(bwd(None, block(grad_pos=base), None, 0), b"grad_pos without gq")


def test_a_4_byte_aligned_address_passes_no_rule_and_an_8_byte_one_only_the_16_bit_rule():
    """The validation alone: every block below fails LATER than the alignment rule (an unknown code of ``y``, which is
    checked after ``x``), so the message says how far the block got and nothing is launched."""
    lib, base, block, err, (F32, FP16, BF16) = _harness()
    fwd = lib.semidetr_add_norm_forward_mixed
    passed_x = b"unknown type code 5 of y"
    err(fwd(None, block(x=base, x_type=F32, y_type=5), None, 0), passed_x)                 # the old rule, fp32 codes: passes
    for code in (FP16, BF16):
        err(fwd(None, block(x=base, x_type=code, y_type=5), None, 0), passed_x)
        err(fwd(None, block(x=base + 8, x_type=code, y_type=5), None, 0), passed_x)        # 8 bytes into a 16-byte line: passes
        err(fwd(None, block(x=base + 4, x_type=code, y_type=5), None, 0), b"rows of x must be 8-byte aligned")
    err(fwd(None, block(x=base + 8, x_type=F32, y_type=5), None, 0), b"rows of x must be 16-byte aligned")


def test_typed_block_pointer_refuses_the_fp32_block():
    import semi_detr_amd
    L = semi_detr_amd._lib
    with pytest.raises(ctypes.ArgumentError):
        L.lib().semidetr_add_norm_forward_mixed(None, ctypes.byref(L.AddNorm()), None, 0)
    assert L.lib().semidetr_add_norm_forward_mixed(None, ctypes.byref(L.AddNormMixed()), None, 0) == -1


def _line16(numel, dtype):
    """a tensor of ``numel`` elements whose storage starts on a 16-byte line"""
    raw = torch.zeros(numel + 16, dtype=dtype)
    skip = (-raw.data_ptr() % 16) // raw.element_size()
    out = raw[skip:skip + numel]
    assert out.data_ptr() % 16 == 0
    return out


def test_rows_native_copies_only_where_the_rule_of_the_dtype_is_violated():
    from semi_detr_amd import _lib
    for dt in (torch.float16, torch.bfloat16):
        t = _line16(3 * 5 * 256, dt).view(3, 5, 256)
        assert _lib.rows_native(t).data_ptr() == t.data_ptr() and _lib.rows_native(t).dtype == dt
        tr = t.transpose(0, 1)                                        # a transposed view stays in place
        got = _lib.rows_native(tr)
        assert got.data_ptr() == tr.data_ptr() and got.stride() == tr.stride() == (256, 1280, 1) and got.dtype == dt
        buf = _line16(3 * 5 * 264, dt).view(3, 5, 264)
        s8 = buf[:, :, 4:260]                                         # rows start 8 bytes into a 16-byte line: in place
        assert s8.data_ptr() % 16 == 8
        got = _lib.rows_native(s8)
        assert got.data_ptr() == s8.data_ptr() and got.stride() == (5 * 264, 264, 1)
        s2 = buf[:, :, 1:257]                                         # rows start 2 bytes in: copied
        got = _lib.rows_native(s2)
        assert got.data_ptr() != s2.data_ptr() and got.is_contiguous() and got.dtype == dt and torch.equal(got, s2)
        odd = _line16(3 * 5 * 258, dt).view(3, 5, 258)[:, :, :256]    # strides that are no multiple of 4 elements: copied
        assert _lib.rows_native(odd).data_ptr() != odd.data_ptr()
        col = _line16(3 * 256 * 5, dt).view(3, 256, 5).transpose(1, 2)     # last stride not 1: copied
        assert _lib.rows_native(col).is_contiguous()
    f = _line16(3 * 5 * 264, torch.float32).view(3, 5, 264)
    assert _lib.rows_native(f[:, :, 4:260]).data_ptr() == f[:, :, 4:260].data_ptr()       # 16 bytes in: in place
    assert _lib.rows_native(f[:, :, 2:258]).data_ptr() != f[:, :, 2:258].data_ptr()       # 8 bytes in: fp32 rows are copied
    assert not _lib.rows_native(f.requires_grad_(True)).requires_grad
    with pytest.raises(TypeError):
        _lib.rows_native(torch.zeros(1, 1, 256, dtype=torch.float64))
