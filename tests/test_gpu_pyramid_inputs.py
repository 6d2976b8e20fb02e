"""GPU: semi_detr_amd.pyramid_inputs (csrc/pyramid_inputs.hip) against the float64 statement tests/pyramid_inputs_ref64.py and
against the stock chain (tests/pyramid_inputs_torch_restated.py) run on the GPU: every case of tests/pyramid_inputs_cases.py
through the entry point its inputs name (image sizes or given masks) and through the C ABI; ``pos`` and the ``level_embed``
gradient within the derived bounds, nothing excluded; masks, valid ratios, reference points and the index tensors bit for bit
equal to the stock chain's.  Before each call NaN-filled buffers of the results' sizes are freed into the caching allocator, so
an element a kernel does not write shows.  The statement's dim_t tables are the ones the mirror hands the kernel.
"""
import ctypes
import importlib

import numpy as np
import pytest
import torch

import pyramid_inputs_cases as C
import pyramid_inputs_ref64 as R
import pyramid_inputs_torch_restated as T

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TORCH = {"fp32": torch.float32, "fp16": torch.float16, "bf16": torch.bfloat16}


def P():
    return importlib.import_module("semi_detr_amd.pyramid_inputs")


def _poison(*shapes):
    junk = [torch.full(s, float("nan"), dtype=torch.float32, device=DEV) for s in shapes for _ in range(2)]
    del junk


def _np(t):
    t = t.detach()
    return (t.float() if t.is_floating_point() else t).cpu().numpy()


def _encoding(case):
    return P().SinePositionalEncodingHW(**case["enc"])


def _tables(case):
    enc = _encoding(case)
    return _np(P().dim_t(DEV, enc.temperatureH)), _np(P().dim_t(DEV, enc.temperatureW))


def _level_embed(case):
    if case["level_embed"] is None:
        return None
    return torch.from_numpy(case["level_embed"]).to(DEV).to(TORCH[case["le_dtype"]]).requires_grad_(True)


def _masks(case):
    return [torch.from_numpy(np.asarray(m)).to(DEV) for m in case["masks"]]


def run(case):
    """the case through its entry point and autograd -> the dict ``R.check`` reads, and the raw result tensors"""
    le = _level_embed(case)
    n, rows, levels = case["g"].shape[0], case["g"].shape[1], len(case["shapes"])
    _poison((n, rows, 256), (n, rows, levels, 2), (n, levels, 2))
    kw = dict(level_embed=le, dtype=TORCH[case["dtype"]], want_reference_points=True)
    if case["masks"] is not None:
        res = P().pyramid_inputs_from_masks(_masks(case), _encoding(case), **kw)
    else:
        res = P().pyramid_inputs(case["img_shapes"], case["input"], case["shapes"], _encoding(case), device=DEV, **kw)
    assert res.pos.dtype == TORCH[case["dtype"]] and res.pos.is_contiguous() and res.pos.shape == (n, rows, 256)
    assert res.mask_flatten.dtype == torch.bool and res.valid_ratios.dtype == res.reference_points.dtype == torch.float32
    assert res.reference_points.shape == (n, rows, levels, 2) and res.reference_points.is_contiguous()
    assert [tuple(m.shape[1:]) for m in res.mlvl_masks] == case["shapes"]
    assert torch.equal(torch.cat([m.flatten(1) for m in res.mlvl_masks], 1), res.mask_flatten)
    assert all(m.data_ptr() == res.mask_flatten[:, int(s):].data_ptr() for m, s in zip(res.mlvl_masks, res.level_start_index.tolist()))
    assert res.pos.requires_grad == (le is not None) and not res.valid_ratios.requires_grad and not res.reference_points.requires_grad
    got = {k: _np(getattr(res, k)) for k in ("pos", "mask_flatten", "valid_ratios", "reference_points", "spatial_shapes",
                                               "level_start_index")}
    raw = [res.pos.detach(), res.mask_flatten, res.valid_ratios, res.reference_points]
    # the backward launches: through autograd where g has pos's dtype, and on their own with the case's g
    g = torch.from_numpy(case["g"]).to(DEV).to(TORCH[case["g_dtype"]])
    if le is not None:
        _poison((levels, 256))
        grad = P().pyramid_inputs_backward(g, case["shapes"], le.dtype)
        assert grad.dtype == le.dtype and grad.shape == (levels, 256)
        if case["g_dtype"] == case["dtype"]:
            res.pos.backward(g)
            assert le.grad.dtype == le.dtype and le.grad.view(torch.uint8).equal(grad.view(torch.uint8))
        got["grad"] = _np(grad)
        raw.append(grad)
    return got, raw, res


def run_c_abi(case):
    """the same through the C ABI alone: the parameter block filled by hand, the workspace from the size query"""
    from semi_detr_amd import _lib
    lib = _lib.lib()
    enc, le = _encoding(case), _level_embed(case)
    n, rows, levels = case["g"].shape[0], case["g"].shape[1], len(case["shapes"])
    p = _lib.PyramidInputsBlock()
    p.batch, p.levels, p.tokens_per_image, start = n, levels, rows, 0
    for l, (h, w) in enumerate(case["shapes"]):
        p.h[l], p.w[l], p.start[l] = h, w, start
        start += h * w
    keep = []
    if case["masks"] is not None:
        keep = [m.contiguous() for m in _masks(case)]
        for l, m in enumerate(keep):
            p.masks[l] = m.data_ptr()
    else:
        p.from_sizes, (p.input_h, p.input_w) = 1, case["input"]
        for i, (img_h, img_w) in enumerate(case["img_shapes"]):
            p.img_h[i], p.img_w[i] = img_h, img_w
    p.normalize, p.offset, p.eps, p.scale = int(enc.normalize), enc.offset, enc.eps, enc.scale
    ty, tx = P().dim_t(DEV, enc.temperatureH), P().dim_t(DEV, enc.temperatureW)
    p.dim_ty, p.dim_tx = ty.data_ptr(), tx.data_ptr()
    if le is not None:
        p.level_embed, p.level_embed_type = le.data_ptr(), _lib.row_type(le.dtype)
    _poison((n, rows, 256), (n, rows, levels, 2))
    pos = torch.empty((n, rows, 256), dtype=TORCH[case["dtype"]], device=DEV)
    mask = torch.empty((n, rows), dtype=torch.bool, device=DEV)
    vr = torch.empty((n, levels, 2), dtype=torch.float32, device=DEV)
    ref = torch.empty((n, rows, levels, 2), dtype=torch.float32, device=DEV)
    p.pos, p.pos_type, p.mask_flatten, p.valid_ratios, p.reference_points = \
        pos.data_ptr(), _lib.row_type(pos.dtype), mask.data_ptr(), vr.data_ptr(), ref.data_ptr()
    nbytes = lib.semidetr_pyramid_inputs_workspace_bytes(ctypes.byref(p), 0)
    assert nbytes == 4 * n * rows
    work = torch.empty((nbytes,), dtype=torch.uint8, device=DEV)
    stream = _lib.current_stream_ptr()
    _lib.check(lib.semidetr_pyramid_inputs_forward(stream, ctypes.byref(p), work.data_ptr(), nbytes), "forward")
    raw = [pos, mask, vr, ref]
    if le is not None:
        g = torch.from_numpy(case["g"]).to(DEV).to(TORCH[case["g_dtype"]])
        grad = torch.empty((levels, 256), dtype=le.dtype, device=DEV)
        p.g, p.g_type, p.grad_level_embed = g.data_ptr(), _lib.row_type(g.dtype), grad.data_ptr()
        p.g_stride[0], p.g_stride[1] = g.stride(0), g.stride(1)
        nbytes = lib.semidetr_pyramid_inputs_workspace_bytes(ctypes.byref(p), 1)
        work = torch.empty((nbytes,), dtype=torch.uint8, device=DEV)
        _lib.check(lib.semidetr_pyramid_inputs_backward(stream, ctypes.byref(p), work.data_ptr(), nbytes), "backward")
        raw.append(grad)
    torch.cuda.synchronize()
    return raw


def stock(case):
    enc = T.SineEncodingHW(**case["enc"])
    le = None if case["level_embed"] is None else torch.from_numpy(case["level_embed"]).to(DEV)
    if case["masks"] is not None:
        return T.chain(_masks(case), enc, le)
    return T.chain_from_sizes(case["img_shapes"], case["input"], case["shapes"], enc, le, DEV)


def want_masks(case):
    return T.level_masks(case["img_shapes"], case["input"], case["shapes"], DEV)


def _same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and a.contiguous().view(torch.uint8).equal(b.contiguous().view(torch.uint8))


@pytest.mark.parametrize("name", C.names())
def test_case_within_bounds_and_equal_to_the_stock_chain(name):
    case = C.cases()[name]
    got, raw, res = run(case)
    ty, tx = _tables(case)
    ratios = R.check(case, got, ty, tx, name)
    print(R.table(name, ratios))
    want = stock(case)
    for key in R.BITWISE:
        R.same_bits(f"{name} {key} against the stock chain on the GPU", got[key], _np(want[key]))
    assert res.spatial_shapes.dtype == res.level_start_index.dtype == torch.long
    print(f"  {name}: pos bit-equal to the stock chain: {_same_bits(res.pos.detach().float(), want['pos'].to(res.pos.dtype).float())}")
    if case["masks"] is None:                     # the other entry point: the stock chain's level masks, given
        other = P().pyramid_inputs_from_masks(want_masks(case), _encoding(case), level_embed=_level_embed(case),
                                              dtype=TORCH[case["dtype"]], want_reference_points=True)
        for a, b in zip(raw[:4], (other.pos.detach(), other.mask_flatten, other.valid_ratios, other.reference_points)):
            assert _same_bits(a, b), "pyramid_inputs and pyramid_inputs_from_masks differ"
    # the C ABI alone gives the same bits as the entry point
    for i, (a, b) in enumerate(zip(raw, run_c_abi(case))):
        assert _same_bits(a, b), f"result {i} differs between the entry point and the C ABI"
    if name == "masks_one_full":
        ref = got["reference_points"]
        assert (got["valid_ratios"][1] == 0).all() and not np.isfinite(ref[1]).any() and np.isfinite(ref[0]).all()
        stock_ref = _np(want["reference_points"])
        assert np.array_equal(np.isnan(ref), np.isnan(stock_ref)) and np.array_equal(np.isposinf(ref), np.isposinf(stock_ref))


@pytest.mark.parametrize("name", ["padded_batch", "real_divisor", "wide_tall_masks", "pos_bf16"])
def test_two_runs_are_bitwise_equal(name):
    case = C.cases()[name]
    (_, a, _), (_, b, _) = run(case), run(case)
    assert len(a) == len(b) == 5
    for x, y in zip(a, b):
        assert _same_bits(x, y), "not bit-identical from run to run"


def test_the_tables_are_the_references_expression():
    t = torch.arange(128, dtype=torch.float32, device=DEV)
    for temperature in (20, 10000):
        assert torch.equal(P().dim_t(DEV, temperature), temperature ** (2 * (t // 2) / 128))
        assert P().dim_t(DEV, temperature) is P().dim_t(torch.device(DEV), temperature)


def test_the_module_mirror_against_the_restated_module():
    import semi_detr_amd as s
    case = dict(C.cases()["masks_random"])
    for enc_kw in (dict(case["enc"]), dict(case["enc"], normalize=False, temperatureH=10000, temperatureW=10000)):
        mine, theirs = s.SinePositionalEncodingHW(**enc_kw), T.SineEncodingHW(**enc_kw)
        ty, tx = _np(P().dim_t(DEV, enc_kw["temperatureH"])), _np(P().dim_t(DEV, enc_kw["temperatureW"]))
        for lvl, m in enumerate(case["masks"]):
            mask = torch.from_numpy(m).to(DEV)
            out, want = mine(mask), theirs(mask)
            assert out.shape == want.shape == (m.shape[0], 256, m.shape[1], m.shape[2]) and out.dtype == want.dtype == torch.float32
            one = dict(case, masks=[m], shapes=[tuple(m.shape[1:])], level_embed=None, enc=enc_kw)
            a = R.pos(one, ty, tx)
            for side, t in (("mirror", out), ("restated", want)):
                R.within(f"{side} level {lvl}", _np(t.permute(0, 2, 3, 1).flatten(1, 2)), a)
            assert torch.equal(mine(mask.to(torch.uint8) * 3), out), "any non-zero byte is a masked pixel"


def _kernels(fn):
    from torch.profiler import ProfilerActivity, profile
    fn()
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    names = [e.name for e in prof.events() if "cuda" in str(e.device_type).lower()]
    return [n for n in names if "memcpy" not in n.lower() and "memset" not in n.lower()], \
        [n for n in names if "memset" in n.lower()]


def test_one_call_is_two_launches_each_way_and_none_of_torchs():
    case = C.cases()["padded_batch"]
    enc = _encoding(case)
    le = _level_embed(case)
    g = torch.from_numpy(case["g"]).to(DEV)
    masks = T.level_masks(case["img_shapes"], case["input"], case["shapes"], DEV)
    state = {}

    def forward():
        state["res"] = P().pyramid_inputs(case["img_shapes"], case["input"], case["shapes"], enc, level_embed=le,
                                          want_reference_points=True, device=DEV)

    def forward_masks():
        P().pyramid_inputs_from_masks(masks, enc, level_embed=le, want_reference_points=True)

    def backward():
        state["grad"] = torch.autograd.grad([state["res"].pos], [le], [g], retain_graph=True)[0]

    for fn, allowed in ((forward, ("pyramid_scan_kernel", "pyramid_emit_kernel")),
                        (forward_masks, ("pyramid_scan_kernel", "pyramid_emit_kernel")),
                        (backward, ("pyramid_grad_rows_kernel", "pyramid_grad_sum_kernel"))):
        kernels, memsets = _kernels(fn)
        print(f"  {fn.__name__}: {kernels}")
        assert not memsets, memsets
        # spatial_shapes / level_start_index travel as two pinned copies (input_proj.pyramid_index): copies, not kernels
        assert len(kernels) == 2 and all(any(a in k for a in allowed) for k in kernels), kernels
    assert state["grad"].shape == le.shape


def test_the_hand_off_to_the_input_projection_and_the_encoder_is_bitwise():
    import detector_chain_cases as DC
    import semi_detr_amd as s
    model = DC.build_model("init").to(DEV)
    hip = DC.hip_model(model)
    DC.set_context(hip, "fp32_fused")
    shapes = DC.PYRAMIDS["patch"]
    feats = [f.to(DEV) for f in DC.inputs("patch")["feats"]]
    img_shapes, batch_input_shape = [(96, 128), (70, 101)], (96, 128)
    enc = s.SinePositionalEncodingHW(128, temperatureH=20, temperatureW=20, normalize=True)
    level_embed = torch.randn(DC.LEVELS, DC.D, generator=torch.Generator().manual_seed(3)).to(DEV)
    res = s.pyramid_inputs(img_shapes, batch_input_shape, shapes, enc, level_embed=level_embed, want_reference_points=True, device=DEV)
    want = T.chain_from_sizes(img_shapes, batch_input_shape, shapes, T.SineEncodingHW(128, 20, 20, True), level_embed, DEV)
    for key in ("mask_flatten", "valid_ratios", "reference_points"):
        assert _same_bits(getattr(res, key), want[key]), key
    assert res.mask_flatten.any() and not res.mask_flatten.all()
    pos_equal = _same_bits(res.pos, want["pos"])
    print(f"  pos bit-equal to the stock chain: {pos_equal}; max |diff| {float((res.pos - want['pos']).abs().max()):.3e}")
    stock_pos = want["pos"] if pos_equal else res.pos        # the stock side is fed the stock tensors wherever they are bit-equal

    def through(pos, pad, vr, ref):
        tokens, q, sh, starts, _ = s.project_pyramid(hip.input_proj, feats, DC.LEVELS, pos=pos)
        return q, s.encoder_forward(hip.enc, tokens, pos, sh, starts, vr, pad, query=q, reference_points=ref)[0], sh, starts
    # the convs and GEMMs underneath are torch's: they are asked for their reproducible kernels, so that two calls on equal bits
    # can be compared bit for bit at all (the encoder's kernel choice is pinned for the same reason)
    s._lib.set_forward_policy(DC.POLICY["patch"])
    flags = (torch.are_deterministic_algorithms_enabled(), torch.is_deterministic_algorithms_warn_only_enabled(),
             torch.backends.cudnn.deterministic, torch.backends.cudnn.benchmark)
    torch.use_deterministic_algorithms(True, warn_only=True)
    torch.backends.cudnn.deterministic, torch.backends.cudnn.benchmark = True, False
    try:
        with torch.no_grad():
            through(res.pos, res.mask_flatten, res.valid_ratios, res.reference_points)      # the libraries choose their kernels
            q_mine, mine, sh, starts = through(res.pos, res.mask_flatten, res.valid_ratios, res.reference_points)
            q_again, again, _, _ = through(res.pos, res.mask_flatten, res.valid_ratios, res.reference_points)
            q_theirs, theirs, _, _ = through(stock_pos, want["mask_flatten"], want["valid_ratios"], want["reference_points"])
            _, own_ref, _, _ = through(stock_pos, want["mask_flatten"], want["valid_ratios"], None)   # the encoder's own call
    finally:
        s._lib.set_forward_policy("adaptive")
        torch.use_deterministic_algorithms(flags[0], warn_only=flags[1])
        torch.backends.cudnn.deterministic, torch.backends.cudnn.benchmark = flags[2], flags[3]
    assert torch.equal(sh, res.spatial_shapes) and torch.equal(starts, res.level_start_index)
    print(f"  q: again {_same_bits(q_mine, q_again)} stock {_same_bits(q_mine, q_theirs)}; memory: again {_same_bits(mine, again)} "
          f"stock {_same_bits(mine, theirs)} own reference points {_same_bits(mine, own_ref)}; "
          f"max |diff| {float((mine - theirs).abs().max()):.3e}")
    assert torch.isfinite(mine).all() and _same_bits(q_mine, q_again) and _same_bits(mine, again), "the chain itself is not reproducible"
    assert _same_bits(q_mine, q_theirs) and _same_bits(mine, theirs) and _same_bits(mine, own_ref)


class _Head(torch.nn.Module):
    """what ``head_inputs`` reads of the detection head"""
    def __init__(self, levels, embed_rows):
        super().__init__()
        self.positional_encoding = P().SinePositionalEncodingHW(128, temperatureH=20, temperatureW=20, normalize=True)
        self.transformer = torch.nn.Module()
        self.transformer.num_feature_levels = levels
        self.transformer.level_embed = None if embed_rows is None else torch.nn.Parameter(torch.randn(embed_rows, 256))
        self.anchor = torch.nn.Parameter(torch.zeros(1))          # a head always has parameters: its device is theirs


@pytest.mark.parametrize("levels, embed_rows", [(4, 4), (4, 6), (1, 4), (4, None)])
def test_head_inputs_reads_the_head_and_the_img_metas(levels, embed_rows):
    import semi_detr_amd as s
    case = C.cases()["padded_batch"]
    shapes = case["shapes"][:levels]
    head = _Head(levels, embed_rows).to(DEV)
    metas = [dict(batch_input_shape=case["input"], img_shape=(h, w, 3)) for h, w in case["img_shapes"]]
    res = s.head_inputs(head, shapes, metas)
    le = head.transformer.level_embed
    used = le is not None and levels > 1                       # the transformer's rule
    want = T.chain_from_sizes(case["img_shapes"], case["input"], shapes, T.SineEncodingHW(128, 20, 20, True),
                              le.detach() if used else None, DEV)
    for key in ("mask_flatten", "valid_ratios", "reference_points", "spatial_shapes", "level_start_index"):
        assert _same_bits(getattr(res, key), want[key]), key
    one = dict(case, shapes=shapes, level_embed=_np(le)[:levels] if used else None, g=case["g"][:, :C.rows_of(shapes)])
    enc = head.positional_encoding
    R.check(one, {"pos": _np(res.pos)}, _np(P().dim_t(DEV, enc.temperatureH)), _np(P().dim_t(DEV, enc.temperatureW)), "head_inputs")
    assert res.pos.device == le.device if le is not None else res.pos.is_cuda
    assert res.pos.requires_grad == used
    if used:
        g = torch.from_numpy(one["g"]).to(DEV)
        res.pos.backward(g)
        assert le.grad.shape == le.shape and not le.grad[levels:].any(), "rows no level uses get a zero gradient"
        R.within("head_inputs grad", _np(le.grad[:levels]), R.grad(dict(one, le_dtype="fp32")))
