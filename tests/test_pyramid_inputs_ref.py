"""CPU: the float64 statement of the pyramid inputs (tests/pyramid_inputs_ref64.py) against stock torch and the reference's
recorded results, so that its bounds are ones stock torch itself meets; the host-side nearest rule against ``F.interpolate``;
every mutant of the statement rejected; the host refusals of ``semi_detr_amd.pyramid_inputs``; the module mirror's surface."""
import importlib
import math
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import pyramid_inputs_cases as C
import pyramid_inputs_ref64 as R
import pyramid_inputs_torch_restated as T

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "pyramid_inputs.npz")
TORCH = {"fp32": torch.float32, "fp16": torch.float16, "bf16": torch.bfloat16}


def tables(case, device="cpu"):
    enc = T.SineEncodingHW(**case["enc"])
    return enc.divisors(enc.temperatureH, device).cpu().numpy(), enc.divisors(enc.temperatureW, device).cpu().numpy()


def stock(case, device="cpu"):
    """the restated chain in torch's fp32 on ``device`` -> the dict ``R.check`` reads (``pos`` rounded once to the case's dtype,
    as the op's contract says, and the gradient from autograd)"""
    enc = T.SineEncodingHW(**case["enc"])
    le = None if case["level_embed"] is None else torch.from_numpy(case["level_embed"]).to(device).requires_grad_(True)
    if case["masks"] is not None:
        out = T.chain([torch.from_numpy(np.asarray(m)).to(device) for m in case["masks"]], enc, le)
    else:
        out = T.chain_from_sizes(case["img_shapes"], case["input"], case["shapes"], enc, le, device)
    got = {k: v.detach().cpu().numpy() for k, v in out.items()}
    got["pos"] = out["pos"].detach().to(TORCH[case["dtype"]]).float().cpu().numpy()
    if le is not None:
        (out["pos"] * torch.from_numpy(case["g"]).to(device)).sum().backward()
        got["grad"] = le.grad.to(TORCH[case["le_dtype"]]).float().cpu().numpy()
    return got


@pytest.mark.parametrize("name", C.names())
def test_stock_torch_is_admissible(name):
    case = C.cases()[name]
    ty, tx = tables(case)
    print(R.table(name, R.check(case, stock(case), ty, tx, name, rule="divide")))     # torch on the CPU
    print(R.table(name + " (numpy fp32)", R.check(case, R.evaluate(case, ty, tx), ty, tx, name)))


def test_the_recorded_reference_results_are_admissible():
    z = np.load(GOLDEN)
    recorded = sorted({k.split(".")[0] for k in z.files})
    assert len(recorded) >= 6
    for name in recorded:
        case = C.cases()[name]
        rows = z[f"{name}.rows"]
        ty, tx = z[f"{name}.dim_ty"], z[f"{name}.dim_tx"]
        want = R.evaluate(case, ty, tx, rule="divide")              # recorded on the CPU
        for key in ("mask_flatten", "valid_ratios", "spatial_shapes", "level_start_index"):
            R.same_bits(f"{name} {key}", z[f"{name}.{key}"], want[key])
        R.same_bits(f"{name} reference_points", z[f"{name}.reference_points"], want["reference_points"][:, rows])
        a = R.pos(case, ty, tx)
        R.within(f"{name} pos", z[f"{name}.pos"], (a[0][:, rows], a[1][:, rows]))
        if case["level_embed"] is not None:
            R.within(f"{name} grad", z[f"{name}.grad"], R.grad(case))
        assert np.array_equal(ty, tables(case)[0]) and np.array_equal(tx, tables(case)[1])


def test_the_nearest_rule_is_f_interpolates():
    P = importlib.import_module("semi_detr_amd.pyramid_inputs")         # the package exports the function of the same name
    for size, outs in C.NEAREST_SIZES:
        for out in outs:
            src = np.array([P.nearest_source_index(d, size, out) for d in range(out)])
            assert np.array_equal(src, [R.nearest_src(d, size, out) for d in range(out)])
            column = torch.ones(size + 1, size, 1)                  # image height v: rows v .. are padding
            for v in range(size + 1):
                column[v, :v] = 0
            want = F.interpolate(column[None], size=(out, 1)).bool()[0, :, :, 0].numpy()
            got = src[None, :] >= np.arange(size + 1)[:, None]
            assert np.array_equal(got, want), (size, out)
            assert all(np.array_equal(np.sort(row), row) for row in got), "the valid set of a level is a prefix"
    # no destination index of the real pyramid gives an exact-integer product; 93 -> 12 does (pyramid_inputs_cases.exact_product)
    for size, outs in ((1333, (167, 84, 42, 21)), (37, (5, 3, 2))):
        for out in outs:
            p = np.arange(1, out, dtype=np.float32) * (np.float32(size) / np.float32(out))
            assert not (p == np.floor(p)).any()
    assert np.float32(4) * (np.float32(93) / np.float32(12)) == 31
    assert P.level_mask(41, 31, 67, 93, 9, 12) == R.masks_of(dict(masks=None, input=(67, 93), shapes=[(9, 12)], img_shapes=[(41, 31)]))[0][0].tolist()


@pytest.mark.parametrize("mutant", R.MUTANTS)
def test_every_mutant_is_rejected(mutant):
    rejected = []
    for name, case in C.cases().items():
        ty, tx = tables(case)
        try:
            R.check(case, R.evaluate(case, ty, tx, mutant), ty, tx, name)
        except R.Inadmissible:
            rejected.append(name)
    print(f"  {mutant}: rejected on {rejected}")
    assert rejected


class _Cuda:
    """stands for a GPU tensor in the host checks, which run before anything touches the device"""
    def __init__(self, shape, dtype=torch.float32):
        self.shape, self.dtype, self.device = shape, dtype, torch.device("cuda", 0)

    def dim(self):
        return len(self.shape)


def test_host_refusals():
    from semi_detr_amd import _lib
    P = importlib.import_module("semi_detr_amd.pyramid_inputs")
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "semidetr_hip.h")).read()
    macro = lambda n: int(re.search(r"#define\s+%s\s+(\d+)" % n, header).group(1))       # noqa: E731
    assert (_lib.PYR_MAX_LEVELS, _lib.PYR_MAX_BATCH) == (macro("SEMIDETR_PYR_MAX_LEVELS"), macro("SEMIDETR_PYR_MAX_BATCH")) == (8, 64)
    enc = P.SinePositionalEncodingHW(128, normalize=True)
    dev = torch.device("cuda", 0)
    with pytest.raises(NotImplementedError, match=r"num_feats=64 \(only 128 is built"):
        P.pyramid_inputs([(8, 8)], (8, 8), [(2, 2)], P.SinePositionalEncodingHW(64), device=dev)
    with pytest.raises(NotImplementedError, match=r"9 levels \(1 \.\. 8\)"):
        P.pyramid_inputs([(8, 8)], (8, 8), [(2, 2)] * 9, enc, device=dev)
    with pytest.raises(NotImplementedError, match=r"65 images \(1 \.\. 64: the image sizes travel by value"):
        P.pyramid_inputs([(8, 8)] * 65, (8, 8), [(2, 2)], enc, device=dev)
    with pytest.raises(NotImplementedError, match=r"must live on the GPU, not on cpu"):
        P.pyramid_inputs([(8, 8)], (8, 8), [(2, 2)], enc, device="cpu")
    with pytest.raises(NotImplementedError, match=r"must live on the GPU, not on cpu"):
        P.pyramid_inputs_from_masks([torch.zeros(1, 2, 2, dtype=torch.bool)], enc)
    with pytest.raises(NotImplementedError, match=r"level 0 is \(65536, 1\); sides of 1 \.\. 65535"):
        P.pyramid_inputs([(8, 8)], (8, 8), [(65536, 1)], enc, device=dev)
    with pytest.raises(NotImplementedError, match=r"normalize with eps=0"):
        P.pyramid_inputs([(8, 8)], (8, 8), [(2, 2)], P.SinePositionalEncodingHW(128, normalize=True, eps=0), device=dev)
    with pytest.raises(ValueError, match=r"image 0 is \(9, 8\), outside batch_input_shape \(8, 8\)"):
        P.pyramid_inputs([(9, 8)], (8, 8), [(2, 2)], enc, device=dev)
    with pytest.raises(ValueError, match=r"level_embed is \(1, 256\)"):
        P.pyramid_inputs([(8, 8)], (8, 8), [(2, 2), (1, 1)], enc, level_embed=_Cuda((1, 256)), device=dev)
    # the library refuses the same before any launch
    lib, p = _lib.lib(), _lib.PyramidInputsBlock()
    fwd = lib.semidetr_pyramid_inputs_forward
    p.batch, p.levels, p.tokens_per_image = 65, 1, 4
    p.h[0], p.w[0] = 2, 2
    assert lib.semidetr_pyramid_inputs_workspace_bytes(p, 0) == 0
    assert fwd(None, p, None, 0) == -1 and b"65 images (1 .. 64" in lib.semidetr_last_error()
    p.batch, p.h[0] = 2, 65536
    assert fwd(None, p, None, 0) == -1 and b"1 .. 65535 each" in lib.semidetr_last_error()
    p.h[0] = 2
    assert lib.semidetr_pyramid_inputs_workspace_bytes(p, 0) == 2 * 2 * 4 * 2
    assert lib.semidetr_pyramid_inputs_workspace_bytes(p, 1) == 2 * 256 * 4
    assert fwd(None, p, None, 0) == -1 and b"workspace null" in lib.semidetr_last_error()
    assert fwd(None, None, None, 0) == -1 and b"null pointer" in lib.semidetr_last_error()


def test_the_module_mirror_has_the_references_surface():
    import semi_detr_amd as s
    m = s.SinePositionalEncodingHW(128, temperatureH=20, temperatureW=20, normalize=True)
    assert repr(m) == f"SinePositionalEncodingHW(num_feats=128, temperatureH=20, temperatureW=20, normalize=True, scale={2 * math.pi}, eps=1e-06)"
    d = s.SinePositionalEncodingHW(num_feats=128)
    assert (d.num_feats, d.temperatureH, d.temperatureW, d.normalize, d.scale, d.eps, d.offset) == \
        (128, 10000, 10000, False, 2 * math.pi, 1e-6, 0.)
    full = s.SinePositionalEncodingHW(128, 20, 30, True, 3.0, 1e-5, -0.5, None)
    assert (full.temperatureW, full.scale, full.eps, full.offset) == (30, 3.0, 1e-5, -0.5) and not list(full.parameters())
    with pytest.raises(AssertionError, match="needs a float or int scale"):
        s.SinePositionalEncodingHW(128, normalize=True, scale="2pi")
    from semi_detr_amd import registry

    class Registry(dict):
        def register_module(self, name, force, module):
            self[name] = module
    given = Registry()
    done, _ = registry.register_all(positional_encoding=given)
    assert "SinePositionalEncodingHW" in done and given == {"SinePositionalEncodingHW": s.SinePositionalEncodingHW}
