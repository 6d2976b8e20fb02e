"""CPU: the exact MSDA backward's accumulator and model.

  * csrc/msda_exactsum.h, built alone for the host (tests/host/msda_exactsum_host_check.cpp through
    tools/msda_exactsum_host_check.sh, the plain build; the same program under AddressSanitizer + UBSan is that script without
    CXXFLAGS, run by hand on a CPU machine), bit for bit against fractions.Fraction;
  * the numpy model of the route (tests/msda_exact_ref.py) is permutation-invariant where sequential fp32 summation of the very
    same contributions is not -- so the GPU invariance tests discriminate -- and meets msda_ref64's grad_value bound with
    n = DEPTH + 1 (derived in msda_exact_ref's docstring);
  * the two C-ABI symbols are declared, exported and refuse what the header says they refuse, without a GPU.
"""
import ctypes
import os
import subprocess
from fractions import Fraction

import numpy as np
import pytest

import msda_exact_cases as C
import msda_exact_ref as X
import msda_ref64 as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _f32(x):
    return np.asarray(x, np.float32).reshape(-1)


def _hex(values):
    return " ".join("%08x" % b for b in X.bits_of(values))


def run_accumulator(requests):
    """requests: list of ("S", values) or ("M", k, values) -> list of result bit patterns, one process for all of them."""
    lines = ["S " + _hex(r[1]) if r[0] == "S" else "M %d %s" % (r[1], _hex(r[2])) for r in requests]
    out = subprocess.run(["bash", os.path.join(ROOT, "tools", "msda_exactsum_host_check.sh")], env=dict(os.environ, CXXFLAGS=""),
                         input="\n".join(lines) + "\n", capture_output=True, text=True)
    assert out.returncode == 0 and "msda_exactsum_host_check: ok" in out.stdout, out.stdout + out.stderr
    got = [int(x, 16) for x in out.stdout.split("\n")[:len(requests)]]
    assert len(got) == len(requests)
    return got


def _p(e):
    return np.float32(2.0) ** np.float32(e) if -126 <= e <= 127 else np.float32(np.ldexp(1.0, e))


MAXF = np.finfo(np.float32).max
INF, NAN = np.float32(np.inf), np.float32(np.nan)


def accumulator_vectors():
    rng = np.random.default_rng(7)
    vecs = {}
    # random signs, mantissas and exponents over the whole finite range, subnormals included
    for i, n in enumerate((1, 2, 3, 17, 64, 300)):
        bits = (rng.integers(0, 2, n).astype(np.uint32) << 31) | (rng.integers(0, 255, n).astype(np.uint32) << 23) | \
            rng.integers(0, 1 << 23, n).astype(np.uint32)
        vecs["random%d" % i] = bits.view(np.float32)
    vecs["narrow"] = (rng.standard_normal(200) * 1e-3).astype(np.float32)
    vecs["cancel"] = [_p(100), -_p(100), _p(-100)]
    vecs["cancel_sub"] = [_p(127), _p(-149), -_p(127)]
    # exact ties of the final rounding: 1 + 2^-24 (down to even), 1 + 2^-23 + 2^-24 (up to even), and one unit either side
    vecs["tie_down"] = [1.0, _p(-24)]
    vecs["tie_up"] = [1.0, _p(-23), _p(-24)]
    vecs["tie_down_plus"] = [1.0, _p(-24), _p(-149)]
    vecs["tie_up_minus"] = [1.0, _p(-23), _p(-24), -_p(-149)]
    vecs["tie_neg"] = [-1.0, -_p(-24)]
    vecs["tie_carry"] = [np.nextafter(np.float32(2), np.float32(0)), _p(-24)]            # rounds up into the next binade
    # overflow: the exact sum is finite although a sequential sum passes through inf, and the reverse
    vecs["finite_via_inf"] = [MAXF, MAXF, -MAXF]
    vecs["finite_via_inf_neg"] = [-MAXF, -MAXF, MAXF, _p(-149)]
    vecs["inf_exact"] = [MAXF, _p(103)]                          # max + half an ulp of max: the tie rounds to 2^128 = inf
    vecs["inf_not_yet"] = [MAXF, np.nextafter(_p(103), np.float32(0))]
    # each addend alone is absorbed by a sequential sum (a quarter ulp of max), together they are one ulp: the exact sum overflows
    vecs["inf_only_exact"] = [MAXF] + [_p(102)] * 4
    vecs["neg_inf_exact"] = [-MAXF, -_p(103)]
    # subnormal results
    vecs["sub_sum"] = [_p(-149)] * 5
    vecs["sub_from_normals"] = [_p(-126), -np.nextafter(_p(-126), np.float32(0))]
    vecs["sub_to_normal"] = [np.nextafter(_p(-126), np.float32(0)), _p(-149)]
    vecs["zero"] = [1.5, -1.5]
    vecs["empty"] = []
    # the three non-finite rules
    vecs["nan"] = [1.0, NAN, 2.0]
    vecs["nan_and_inf"] = [INF, NAN]
    vecs["both_inf"] = [INF, 1.0, -INF]
    vecs["pos_inf"] = [MAXF, INF, -MAXF, -MAXF]
    vecs["neg_inf"] = [-INF, MAXF, MAXF]
    return {k: _f32(v) for k, v in vecs.items()}


def test_accumulator_matches_the_fraction_model_bit_for_bit():
    vecs = accumulator_vectors()
    rng = np.random.default_rng(8)
    reqs, want, names = [], [], []
    for name, v in vecs.items():
        w = X.exact_sum_bits(v)
        perm = rng.permutation(len(v))
        for label, r in (("seq", ("S", v)), ("perm", ("S", v[perm])), ("reversed", ("S", v[::-1])), ("merge3", ("M", 3, v)),
                         ("merge8", ("M", 8, v[perm]))):
            reqs.append(r)
            want.append(w)
            names.append(name + ":" + label)
    got = run_accumulator(reqs)
    bad = [(n, "%08x" % g, "%08x" % w) for n, g, w in zip(names, got, want) if g != w]
    assert not bad, bad
    # the vectors do what their names say: what a sequential fp32 sum makes of them
    seq = {k: X.sequential_sum_bits(v) for k, v in vecs.items()}
    assert seq["finite_via_inf"] == 0x7f800000 and X.exact_sum_bits(vecs["finite_via_inf"]) == int(X.bits_of(MAXF)[0])
    assert seq["inf_only_exact"] == int(X.bits_of(MAXF)[0]) and X.exact_sum_bits(vecs["inf_only_exact"]) == 0x7f800000
    assert X.exact_sum_bits(vecs["inf_exact"]) == 0x7f800000 and X.exact_sum_bits(vecs["inf_not_yet"]) == int(X.bits_of(MAXF)[0])
    assert X.exact_sum_bits(vecs["tie_down"]) == 0x3f800000 and X.exact_sum_bits(vecs["tie_up"]) == 0x3f800002
    assert X.exact_sum_bits(vecs["tie_down_plus"]) == 0x3f800001 and X.exact_sum_bits(vecs["tie_up_minus"]) == 0x3f800001
    assert X.exact_sum_bits(vecs["cancel"]) == int(X.bits_of(_p(-100))[0]) and seq["cancel"] == int(X.bits_of(_p(-100))[0])
    assert X.exact_sum_bits(vecs["cancel_sub"]) == 1 and seq["cancel_sub"] == 0
    assert X.exact_sum_bits(vecs["sub_sum"]) == 5 and X.exact_sum_bits(vecs["sub_from_normals"]) == 1
    assert X.exact_sum_bits(vecs["sub_to_normal"]) == 0x00800000
    assert X.exact_sum_bits(vecs["both_inf"]) == 0x7fc00000 and X.exact_sum_bits(vecs["pos_inf"]) == 0x7f800000


def test_round_fraction_bits_is_round_to_nearest_even():
    """the model's own rounding against numpy's float64 -> float32 conversion (RNE) on values float64 holds exactly"""
    rng = np.random.default_rng(9)
    xs = np.concatenate([rng.standard_normal(300) * 10.0 ** rng.integers(-44, 38, 300), [0.0, 2.0 ** -150, 3 * 2.0 ** -150, 2.0 ** -149,
                         (2 - 2.0 ** -24) * 2.0 ** 127, (2 - 2.0 ** -25) * 2.0 ** 127, -(2 - 2.0 ** -24) * 2.0 ** 127, 1 + 2.0 ** -24,
                         1 + 3 * 2.0 ** -24]])
    with np.errstate(over="ignore", under="ignore"):
        want = xs.astype(np.float32).view(np.uint32)
    for x, w in zip(xs, want):
        if x == 0:
            continue
        assert X.round_fraction_bits(Fraction(float(x))) == int(w), (x, hex(int(w)))


@pytest.fixture(scope="module")
def case_a():
    c = C.case_a()
    c["contrib"] = X.contributions(c["shapes"], c["loc"], c["attn"], c["gout"])
    return c


def test_model_is_permutation_invariant_and_sequential_fp32_is_not(case_a):
    c = case_a
    N, S, M = c["value"].shape[:3]
    dest, contrib = c["contrib"]
    exact, counts = X.exact_grad_value(N, S, M, dest, contrib)
    assert (counts == 0).any() and counts.max() > 64, "the case is to have empty rows and long ones"
    perm = np.random.default_rng(1).permutation(c["loc"].shape[1])
    dest_p, contrib_p = X.contributions(c["shapes"], c["loc"][:, perm], c["attn"][:, perm], c["gout"][:, perm])
    exact_p = X.exact_grad_value(N, S, M, dest_p, contrib_p)[0]
    assert np.array_equal(exact.view(np.uint32), exact_p.view(np.uint32))
    seq = X.sequential_grad_value(N, S, M, dest, contrib)
    seq_p = X.sequential_grad_value(N, S, M, dest_p, contrib_p)
    differ = int((seq.view(np.uint32) != seq_p.view(np.uint32)).sum())
    print("sequential fp32 sums differ in %d of %d elements after a permutation of the queries; the exact sum in 0" % (differ, seq.size))
    assert differ > seq.size // 4


def test_model_meets_the_ref64_bound_with_one_rounding_for_the_sum(case_a):
    c = case_a
    ref = R.msda(c["value"], c["shapes"], c["loc"], c["attn"], c["gout"])["grad_value"]
    got = X.exact_grad_value(*c["value"].shape[:3], *c["contrib"])[0]
    worst = R.check("exact model", "grad_value", got, X.bounded_exact(ref))
    print("exact model: worst err / bound (n = DEPTH + 1) %.3f" % worst)
    # ... and the bound means something: msda_ref64's own n (contributions + DEPTH) is far wider on the long rows
    assert float(np.max(ref.n)) > 10 * (R.DEPTH + 1)


def test_case_d_exceeds_the_split_length():
    d = C.case_d()
    dest, _ = X.contributions(d["shapes"], d["loc"], d["attn"], d["gout"])
    assert len(dest) == 8192 and len(set(dest.tolist())) == 1 and len(dest) > C.split_len()


def test_case_e_contributions_are_grad_out_exactly():
    e = C.case_e()
    dest, contrib = X.contributions(e["shapes"], e["loc"], e["attn"], e["gout"])
    nz = np.abs(contrib).max(1) > 0
    N, Lq, M, _, P, _ = e["loc"].shape
    assert int(nz.sum()) == N * Lq * M * P                      # one non-zero contribution per sample: its pixel
    g = np.repeat(e["gout"].reshape(N * Lq * M, 1, C.D), P, 1).reshape(-1, C.D)
    assert np.array_equal(contrib[nz].view(np.uint32), g.view(np.uint32))
    pix = e["pix"].reshape(N, Lq, M, P, 2)
    n_i, _, m_i, _ = np.meshgrid(np.arange(N), np.arange(Lq), np.arange(M), np.arange(P), indexing="ij")
    want = (n_i * 16 + pix[..., 1] * 4 + pix[..., 0]) * M + m_i
    assert np.array_equal(dest[nz], want.reshape(-1))


# ---- ABI ------------------------------------------------------------------------------------------------------------------------

def _exact_call(lib, D=32, L=4, P=4, Lq=120, work=1 << 40, work_ptr=4096, N=2, S=65, M=2):
    p = ctypes.c_void_p(4096)                    # never dereferenced: every refusal is decided on the host before any launch
    return lib.semidetr_msda_backward_exact_f32(None, p, p, p, p, p, p, N, S, M, D, L, Lq, P, 0, ctypes.c_void_p(work_ptr), work, p, p, p)


def test_exact_abi_is_declared_exported_and_refuses_on_the_host():
    import semi_detr_amd
    from test_cabi_mirror import declarations
    names = declarations()
    assert "semidetr_msda_exact_workspace_bytes" in names and "semidetr_msda_backward_exact_f32" in names
    assert "semidetr_msda_backward_exact_f32" in semi_detr_amd._lib.SIGNATURES
    lib = semi_detr_amd._lib.lib()
    assert lib.semidetr_abi_version() == 7
    size = lib.semidetr_msda_exact_workspace_bytes
    need = size(2, 65, 2, 4, 120, 4)
    entries = 2 * 2 * 120 * 4 * 4 * 4 * 8                       # 8 bytes x N M Lq L P 4
    assert entries <= need <= entries + 2 * (2 * 2 * 65 * 4 + 256)
    assert size(0, 65, 2, 4, 120, 4) == 0 and size(1, 1, 1, 4, 1 << 26, 4) == 0 and size(1, 1, 1, 4, (1 << 26) - 1, 4) > 0

    def refused(rc, text):
        err = lib.semidetr_last_error().decode()
        assert rc == -1 and text in err, (rc, err)
    refused(_exact_call(lib, D=16), "channels must be 32")
    refused(_exact_call(lib, D=64), "channels must be 32")
    refused(_exact_call(lib, L=8, P=8), "does not fit the gather kernel's LDS")
    refused(_exact_call(lib, L=9, P=7), "does not fit the gather kernel's LDS")
    refused(_exact_call(lib, work=need - 1), "workspace too small")
    refused(_exact_call(lib, work=0), "workspace too small")
    refused(_exact_call(lib, work_ptr=4100), "workspace must be 16-byte aligned")
    refused(_exact_call(lib, N=1, S=1, M=1, Lq=1 << 26, L=4, P=4), "below 2^32")
    rc = lib.semidetr_msda_backward_exact_f32(None, None, None, None, None, None, None, 1, 1, 1, 32, 1, 1, 1, 0, None, 0, None, None, None)
    assert rc == -1 and "null pointer" in lib.semidetr_last_error().decode()


def test_module_attribute_and_converter_need_no_gpu():
    import copy
    import pickle

    import torch

    import semi_detr_amd as s
    m = s.MSDeformAttn(64, 2, 2, 2)
    assert m.exact_backward is False and "exact_backward" not in m.state_dict()
    net = torch.nn.Sequential(m, torch.nn.Linear(2, 2), s.MSDeformAttn(64, 2, 2, 2))
    assert s.convert_exact_backward(net, "auto") == 2 and net[0].exact_backward == "auto" and net[2].exact_backward == "auto"
    assert s.convert_exact_backward(net, True) == 2 and copy.deepcopy(net)[0].exact_backward is True
    assert s.convert_exact_backward(net, False) == 2 and net[2].exact_backward is False
    with pytest.raises(ValueError):
        s.convert_exact_backward(net, "yes")
    old = pickle.loads(pickle.dumps(m))
    del old.__dict__["exact_backward"]                          # a module pickled before the attribute existed
    assert pickle.loads(pickle.dumps(old)).exact_backward is False
    assert s.MSDeformAttnExactFunction.apply is not None
