"""CPU: the float64 statement of the evaluation-time decode (tests/det_ref64.py) against the fixture the reference's own
functions produced (tests/golden/detect.npz, tools/gen_detect_golden.py), its fp32 bounds against the reference's float32 run,
mutants, the torch restatement that the probe uses as its baseline, and the C-ABI surface."""
import functools

import numpy as np
import pytest

import det_ref64 as R
from conftest import Golden

G = Golden("detect.npz")
NAMES = G.names()
PLAIN = [n for n in NAMES if not int(G[n]["tie"])]
TIES = [n for n in NAMES if int(G[n]["tie"])]


@functools.lru_cache(maxsize=None)
def case(name):
    """The fixture's case with its inputs regenerated from the seed (and checked against what the fixture holds of them)."""
    c = dict(G[name])
    L, B, Q, C, k = (int(v) for v in c["dims"])
    cls, box = R.seeded_inputs(int(c["seed"]), str(c["kind"]), L, B, Q, C, k)
    assert R.checksum(cls, box) == int(c["checksum"]), f"{name}: the seeded inputs are not the generator's"
    if "cls" in c:
        assert cls.tobytes() == c["cls"].tobytes() and box.tobytes() == c["box"].tobytes()
    c.update(cls=cls, box=box, L=L, B=B, Q=Q, C=C, k=k, rescale=bool(c["rescale"]),
             img_hw=c["img_shape"][:, :2].astype(np.float64), scale=c["scale_factor"] if int(c["rescale"]) else None,
             metas=[dict(img_shape=tuple(int(v) for v in c["img_shape"][b]), scale_factor=c["scale_factor"][b]) for b in range(B)])
    return c


@functools.lru_cache(maxsize=None)
def statement(name, mutant=None):
    c = case(name)
    return R.statement(c["cls"], c["box"], c["img_hw"], c["scale"], c["k"], mutant)


def diff(a, b):
    """|a - b| with equal infinities and NaN against NaN counting as 0."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    with np.errstate(invalid="ignore"):
        return np.where((a == b) | (np.isnan(a) & np.isnan(b)), 0.0, np.abs(a - b))


def test_cases_cover_what_the_issue_lists():
    dims = {n: tuple(int(v) for v in G[n]["dims"][2:]) for n in NAMES}
    assert {(5, 3, 15), (5, 3, 1), (37, 20, 100), (900, 80, 300), (900, 80, 900)} <= {dims[n] for n in PLAIN}
    c = case("full_k300")
    assert c["B"] == 2 and c["rescale"] and len({tuple(r) for r in c["img_shape"]}) == 2
    assert (c["scale_factor"][:, 0] != c["scale_factor"][:, 1]).all() and (c["scale_factor"][0] != c["scale_factor"][1]).any()
    assert {bool(case(n)["rescale"]) for n in PLAIN} == {True, False}
    assert {str(G[n]["kind"]) for n in TIES} == set(R.TIE_KINDS)
    for n in ("q37", "full_k300", "full_k900"):                 # the clamp is active on both sides, and zero-size boxes are selected
        c, s = case(n), statement(n)
        raw = R.decode(c["cls"][-1], c["box"][-1], s["idx"], c["img_hw"], None)["dets"][..., :4]
        picked = c["box"][-1].astype(np.float64)[np.arange(c["B"])[:, None], s["idx"] // c["C"]]
        assert (picked[..., :2] - 0.5 * picked[..., 2:] < 0).any() and (picked[..., :2] + 0.5 * picked[..., 2:] > 1).any()
        assert (raw[..., :2] == 0).any() and (raw[..., 2:] == np.asarray(c["img_hw"])[:, None, ::-1]).any()
        assert ((raw[..., 2] == raw[..., 0]) & (raw[..., 2] > 0)).any() or ((raw[..., 3] == raw[..., 1]) & (raw[..., 3] > 0)).any()
    c = case("tie_dup_chunks")                                  # equal logits on both sides of the kernel's chunk boundaries
    flat = c["cls"][-1].reshape(-1)
    assert (flat[[8191, 8192, 8193, 16383, 16384]] == flat[0]).all() and (flat == flat[0]).sum() > c["k"]
    c = case("tie_saturated")
    assert (c["cls"][-1] > 17).all() and len(np.unique(c["cls"][-1])) == c["cls"][-1].size and (c["dets32"][..., 4] == 1).all()
    c = case("tie_inf_nan")
    assert np.isnan(c["cls"][-1]).sum() == 1 and np.isposinf(c["cls"][-1]).any() and np.isneginf(c["cls"][-1]).any()
    c = case("tie_zeros")
    z = c["cls"][-1][c["cls"][-1] == 0]
    assert np.signbit(z).any() and (~np.signbit(z)).any() and len(z) > c["k"]


@pytest.mark.parametrize("name", PLAIN)
def test_statement_reproduces_the_reference_exactly_in_decisions_and_within_bounds_in_values(name):
    c, s = case(name), statement(name)
    # decisions of the float32 run: every index, label, grouped position and offset -- no element is left out
    assert np.array_equal(s["idx"], c["idx32"]) and np.array_equal(s["labels"], c["labels32"])
    assert np.array_equal(s["offsets"], c["offsets32"])
    n = np.arange(c["B"])[:, None]
    assert np.array_equal(c["dets32"][n, s["order"]], c["grouped32"])
    # values: the float64 run is the statement, the float32 run lies within the derived bounds
    assert diff(s["dets"], c["dets64"]).max() <= 1e-9 * max(1.0, np.abs(c["dets64"]).max())
    err = diff(c["dets32"], s["dets"])
    assert (err <= s["bound"]).all(), float((err / s["bound"]).max())


@pytest.mark.parametrize("name", TIES)
def test_tie_cases_are_admissible_results_of_the_reference(name):
    c, s = case(name), statement(name)
    import torch
    ref = c["dets32"][..., 4]
    # the reference's own fp32 scores of ALL Q * C candidates: the same op on the same (Q, C) tensor as its cls_score.sigmoid()
    table = np.stack([torch.from_numpy(c["cls"][-1][b]).sigmoid().view(-1).numpy() for b in range(c["B"])])
    for b in range(c["B"]):
        mine = table[b][s["idx"][b]]
        # the sorted score multiset equals the reference's (NaN == NaN)
        assert np.array_equal(np.sort(mine), np.sort(ref[b]), equal_nan=True)
        # each selected index is admissible: its score reaches the reference's k-th
        assert (np.isnan(mine) | (mine >= np.nanmin(ref[b]))).all()
        assert len(set(s["idx"][b].tolist())) == c["k"]
        # and the reference's own choice is admissible under the same rule (the rule is not vacuous)
        assert np.array_equal(np.sort(table[b][c["idx32"][b]]), np.sort(ref[b]), equal_nan=True)


def _disagrees(mutant):
    for name in NAMES:
        c, s, good = case(name), statement(name, mutant), statement(name)
        if int(c["tie"]):
            if mutant == "ties_high" and not np.array_equal(s["idx"], good["idx"]):
                return True
            continue
        n = np.arange(c["B"])[:, None]
        if not (np.array_equal(s["idx"], c["idx32"]) and np.array_equal(s["labels"], c["labels32"])):
            return True
        if not (diff(c["dets32"], s["dets"]) <= s["bound"]).all():
            return True
        if not (np.array_equal(s["offsets"], c["offsets32"]) and np.array_equal(c["dets32"][n, s["order"]], c["grouped32"])):
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
    import detect_torch_restated as T
    for name in PLAIN:
        c = case(name)
        cls, box = torch.from_numpy(c["cls"]), torch.from_numpy(c["box"])
        got = T.get_bboxes(cls, box, c["metas"], c["rescale"], c["k"])
        assert np.stack([g[0].numpy() for g in got]).tobytes() == c["dets32"].tobytes()
        assert np.array_equal(np.stack([g[1].numpy() for g in got]), c["labels32"])
        res = T.detection_results(cls, box, c["metas"], c["C"], c["rescale"], c["k"])
        for b in range(c["B"]):
            want = R.split(c["grouped32"][b], c["offsets32"][b], c["C"])
            assert len(res[b]) == c["C"] and all(a.tobytes() == w.tobytes() for a, w in zip(res[b], want))


def test_cabi_surface_and_argument_errors():
    import semi_detr_amd
    assert {"semidetr_det_workspace_bytes", "semidetr_det_decode_f32"} <= set(semi_detr_amd._lib.SIGNATURES)
    lib = semi_detr_amd._lib.lib()
    assert lib.semidetr_abi_version() == 7
    assert lib.semidetr_det_workspace_bytes(2, 900, 80, 300) == 2 * 9 * 300 * 8
    assert lib.semidetr_det_workspace_bytes(1, 5, 3, 16) == 0 and lib.semidetr_det_workspace_bytes(1, 900, 80, 2049) == 0
    one = 16                                            # non-null, never dereferenced: the checks below fail on the host
    args = lambda k, ws=1 << 20, by=one, off=one: (None, one, one, one, None, 1, 900, 80, k, one, ws, one, one, by, off)  # noqa: E731
    assert lib.semidetr_det_decode_f32(None, None, one, one, None, 1, 900, 80, 300, one, 1 << 20, one, one, None, None) == -1
    assert b"null pointer" in lib.semidetr_last_error()
    assert lib.semidetr_det_decode_f32(*args(0)) == -1 and b"bad sizes" in lib.semidetr_last_error()
    assert lib.semidetr_det_decode_f32(None, one, one, one, None, 1, 5, 3, 16, one, 1 << 20, one, one, None, None) == -1
    assert lib.semidetr_det_decode_f32(*args(2049)) == -2 and b"too large" in lib.semidetr_last_error()      # SEMIDETR_E_TOOLARGE
    assert lib.semidetr_det_decode_f32(None, one, one, one, None, 1, 1 << 16, 1 << 15, 5, one, 1 << 20, one, one, None, None) == -2
    assert lib.semidetr_det_decode_f32(*args(300, ws=8)) == -1 and b"workspace" in lib.semidetr_last_error()
    assert lib.semidetr_det_decode_f32(*args(300, off=None)) == -1 and b"together" in lib.semidetr_last_error()
    import torch
    import semi_detr_amd as s
    assert s.get_bboxes is s.detect.get_bboxes and s.detection_results is s.detect.detection_results
    metas = [dict(img_shape=(48, 64, 3), scale_factor=np.ones(4, np.float32))]
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        s.get_bboxes(torch.zeros(2, 1, 5, 3), torch.zeros(2, 1, 5, 4), metas)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        s.detection_results(torch.zeros(2, 1, 5, 3), torch.zeros(2, 1, 5, 4), metas, 3)
