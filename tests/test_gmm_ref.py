"""CPU checks of the cost-GMM double filter's contract: the fp64 restatement (tests/gmm_ref64.py) against the reference's own
fixtures (tests/golden/gmm.npz, tools/gen_gmm_golden.py) and live scikit-learn, the set logic of the filter, the segment
buffer over gloo, and the host-side argument checks of the new C-ABI entry points."""
import os
import socket
import warnings

import numpy as np
import pytest
import torch

from conftest import GOLDEN
from gmm_ref64 import double_filter_sets, fit_gmm_ref64

Z = np.load(os.path.join(GOLDEN, "gmm.npz"))
FIT_NAMES = [str(n) for n in Z["fit_names"]]


def _case(name):
    return {k.split(".", 2)[2]: Z[k] for k in Z.files if k.startswith(f"fit.{name}.")}


@pytest.mark.parametrize("name", FIT_NAMES)
def test_ref64_reproduces_reference_fixture(name):
    c = _case(name)
    r = fit_gmm_ref64(c["costs"], max_iter=int(c["max_iter"]))
    assert np.float32(r["thr"]).tobytes() == np.float32(c["thr"]).tobytes(), (r["thr"], c["thr"])
    if "labels" in c:
        np.testing.assert_array_equal(r["labels"], c["labels"])
        assert r["n_iter"] == int(c["n_iter"]) and r["converged"] == bool(c["converged"])
        np.testing.assert_allclose(r["scores"], c["scores"], rtol=1e-12, atol=0)


def test_fixture_covers_the_required_cases():
    assert str(Z["sklearn_version"]) == "1.7.2"
    assert _case("n0")["costs"].size == 0 and _case("n1")["costs"].size == 1
    assert not (_case("empty_comp0")["labels"] == 0).any()                   # the fallback branch
    assert not bool(_case("maxiter2")["converged"]) and int(_case("maxiter2")["n_iter"]) == 2
    assert _case("n2400")["costs"].size == 2400


def _random_costs(rng, t):
    n = int(rng.integers(2, 400))
    k = t % 4
    if k == 0:
        c = np.concatenate([rng.normal(1, 0.3, n), rng.normal(4, 1, n // 3)])
    elif k == 1:
        c = rng.gamma(1.5, 1.0, n) * 3
    elif k == 2:
        c = rng.normal(5, 0.5, n)
    else:
        c = rng.uniform(0, 10, n)
    return c.astype(np.float32)


def test_ref64_agrees_with_live_sklearn():
    skm = pytest.importorskip("sklearn.mixture")
    rng = np.random.default_rng(11)
    checked = 0
    for t in range(520):
        c = _random_costs(rng, t)
        x = np.sort(c).reshape(-1, 1)
        g = skm.GaussianMixture(2, weights_init=np.array([0.5, 0.5]), means_init=np.array([x.min(), x.max()]).reshape(2, 1),
                                precisions_init=np.array([1.0, 1.0]).reshape(2, 1), covariance_type="diag", reg_covar=1e-5)
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            g.fit(x)
        lab, sc = g.predict(x), g.score_samples(x)
        r = fit_gmm_ref64(c)
        if r["margin"] < 1e-12:
            continue
        np.testing.assert_array_equal(r["labels"], lab)
        assert r["n_iter"] == g.n_iter_ and r["converged"] == g.converged_
        np.testing.assert_allclose(r["scores"], sc, rtol=1e-11, atol=0)
        m = lab == 0 if (lab == 0).any() else lab == 1
        assert r["thr"] == x[m, 0][int(np.argmax(sc[m]))]
        checked += 1
    assert checked >= 500


def _split(flat, counts):
    out, o = [], 0
    for c in counts:
        out.append(flat[o:o + c])
        o += c
    return out


def test_set_logic_matches_end_to_end_fixture():
    counts = Z["e2e.counts"]
    gt_b, gt_l, gt_s = (_split(Z[f"e2e.{k}"], counts) for k in ("gt_bboxes", "gt_labels", "gt_scores"))
    det_b, det_l, det_s = (_split(Z[f"e2e.{k}"], counts) for k in ("det_bboxes", "det_labels", "det_scores"))
    mc, mi = _split(Z["e2e.match_cost"], Z["e2e.match_counts"]), _split(Z["e2e.match_inds"], Z["e2e.match_counts"])
    thr = Z["e2e.thr"][0]
    assert thr.tobytes() == fit_gmm_ref64(Z["e2e.match_cost"])["thr"].tobytes()
    got = {k: [] for k in ("gt_bboxes_list", "gt_labels_list", "gt_scores_list", "unsup_bboxes_gmm_list",
                           "unsup_labels_gmm_list", "unsup_scores_gmm_list", "det_bboxes_gmm_list", "det_labels_gmm_list",
                           "det_scores_gmm_list")}
    for b in range(len(counts)):
        base, union = double_filter_sets(mc[b], mi[b], gt_s[b], thr)
        for k, src, idx in (("gt_bboxes_list", gt_b, base), ("gt_labels_list", gt_l, base), ("gt_scores_list", gt_s, base),
                            ("unsup_bboxes_gmm_list", gt_b, union), ("unsup_labels_gmm_list", gt_l, union),
                            ("unsup_scores_gmm_list", gt_s, union), ("det_bboxes_gmm_list", det_b, union),
                            ("det_labels_gmm_list", det_l, union), ("det_scores_gmm_list", det_s, union)):
            got[k].append(src[b][idx])
    for k, lists in got.items():
        np.testing.assert_array_equal([len(v) for v in lists], Z[f"e2e.{k}.counts"])
        flat = np.concatenate(lists)
        assert flat.tobytes() == Z[f"e2e.{k}"].tobytes(), k


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _gloo_worker(rank, world, port, capacity, q):
    import torch.distributed as dist
    import semi_detr_amd.gmm_filter as gf
    dist.init_process_group("gloo", init_method=f"tcp://127.0.0.1:{port}", rank=rank, world_size=world)
    try:
        n = [3, 0, 7][rank]                           # uneven counts, one rank without pairs
        costs = torch.arange(n, dtype=torch.float32) + 10.0 * rank + 0.5
        gathered = gf.gather_segments(gf.pack_segment(costs, capacity))
        q.put((rank, gf.segment_counts(gathered).tolist(), gf.segment_costs(gathered).tolist()))
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("world", [2, 3])
def test_segment_buffer_round_trips_over_gloo(world):
    import multiprocessing as mp
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_gloo_worker, args=(r, world, port, 8, q)) for r in range(world)]
    for p in procs:
        p.start()
    res = [q.get(timeout=120) for _ in range(world)]
    for p in procs:
        p.join(60)
        assert p.exitcode == 0
    want_counts = [3, 0, 7][:world]
    want = [10.0 * r + 0.5 + i for r in range(world) for i in range(want_counts[r])]
    for _, counts, costs in res:
        assert counts == want_counts and costs == want


def test_pack_segment_rejects_overflow():
    import semi_detr_amd.gmm_filter as gf
    with pytest.raises(ValueError, match="capacity"):
        gf.pack_segment(torch.ones(5), 4)


def test_gmm_abi_rejects_bad_arguments_without_gpu():
    import semi_detr_amd
    lib = semi_detr_amd._lib.lib()
    err = lambda: lib.semidetr_last_error().decode()  # noqa: E731
    # unsupported covariance type (only SEMIDETR_GMM_COVARIANCE_DIAG = 1)
    assert lib.semidetr_gmm_fit_f64(None, None, 0, None, 1, 1, 0, 2, 1e-5, 1e-3, 100, None, None, None, None) == -1
    assert "'diag'" in err()
    assert lib.semidetr_gmm_fit_f64(None, None, 0, None, 1, 0, 0, 1, 1e-5, 1e-3, 100, None, None, None, None) == -1
    assert lib.semidetr_gmm_fit_f64(None, None, 4, None, 1, 1, 8, 1, 1e-5, 1e-3, 100, None, None, None, None) == -1
    assert "stride" in err()
    assert lib.semidetr_gmm_fit_f64(None, None, 8, None, 1, 1, 8, 1, 1e-5, 1e-3, 0, None, None, None, None) == -1
    assert lib.semidetr_gmm_fit_f64(None, None, 8, None, 1, 1, 8, 1, 1e-5, 1e-3, 100, None, None, None, None) == -1
    assert "null pointer" in err()
    # more pairs than the segment holds; null outputs
    assert lib.semidetr_gmm_match_costs_f32(None, None, None, None, None, None, 2, 10, 9, 8, None, None) == -1
    assert "capacity" in err()
    assert lib.semidetr_gmm_match_costs_f32(None, None, None, None, None, None, 2, 10, 4, 8, None, None) == -1
    assert "null pointer" in err()
    # more gts in an image than its output slot; null pointers
    args = [None] * 11
    assert lib.semidetr_gmm_double_filter_f32(None, *args, 2, 301, 0.4, 300, *([None] * 10)) == -1
    assert "slot" in err()
    assert lib.semidetr_gmm_double_filter_f32(None, *args, 2, 10, 0.4, 300, *([None] * 10)) == -1
    assert "null pointer" in err()
    assert lib.semidetr_abi_version() == 7


def test_python_api_rejects_other_covariance_types():
    import semi_detr_amd
    for cov in ("full", "tied", "spherical"):
        with pytest.raises(NotImplementedError, match="'diag'"):
            semi_detr_amd.fit_gmm_threshold(torch.zeros(3), covariance_type=cov)
