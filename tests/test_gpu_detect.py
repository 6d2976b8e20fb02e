"""The evaluation-time decode on the MI355X (csrc/detect.hip) against the float64 statement with its fp32 bounds
(tests/det_ref64.py) on every case of the reference's fixture (tests/golden/detect.npz), through the public Python functions
and through the C ABI."""
import ctypes

import numpy as np
import pytest
import torch

import det_ref64 as R
from test_detect_ref import NAMES, case, diff, statement

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")


def _np(t):
    return t.detach().cpu().numpy()


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _report(what, err, bound):
    worst = float((err / bound).max(initial=0.0))
    print(f"[detect] {what}: worst err / bound = {worst:.3f}")
    assert (err <= bound).all(), (what, worst)


def run_abi(cls, box, img_hw, scale, k, grouped=True):
    """Straight through the C ABI on (B, Q, C) / (B, Q, 4) arrays; outputs pre-filled with a pattern (every element is written)."""
    import semi_detr_amd
    lib = semi_detr_amd._lib.lib()
    P = ctypes.c_void_p
    B, Q, C = cls.shape
    nbytes = lib.semidetr_det_workspace_bytes(B, Q, C, k)
    assert nbytes > 0
    ws = torch.full((nbytes // 8,), -1, dtype=torch.int64, device=DEV)        # not zero: the kernels must not rely on a memset
    lg, bx, hw = _dev(cls), _dev(box), _dev(np.asarray(img_hw, np.float32))
    sf = None if scale is None else _dev(np.asarray(scale, np.float32))
    dets = torch.full((B, k, 5), -7.0, device=DEV)
    labels = torch.full((B, k), -7, dtype=torch.int64, device=DEV)
    by_class = torch.full((B, k, 5), -7.0, device=DEV)
    offsets = torch.full((B, C + 1), -7, dtype=torch.int32, device=DEV)
    rc = lib.semidetr_det_decode_f32(P(torch.cuda.current_stream().cuda_stream), P(lg.data_ptr()), P(bx.data_ptr()),
                                     P(hw.data_ptr()), None if sf is None else P(sf.data_ptr()), B, Q, C, k, P(ws.data_ptr()),
                                     nbytes, P(dets.data_ptr()), P(labels.data_ptr()),
                                     P(by_class.data_ptr()) if grouped else None, P(offsets.data_ptr()) if grouped else None)
    assert rc == 0, lib.semidetr_last_error()
    return _np(dets), _np(labels), _np(by_class), _np(offsets)


def check_against_statement(what, s, dets, labels, by_class, offsets, C):
    """Labels exact, values within the derived bounds, grouped rows bytewise the stable partition of the rows, offsets exact."""
    assert np.array_equal(labels, s["labels"])
    _report(what, diff(dets, s["dets"]), s["bound"])
    n = np.arange(dets.shape[0])[:, None]
    assert by_class.tobytes() == np.ascontiguousarray(dets[n, s["order"]]).tobytes()
    assert np.array_equal(offsets, s["offsets"]) and offsets.dtype == np.int32


@pytest.mark.parametrize("name", NAMES)
def test_fixture_cases_through_the_c_abi(name):
    c, s = case(name), statement(name)
    dets, labels, by_class, offsets = run_abi(c["cls"][-1], c["box"][-1], c["img_hw"], c["scale"], c["k"])
    check_against_statement(name, s, dets, labels, by_class, offsets, c["C"])
    # the flat indices themselves, exactly: a second decode over a box tensor that carries the query number (cx = q / 1024,
    # w = h = 0, W = 1024: x1 = q without a rounding) gives index = q * C + label
    B, Q, C, k = c["B"], c["Q"], c["C"], c["k"]
    tag = np.zeros((B, Q, 4), np.float32)
    tag[..., 0] = np.arange(Q, dtype=np.float32)[None] / 1024          # cx = q / 1024, w = h = 0, W = 1024: x1 = q exactly
    d2, l2, _, _ = run_abi(c["cls"][-1], tag, np.full((B, 2), 1024.0), None, k, grouped=False)
    idx = d2[..., 0].astype(np.int64) * C + l2
    assert np.array_equal(idx, s["idx"])
    if not int(c["tie"]):
        assert np.array_equal(idx, c["idx32"])                          # the reference's own choice and order


@pytest.mark.parametrize("name", NAMES)
def test_public_functions(name):
    import semi_detr_amd as sda
    c, s = case(name), statement(name)
    cls, box = _dev(c["cls"]), _dev(c["box"])
    runs = []
    for _ in range(2):
        torch.cuda.synchronize()
        torch.cuda.set_sync_debug_mode("error")
        try:
            out = sda.get_bboxes(cls, box, c["metas"], rescale=c["rescale"], max_per_img=c["k"])
        finally:
            torch.cuda.set_sync_debug_mode("default")
        assert len(out) == c["B"] and all(d.shape == (c["k"], 5) and l.shape == (c["k"],) and l.dtype == torch.int64 for d, l in out)
        runs.append((np.stack([_np(d) for d, _ in out]), np.stack([_np(l) for _, l in out])))
    assert runs[0][0].tobytes() == runs[1][0].tobytes() and runs[0][1].tobytes() == runs[1][1].tobytes()      # run to run
    dets, labels = runs[0]
    assert np.array_equal(labels, s["labels"])
    _report(f"{name} get_bboxes", diff(dets, s["dets"]), s["bound"])
    # detection_results == bbox2result applied to get_bboxes, for the head's class count, one less and one more
    for num_classes in (c["C"], c["C"] + 1, max(c["C"] - 1, 1)):
        res = sda.detection_results(cls, box, c["metas"], num_classes, rescale=c["rescale"], max_per_img=c["k"])
        pending = sda.detection_results(cls, box, c["metas"], num_classes, rescale=c["rescale"], max_per_img=c["k"], wait=False)
        later = pending.result()
        assert len(res) == c["B"]
        for b in range(c["B"]):
            want = [dets[b][labels[b] == i, :] for i in range(num_classes)]          # transforms.py:117
            assert len(res[b]) == num_classes
            for got, again, w in zip(res[b], later[b], want):
                assert got.dtype == np.float32 and got.shape == w.shape and got.tobytes() == w.tobytes() == again.tobytes()
    # a list of per-layer tensors, as the head returns when it unbinds; and the default k = Q
    out = sda.get_bboxes(list(cls), list(box), c["metas"], rescale=c["rescale"], max_per_img=c["k"])
    assert np.stack([_np(d) for d, _ in out]).tobytes() == dets.tobytes()
    if c["Q"] <= min(c["Q"] * c["C"], 2048):
        out = sda.get_bboxes(cls, box, c["metas"])
        assert all(d.shape == (c["Q"], 5) for d, _ in out)
        full = R.statement(c["cls"], c["box"], c["img_hw"], None, c["Q"])
        assert np.array_equal(np.stack([_np(l) for _, l in out]), full["labels"])


@pytest.mark.parametrize("B,Q,C,k", [(1, 900, 80, 2048), (2, 103, 80, 2048), (3, 8, 1025, 64), (1, 1, 1, 1), (2, 2048, 4, 8)])
def test_seeded_sizes_that_take_the_other_paths(B, Q, C, k):
    """k = 2048 at 72 000 candidates: the survivors do not fit LDS and the merge reads them from the workspace.  Q * C = 8240
    and 8200: a last chunk of 48 / 8 candidates, shorter than k.  One candidate.  Exactly one full chunk (8192).  Quantised
    logits, so that ties cross every boundary."""
    cls, box = R.seeded_inputs(7 + B + Q, "quantized", 1, B, Q, C, k)
    hw = np.asarray([(480 + 7 * b, 640 - 5 * b) for b in range(B)], np.float64)
    sf = np.asarray([(1.25 + b, 0.75, 1.25 + b, 0.75) for b in range(B)], np.float32)
    s = R.statement(cls, box, hw, sf, k)
    dets, labels, by_class, offsets = run_abi(cls[-1], box[-1], hw, sf, k)
    check_against_statement(f"B{B} Q{Q} C{C} k{k}", s, dets, labels, by_class, offsets, C)
    tag = np.zeros((B, Q, 4), np.float32)
    tag[..., 0] = np.arange(Q, dtype=np.float32)[None] / 4096
    d2, l2, _, _ = run_abi(cls[-1], tag, np.full((B, 2), 4096.0), None, k, grouped=False)
    assert np.array_equal(d2[..., 0].astype(np.int64) * C + l2, s["idx"])


def test_graph_capture_and_replay():
    import semi_detr_amd as sda
    c = case("full_k300")
    cls, box = _dev(c["cls"]), _dev(c["box"])
    hw = _dev(c["img_hw"].astype(np.float32))
    sf = _dev(c["scale_factor"])
    B, Q, C, k = c["B"], c["Q"], c["C"], c["k"]
    nbytes = int(sda._lib.lib().semidetr_det_workspace_bytes(B, Q, C, k))
    ws = torch.empty(nbytes // 8, dtype=torch.int64, device=DEV)
    outs = [torch.empty((B, k, 5), device=DEV), torch.empty((B, k), dtype=torch.int64, device=DEV),
            torch.empty((B, k, 5), device=DEV), torch.empty((B, C + 1), dtype=torch.int32, device=DEV)]

    def step():
        sda._lib.call("semidetr_det_decode_f32", DEV, cls[-1].contiguous(), box[-1].contiguous(), hw, sf, B, Q, C, k, ws, nbytes,
                      *outs)
    step()
    torch.cuda.synchronize()
    eager = [_np(t).copy() for t in outs]
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        step()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        step()
    for _ in range(2):
        for t in outs:
            t.fill_(-1)
        ws.fill_(-1)
        graph.replay()
        torch.cuda.synchronize()
        for a, b in zip(eager, outs):
            assert a.tobytes() == _np(b).tobytes()
    s = statement("full_k300")
    check_against_statement("graph replay", s, _np(outs[0]), _np(outs[1]), _np(outs[2]), _np(outs[3]), C)


def test_errors():
    import semi_detr_amd as sda
    metas = [dict(img_shape=(48, 64, 3), scale_factor=np.ones(4, np.float32))]
    cls, box = torch.zeros(2, 1, 5, 3, device=DEV), torch.zeros(2, 1, 5, 4, device=DEV)
    with pytest.raises(RuntimeError, match="selected index k out of range"):
        sda.get_bboxes(cls, box, metas, max_per_img=16)
    big = torch.zeros(1, 1, 700, 3, device=DEV)
    with pytest.raises(ValueError, match="1..2048"):
        sda.get_bboxes(big, torch.zeros(1, 1, 700, 4, device=DEV), metas, max_per_img=2049)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        sda.get_bboxes(cls.cpu(), box.cpu(), metas)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        sda.get_bboxes(cls, box.cpu(), metas)
    with pytest.raises(ValueError, match="expected cls_scores"):
        sda.get_bboxes(cls, torch.zeros(2, 1, 4, 4, device=DEV), metas)
    with pytest.raises(ValueError, match="expected cls_scores"):
        sda.get_bboxes(cls[:, 0], box, metas)
    with pytest.raises(ValueError, match="img_metas"):
        sda.get_bboxes(cls, box, metas * 2)
    with pytest.raises(ValueError, match="scale_factor"):
        sda.get_bboxes(cls, box, [dict(img_shape=(48, 64, 3), scale_factor=np.ones(2, np.float32))], rescale=True)
    lib = sda._lib.lib()
    P = ctypes.c_void_p
    ok = torch.zeros(64, device=DEV)
    rc = lib.semidetr_det_decode_f32(None, P(ok.data_ptr()), P(ok.data_ptr()), P(ok.data_ptr()), None, 1, 5, 3, 16,
                                     P(ok.data_ptr()), 256, P(ok.data_ptr()), P(ok.data_ptr()), None, None)
    assert rc == -1 and b"bad sizes" in lib.semidetr_last_error()
    rc = lib.semidetr_det_decode_f32(None, P(ok.data_ptr()), P(ok.data_ptr()), P(ok.data_ptr()), None, 1, 900, 80, 2049,
                                     P(ok.data_ptr()), 256, P(ok.data_ptr()), P(ok.data_ptr()), None, None)
    assert rc == -2 and b"too large" in lib.semidetr_last_error()
