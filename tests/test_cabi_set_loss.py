"""CPU: the set-loss entry points (semidetr_set_loss_*) reject bad segment tables, sizes and null pointers with
SEMIDETR_E_BADARG before touching a device, and the Python front end refuses CPU tensors (no CPU fallback)."""
import ctypes

import pytest
import torch

BADARG = -1


def _good():
    from semi_detr_amd import set_loss as sl
    s = sl._Segment()
    s.kind, s.num_layers, s.num_images, s.num_query, s.num_classes = sl.MATCHED, 2, 2, 8, 80
    s.logits, s.labels = 4096, 8192              # never dereferenced: every call below fails its host-side checks
    s.logit_stride[:] = [2 * 8 * 80, 8 * 80, 80]
    s.gamma, s.alpha, s.iou_eps = 2.0, 0.25, 1e-6
    return s


def _table(*segs):
    from semi_detr_amd import set_loss as sl
    arr = (sl._Segment * len(segs))()
    for i, s in enumerate(segs):
        arr[i] = s
    return arr


def _fwd(tab, n, ws=1, nbytes=1 << 20, stats=1, norms=1):
    from semi_detr_amd import _lib
    P = ctypes.c_void_p
    return _lib.lib().semidetr_set_loss_forward_f32(None, tab, n, P(ws), nbytes, P(stats), P(norms), None, None)


def test_workspace_bytes_of_a_good_table():
    from semi_detr_amd import _lib
    n = _lib.lib().semidetr_set_loss_workspace_bytes(_table(_good()), 1)
    assert n == 2 * 1 * 10 * 8                    # 2 layers x one 64-row chunk x 10 fp64 statistics


@pytest.mark.parametrize("field,value", [("kind", 7), ("num_layers", 0), ("num_images", -1), ("num_query", 0),
                                         ("num_classes", 0), ("logits", None), ("labels", None), ("gamma", -1.0),
                                         ("iou_eps", 0.0)])
def test_bad_segment_fields_are_rejected(field, value):
    from semi_detr_amd import _lib
    s = _good()
    setattr(s, field, value)
    assert _fwd(_table(s), 1) == BADARG
    assert _lib.lib().semidetr_set_loss_workspace_bytes(_table(s), 1) == BADARG
    assert b"set_loss" in _lib.lib().semidetr_last_error()


def test_bad_tables_sizes_and_pointers_are_rejected():
    from semi_detr_amd import _lib
    from semi_detr_amd import set_loss as sl
    lib = _lib.lib()
    g = _good()
    assert _fwd(None, 1) == BADARG
    assert _fwd(_table(g), 0) == BADARG
    assert _fwd(_table(g, g, g, g), 4) == BADARG                       # at most three segments
    many = _good()
    many.num_layers = 65
    many.logit_stride[0] = 2 * 8 * 80
    assert _fwd(_table(many), 1) == BADARG                             # at most 64 (segment, layer) pairs
    ov = _good()
    ov.logit_stride[2] = 40                                            # rows overlap the class dimension
    assert _fwd(_table(ov), 1) == BADARG
    assert _fwd(_table(g), 1, ws=0) == BADARG
    assert _fwd(_table(g), 1, nbytes=8) == BADARG                      # smaller than the workspace query
    assert _fwd(_table(g), 1, stats=0) == BADARG
    boxes = _good()
    boxes.boxes = 4096
    boxes.box_stride[:] = [64, 32, 4]
    assert _fwd(_table(boxes), 1) == BADARG                            # boxes without targets / img_wh
    dn = _good()
    dn.kind, dn.boxes, dn.img_wh = sl.DN, 4096, 4096
    dn.box_stride[:] = [64, 32, 4]
    dn.gt_offsets, dn.gt_boxes, dn.gt_labels, dn.single_pad, dn.dn_groups = 4096, 4096, 4096, 3, 2
    assert _fwd(_table(dn), 1) == BADARG                               # Q = 8 != single_pad * groups = 6
    wu = _good()
    wu.kind = sl.WARMUP
    assert _fwd(_table(wu), 1) == BADARG                               # warm-up needs the alignment metrics
    P = ctypes.c_void_p
    assert lib.semidetr_set_loss_finalize_f32(None, _table(g), 1, P(1), P(1), None, P(1), P(1)) == BADARG
    assert lib.semidetr_set_loss_backward_f32(None, _table(g), 1, None, None) == BADARG
    mis = _good()
    mis.grad_logits = 4100                                             # gradients are written as float4
    assert lib.semidetr_set_loss_backward_f32(None, _table(mis), 1, None, P(1)) == BADARG


def test_cpu_tensors_have_no_fallback():
    import semi_detr_amd as s
    x = torch.randn(5, 80, requires_grad=True)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        s.FocalLoss(loss_weight=2.0)(x, torch.full((5,), 80, dtype=torch.long), avg_factor=3.0)
    seg = s.SetLossSegment(0, x.detach()[None, None], labels=torch.zeros(1, 5, dtype=torch.long))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        s.set_losses([seg])


def test_focal_loss_reduction_contract():
    import semi_detr_amd as s
    with pytest.raises(NotImplementedError):
        s.FocalLoss(reduction="none")(torch.randn(2, 3), torch.zeros(2, dtype=torch.long))
    with pytest.raises(AssertionError):
        s.FocalLoss(use_sigmoid=False)


def test_register_losses_without_mmdet():
    from semi_detr_amd import registry
    done, skipped = registry.register_losses()
    assert done + skipped == ["FocalLoss"]
