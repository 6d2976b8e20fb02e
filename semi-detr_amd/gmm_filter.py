"""Cost-GMM double filter of the unsupervised loss on the MI355X (``csrc/gmm_filter.hip``).

* ``fit_gmm_threshold`` replaces ``DinoDetrSSOD._fit_gmm`` (detr_ssod/models/dino_detr_ssod.py:832-890): a two-component,
  one-feature ``sklearn.mixture.GaussianMixture`` (covariance_type 'diag', weights_init [.5, .5], means_init [min, max],
  precisions_init [[1], [1]], reg_covar 1e-5) fitted in fp64 in one workgroup, then predict / score_samples and the
  threshold pick -- a 1-element device tensor, no host round trip.  ``fit_gmm`` is the same as a method
  (``DinoDetrSSOD._fit_gmm = semi_detr_amd.fit_gmm``).
* ``unsup_gmm_filter`` replaces the top of ``DinoDetrSSOD.unsup_loss`` (:243-353): cost matrix + LSAP of every image, the
  matched costs gathered over the ranks, the GMM threshold, and the double filter that gives the nine pseudo-label lists.
  One pinned read-back of the list lengths per call (``wait=False`` defers it to ``result()``).

Ties in the threshold pick go to the smaller cost (the reference sorts ascending and takes ``topk``'s first maximum).
"""
import collections

import torch

from . import _lib
from .matcher import lsap_batch, match_cost_batch

COVARIANCE_DIAG = _lib.CONSTANTS["SEMIDETR_GMM_COVARIANCE_DIAG"]


def _check_covariance(covariance_type):
    if covariance_type != "diag":
        raise NotImplementedError(f"covariance_type={covariance_type!r}: only 'diag' is implemented (the covariance type "
                                  "DinoDetrSSOD fixes, dino_detr_ssod.py:87)")


def _fit(values, value_stride, counts, count_stride, world, capacity, n_max, reg_covar, tol, max_iter, details):
    dev = values.device
    thr = torch.empty(1, dtype=torch.float32, device=dev)
    info = torch.empty(4, dtype=torch.int32, device=dev)
    labels = torch.empty(n_max, dtype=torch.int32, device=dev) if details else None
    scores = torch.empty(n_max, dtype=torch.float64, device=dev) if details else None
    want = details and n_max > 0            # the kernel writes n values through these: never hand it an empty tensor's pointer
    if int(max_iter) < 1:
        raise ValueError(f"max_iter must be >= 1, got {max_iter}")
    _lib.call("semidetr_gmm_fit_f64", dev, values, int(value_stride), counts, int(count_stride), int(world), int(capacity),
              COVARIANCE_DIAG, float(reg_covar), float(tol), int(max_iter), thr, labels if want else None,
              scores if want else None, info)
    if not details:
        return thr
    return thr, dict(labels=labels, scores=scores, n_iter=info[0], converged=info[1] != 0, error=info[2], info=info)


def fit_gmm_threshold(costs, covariance_type="diag", reg_covar=1e-5, tol=1e-3, max_iter=100, return_details=False):
    """costs: device fp32 vector of matched costs (any order).  Returns the (1,) fp32 device threshold, queued on the current
    stream (no host sync).  ``return_details=True`` returns ``(thr, details)``: ``labels`` (n,) int32 = predict, ``scores`` (n,)
    fp64 = score_samples, both in the INPUT order (the reference reports them for the sorted costs; equal costs get equal
    values, so sorting the input gives the reference's arrays), ``n_iter`` / ``converged`` / ``error`` 0-d device tensors
    (error 1: a component's covariance fell to <= 0, where sklearn raises; the threshold is NaN then)."""
    _check_covariance(covariance_type)
    if not costs.is_cuda:
        raise RuntimeError("fit_gmm_threshold: costs must live on the GPU (no CPU fallback)")
    x = costs.detach().reshape(-1).to(torch.float32).contiguous()
    n = x.numel()
    count = _lib.small_to_device([n], torch.int32, x.device)
    return _fit(x, n, count, 1, 1, n, n, reg_covar, tol, max_iter, return_details)


def fit_gmm_threshold_segments(values, counts, covariance_type="diag", reg_covar=1e-5, tol=1e-3, max_iter=100,
                               return_details=False):
    """The fit over a padded multi-segment buffer: values (W, capacity) fp32 device, counts (W,) int32 device; segment s holds
    ``values[s, :counts[s]]`` and the fit runs over their concatenation in segment order (what ``all_gather`` of one fixed-size
    segment per rank gives).  Labels / scores (details) are in that concatenated order, padded to W * capacity."""
    _check_covariance(covariance_type)
    if not (values.is_cuda and counts.is_cuda):
        raise RuntimeError("fit_gmm_threshold_segments: tensors must live on the GPU (no CPU fallback)")
    if values.dim() != 2 or values.dtype != torch.float32 or values.stride(1) != 1:
        raise ValueError("values must be a (W, capacity) fp32 tensor with contiguous rows")
    if counts.dtype != torch.int32 or counts.numel() != values.shape[0]:
        raise ValueError("counts must be a (W,) int32 tensor")
    W, cap = values.shape
    counts = counts.contiguous()
    return _fit(values, values.stride(0), counts, 1, W, cap, W * cap, reg_covar, tol, max_iter, return_details)


def fit_gmm(self, data_points, device=None):
    """``DinoDetrSSOD._fit_gmm`` as a method (``DinoDetrSSOD._fit_gmm = semi_detr_amd.fit_gmm``): the (1,) fp32 threshold on the
    GPU.  The reference's call site hands it the gathered costs on the CPU (dino_detr_ssod.py:303) and wraps the result in
    ``cost_.new_tensor``; a CPU input is moved to ``device`` (default: the current GPU) for the fit."""
    _check_covariance(getattr(self, "covariance_type", "diag"))
    x = torch.as_tensor(data_points)
    if not x.is_cuda:
        dev = torch.device(device) if device is not None and torch.device(device).type == "cuda" else \
            torch.device("cuda", torch.cuda.current_device())
        x = x.to(device=dev, dtype=torch.float32)
    return fit_gmm_threshold(x)


# ---------------------------------------------------------------------------------------------
# the segment buffer: one fixed-capacity segment per rank, its count in the last slot (int32 bits)
# ---------------------------------------------------------------------------------------------
def pack_segment(costs, capacity):
    """(capacity + 1,) fp32 buffer: ``costs`` in the first slots, len(costs) as int32 bits in the last.  (The device path writes
    this layout from the matching kernel directly; this host composition is for callers with a cost vector in hand.)"""
    n = costs.numel()
    if n > capacity:
        raise ValueError(f"{n} matched costs exceed the segment capacity {capacity}")
    buf = torch.zeros(capacity + 1, dtype=torch.float32, device=costs.device)
    buf[:n] = costs.reshape(-1)
    buf.view(torch.int32)[capacity] = n
    return buf


def gather_segments(buf, group=None):
    """One ``all_gather`` of every rank's (capacity + 1,) segment buffer -> (world, capacity + 1).  Every rank must use the
    same capacity (num_imgs x max_per_img).  World size 1 (or no process group): the buffer itself, as one row."""
    import torch.distributed as dist
    if not dist.is_available() or not dist.is_initialized() or dist.get_world_size(group) == 1:
        return buf.reshape(1, -1)
    world = dist.get_world_size(group)
    out = torch.empty((world, buf.numel()), dtype=buf.dtype, device=buf.device)
    dist.all_gather(list(out.unbind(0)), buf.contiguous(), group=group)
    return out


def segment_counts(gathered):
    """(world,) int32 view of the counts of a gathered (world, capacity + 1) segment buffer."""
    return gathered.view(torch.int32)[:, -1]


def segment_costs(gathered):
    """The concatenation of every segment's costs in rank order (a host-side read: for tests and tools)."""
    counts = segment_counts(gathered).tolist()
    return torch.cat([gathered[r, :c] for r, c in enumerate(counts)]) if counts else gathered.new_zeros(0)


# ---------------------------------------------------------------------------------------------
# the double filter
# ---------------------------------------------------------------------------------------------
GmmFilterResult = collections.namedtuple("GmmFilterResult", [
    "gt_bboxes_list", "gt_labels_list", "gt_scores_list",
    "unsup_bboxes_gmm_list", "unsup_labels_gmm_list", "unsup_scores_gmm_list",
    "det_bboxes_gmm_list", "det_labels_gmm_list", "det_scores_gmm_list",
    "thr", "match_gt_cost_list", "match_gt_inds_list"])


class PendingGmmFilter:
    """The filter's outputs with their list lengths still on the way to the host (pinned buffer + event), as
    ``PendingPseudoLabels``: ``result()`` waits for the event, checks the LSAP status and the fit, and slices."""

    def __init__(self, outs, thr, seg, cols, pair_offs, slot, label_dtypes, host_words):
        self._outs, self._thr, self._seg, self._cols = outs, thr, seg, cols
        self._pair_offs, self._slot, self._label_dtypes = pair_offs, slot, label_dtypes
        self._host = torch.empty(tuple(host_words.shape), dtype=torch.int32).pin_memory()
        self._host.copy_(host_words, non_blocking=True)
        self._event = torch.cuda.Event()
        self._event.record()
        self._result = None

    def result(self):
        if self._result is None:
            self._event.synchronize()
            words = self._host.tolist()
            B = len(self._pair_offs) - 1
            nb, nu, status, info = words[:B], words[B:2 * B], words[2 * B:3 * B], words[3 * B:]
            bad = [s for s in status if s]
            if bad:              # scipy's exceptions, as raise_on_status gives them
                raise ValueError("cost matrix is infeasible" if bad[0] == 1 else "matrix contains invalid numeric entries")
            if info[2]:
                raise RuntimeError("GMM fit failed: " + ("a component's covariance fell to <= 0 (sklearn raises: "
                                                         "ill-defined empirical covariance)" if info[2] == 1 else
                                                         "a rank's segment count is outside [0, capacity]"))
            (ob, ol, os_, gb, gl, gs, db, dl, ds) = self._outs
            m, po = self._slot, self._pair_offs

            def cut(t, counts, b, dt=None):
                v = t[b * m:b * m + counts[b]]
                return v if dt is None else v.to(dt)
            lt = self._label_dtypes
            self._result = GmmFilterResult(
                [cut(ob, nb, b) for b in range(B)], [cut(ol, nb, b, lt[b]) for b in range(B)],
                [cut(os_, nb, b) for b in range(B)],
                [cut(gb, nu, b) for b in range(B)], [cut(gl, nu, b, lt[b]) for b in range(B)],
                [cut(gs, nu, b) for b in range(B)],
                [cut(db, nu, b) for b in range(B)], [cut(dl, nu, b) for b in range(B)], [cut(ds, nu, b) for b in range(B)],
                self._thr,
                [self._seg[po[b]:po[b + 1]] for b in range(B)], [self._cols[po[b]:po[b + 1]] for b in range(B)])
        return self._result


def _cat(tensors, cols, dtype, dev):
    parts = [t.detach().reshape(-1, t.shape[-1])[:, :cols] if cols else t.detach().reshape(-1) for t in tensors]
    if not parts:
        return torch.zeros((0, cols) if cols else (0,), dtype=dtype, device=dev)
    return torch.cat([p.to(device=dev, dtype=dtype) for p in parts]).contiguous()


def unsup_gmm_filter(cls_scores, bbox_preds, gt_bboxes_list, gt_labels_list, gt_scores_list, det_bboxes_list,
                     det_labels_list, det_scores_list, img_metas, assigner, base_thr=0.4, group=None, max_per_img=300,
                     wait=True):
    """dino_detr_ssod.py:243-353 on the device.  cls_scores (B,Q,C) logits and bbox_preds (B,Q,4) normalised cxcywh of the
    student's last decoder layer; per image the strong-view pseudo gts ``gt_bboxes (G,4+)`` / ``gt_labels (G,)`` /
    ``gt_scores (G,)`` and the teacher's weak-view ``det_*`` (same G, same order); ``assigner``: the
    ``semi_detr_amd.HungarianAssigner`` whose cost weights build the matching cost (the reference's ``assigner2``);
    ``base_thr``: ``train_cfg.pseudo_label_initial_score_thr`` (compared in fp32).  With a process group of world size > 1
    the matched costs of every rank are gathered (one all_gather of a fixed (B * max_per_img + 1) buffer; every rank must
    pass the same B and max_per_img).  Returns a ``GmmFilterResult`` (the nine lists, ``thr`` (1,) fp32, and per image the
    matched costs / gt indices in scipy's pair order), or with ``wait=False`` a ``PendingGmmFilter``."""
    if not (cls_scores.is_cuda and bbox_preds.is_cuda):
        raise RuntimeError("unsup_gmm_filter: tensors must live on the GPU (no CPU fallback)")
    B, Q = int(bbox_preds.shape[0]), int(bbox_preds.shape[1])
    dev = bbox_preds.device
    lists = (gt_bboxes_list, gt_labels_list, gt_scores_list, det_bboxes_list, det_labels_list, det_scores_list, img_metas)
    if any(len(v) != B for v in lists):
        raise ValueError("unsup_gmm_filter: one entry per image expected in every list")
    counts = [int(g.shape[0]) if g.dim() > 1 else (1 if g.numel() else 0) for g in gt_bboxes_list]
    for b in range(B):
        if not (gt_labels_list[b].numel() == gt_scores_list[b].numel() == det_labels_list[b].numel()
                == det_scores_list[b].numel() == counts[b]) or det_bboxes_list[b].reshape(-1).numel() < 4 * counts[b]:
            raise ValueError(f"unsup_gmm_filter: image {b}: gt / det lists of different lengths")
    if counts and max(counts) > max_per_img:
        raise ValueError(f"unsup_gmm_filter: {max(counts)} pseudo boxes in an image exceed max_per_img={max_per_img}")
    gt_b = _cat(gt_bboxes_list, 4, torch.float32, dev)
    gt_l = _cat(gt_labels_list, 0, torch.int64, dev)
    gt_s = _cat(gt_scores_list, 0, torch.float32, dev)
    det_b = _cat(det_bboxes_list, 4, torch.float32, dev)
    det_l = _cat(det_labels_list, 0, torch.int64, dev)
    det_s = _cat(det_scores_list, 0, torch.float32, dev)
    wh = _lib.small_to_device([[m["img_shape"][1], m["img_shape"][0]] for m in img_metas] or [[1, 1]], torch.float32, dev)
    cost, offs_dev, offs = match_cost_batch(bbox_preds, cls_scores, gt_b, gt_l, counts, wh, assigner._cost_params())
    res = lsap_batch(cost, offs_dev, offs, Q, want_pairs=True, want_assign=False)
    pair_offs = res["pair_offsets"]
    num_pairs, cap = pair_offs[-1], B * int(max_per_img)
    if num_pairs > cap:
        raise ValueError(f"unsup_gmm_filter: {num_pairs} matched pairs exceed this rank's capacity {cap} "
                         f"(num_imgs x max_per_img)")
    pair_dev = _lib.small_to_device(pair_offs, torch.int32, dev)
    seg = torch.empty(cap + 1, dtype=torch.float32, device=dev)
    seg_i = seg.view(torch.int32)
    rows = res["rows"] if res["rows"].numel() else None
    cols = res["cols"]
    _lib.call("semidetr_gmm_match_costs_f32", dev, cost, offs_dev, pair_dev, rows, cols if num_pairs else None, B, Q,
              num_pairs, cap, seg, seg_i[cap:])
    gathered = gather_segments(seg, group)
    W = gathered.shape[0]
    thr, det = _fit(gathered, cap + 1, segment_counts(gathered), cap + 1, W, cap, 0, 1e-5, 1e-3, 100, True)
    slot = int(max_per_img)
    outs = (torch.empty((B * slot, 4), dtype=torch.float32, device=dev),
            torch.empty(B * slot, dtype=torch.int64, device=dev), torch.empty(B * slot, dtype=torch.float32, device=dev),
            torch.empty((B * slot, 4), dtype=torch.float32, device=dev),
            torch.empty(B * slot, dtype=torch.int64, device=dev), torch.empty(B * slot, dtype=torch.float32, device=dev),
            torch.empty((B * slot, 4), dtype=torch.float32, device=dev),
            torch.empty(B * slot, dtype=torch.int64, device=dev), torch.empty(B * slot, dtype=torch.float32, device=dev))
    out_counts = torch.empty(2 * B, dtype=torch.int32, device=dev)
    _lib.call("semidetr_gmm_double_filter_f32", dev, seg, pair_dev, cols if num_pairs else None, thr, gt_b, gt_l, gt_s, det_b,
              det_l, det_s, offs_dev, B, max(counts) if counts else 0, base_thr, slot, *outs, out_counts)
    words = torch.cat([out_counts, res["status"], det["info"]])
    pending = PendingGmmFilter(outs, thr, seg, cols, pair_offs, slot, [t.dtype for t in gt_labels_list], words)
    return pending.result() if wait else pending
