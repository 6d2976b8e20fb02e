"""ctypes binding of ``libsemidetr_hip.so`` (C ABI declared in ``include/semidetr_hip.h``).

There is NO fallback: if the shared library is missing or a call fails, an exception is raised.  The
library is built in-tree by ``__graft_entry__.build()`` / ``make -C semi-detr_amd/csrc``.
"""
import contextlib
import ctypes
import os

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
# SEMIDETR_EXPERIMENTS=1 (tests that force kernel variants, tools/, bench.py's HBM-peak probe) selects the experiments
# build: the same sources with every measured-and-rejected kernel variant + the tuning entry points
# (include/semidetr_hip_experiments.h).  The product library has neither.
EXPERIMENTS = os.environ.get("SEMIDETR_EXPERIMENTS", "0") not in ("", "0")
LIB_PATH = os.path.join(_HERE, "csrc", "libsemidetr_hip_exp.so" if EXPERIMENTS else "libsemidetr_hip.so")

c_void_p, c_int, c_int64, c_double = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64, ctypes.c_double


class CostParams(ctypes.Structure):
    """Mirror of ``semidetr_cost_params`` (include/semidetr_hip.h)."""
    _fields_ = [("cls_weight", ctypes.c_float), ("alpha", ctypes.c_float), ("gamma", ctypes.c_float),
                ("eps", ctypes.c_float), ("reg_weight", ctypes.c_float), ("reg_xywh", ctypes.c_int),
                ("iou_weight", ctypes.c_float), ("iou_giou", ctypes.c_int), ("pred_xyxy", ctypes.c_int)]


_MSDA_FWD = [c_void_p] * 6 + [c_int] * 7 + [c_void_p]
_MSDA_BWD = [c_void_p] * 7 + [c_int] * 7 + [c_void_p] * 3
_MSDA_FWD_F32 = [c_void_p] * 6 + [c_int] * 8 + [c_void_p]           # f32 entry points carry `flags`
_MSDA_BWD_F32 = [c_void_p] * 7 + [c_int] * 8 + [c_void_p] * 3

# name -> (restype, argtypes); must list every function include/semidetr_hip.h declares
SIGNATURES = {
    "semidetr_abi_version": (c_int, []),
    "semidetr_last_error": (ctypes.c_char_p, []),
    "semidetr_msda_forward_f32": (c_int, _MSDA_FWD_F32),
    "semidetr_msda_forward_f64": (c_int, _MSDA_FWD),
    "semidetr_msda_backward_f32": (c_int, _MSDA_BWD_F32),
    "semidetr_msda_backward_f64": (c_int, _MSDA_BWD),
    "semidetr_msda_fused_forward_f32": (c_int, [c_void_p] * 5 + [c_int] + [c_void_p] * 4 + [c_int] * 8 + [c_void_p]),
    "semidetr_msda_fused_backward_f32": (c_int, [c_void_p] * 6 + [c_int] + [c_void_p] * 4 + [c_int] * 8 + [c_void_p] * 3),
    "semidetr_msda_mask_extents": (c_int, [c_void_p] * 4 + [c_int] * 3 + [c_void_p]),
    "semidetr_msda_last_kernels": (ctypes.c_char_p, []),
    "semidetr_msda_forward_h16": (c_int, [c_void_p, c_int] + [c_void_p] * 5 + [c_int] * 7 + [c_void_p]),
    "semidetr_msda_backward_h16_workspace_bytes": (ctypes.c_size_t, [c_int] * 4),
    "semidetr_msda_backward_h16": (c_int, [c_void_p, c_int] + [c_void_p] * 6 + [c_int] * 7 + [c_void_p] * 4),
    "semidetr_msda_h16_last_kernels": (ctypes.c_char_p, []),
    "semidetr_msda_set_forward_policy": (c_int, [c_int]),
    "semidetr_msda_forward_policy_state": (c_int, [c_void_p] * 4),
    "semidetr_msda_forward_policy_state_slot": (c_int, [c_int] + [c_void_p] * 4),
    "semidetr_msda_gather_choice": (c_int, [c_int]),
    "semidetr_match_cost_f32": (c_int, [c_void_p] * 7 + [c_int] * 4 + [ctypes.POINTER(CostParams), c_void_p]),
    "semidetr_lsap_workspace_bytes": (c_int64, [c_int, c_int, c_int]),
    "semidetr_lsap_solve": (c_int, [c_void_p] * 4 + [c_int] * 4 + [c_void_p] * 6),
    "semidetr_build_targets": (c_int, [c_void_p] * 6 + [c_int, c_int, c_int64] + [c_void_p] * 5),
    "semidetr_ema_multi_f32": (c_int, [c_void_p] * 5 + [c_int, c_int, c_double]),
    "semidetr_ema_flat_f32": (c_int, [c_void_p, c_void_p, c_void_p, c_int64, c_double]),
    "semidetr_pseudo_label_filter_f32": (c_int, [c_void_p] * 5 + [c_int] + [c_void_p] * 6),
    "semidetr_nms_workspace_bytes": (ctypes.c_size_t, [c_int, c_int, c_int]),
    "semidetr_pseudo_nms_f32": (c_int, [c_void_p] * 4 + [c_int] * 3 + [ctypes.c_float, ctypes.c_float, c_int, c_void_p,
                                                                       ctypes.c_size_t] + [c_void_p] * 3),
    "semidetr_o2m_assign_f32": (c_int, [c_void_p] * 7 + [c_int] * 7 + [ctypes.c_float, ctypes.c_float] + [c_void_p] * 7),
    "semidetr_tal_loss_workspace_bytes": (ctypes.c_size_t, []),
    "semidetr_tal_loss_f32": (c_int, [c_void_p] * 4 + [c_int64, c_int, ctypes.c_float, c_int] + [c_void_p] * 3),
    "semidetr_transform_bboxes_f32": (c_int, [c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_int, c_int] + [c_void_p] * 3),
    "semidetr_gmm_match_costs_f32": (c_int, [c_void_p] * 6 + [c_int] * 4 + [c_void_p] * 2),
    "semidetr_gmm_fit_f64": (c_int, [c_void_p, c_void_p, c_int64, c_void_p, c_int64] + [c_int] * 3 + [c_double, c_double, c_int]
                             + [c_void_p] * 4),
    "semidetr_gmm_double_filter_f32": (c_int, [c_void_p] * 12 + [c_int, c_int, ctypes.c_float, c_int] + [c_void_p] * 10),
    # the segment table (semidetr_set_loss_segment[], set_loss._Segment) is passed as a host pointer
    "semidetr_set_loss_workspace_bytes": (c_int64, [c_void_p, c_int]),
    "semidetr_set_loss_forward_f32": (c_int, [c_void_p, c_void_p, c_int, c_void_p, c_int64] + [c_void_p] * 4),
    "semidetr_set_loss_finalize_f32": (c_int, [c_void_p, c_void_p, c_int] + [c_void_p] * 5),
    "semidetr_set_loss_backward_f32": (c_int, [c_void_p, c_void_p, c_int, c_void_p, c_void_p]),
    # the parameter blocks (semidetr_dn_build / _consistency / _layout, dn_query._Build ...) are passed as host pointers
    "semidetr_dn_build_f32": (c_int, [c_void_p, c_void_p]),
    "semidetr_dn_consistency_f32": (c_int, [c_void_p, c_void_p]),
    "semidetr_dn_label_backward_f32": (c_int, [c_void_p] * 5 + [c_int] * 5 + [c_void_p]),
    "semidetr_dn_gather_rows_f32": (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_void_p]),
    # two-stage query selection (query_select.py)
    "semidetr_qsel_proposals_f32": (c_int, [c_void_p] * 5 + [c_int] * 4 + [c_void_p] * 3),
    "semidetr_qsel_proposals_backward_f32": (c_int, [c_void_p] * 3 + [c_int] * 3 + [c_void_p]),
    "semidetr_qsel_topk_workspace_bytes": (ctypes.c_size_t, [c_int, c_int]),
    "semidetr_qsel_topk_f32": (c_int, [c_void_p, c_void_p] + [c_int] * 4 + [c_void_p, ctypes.c_size_t, c_void_p, c_void_p]),
    "semidetr_qsel_gather_f32": (c_int, [c_void_p] * 5 + [c_int] * 4 + [c_void_p] * 4),
    "semidetr_qsel_gather_backward_f32": (c_int, [c_void_p] * 6 + [c_int] * 4 + [c_void_p] * 2),
    # detection decode at evaluation / inference time (detect.py)
    "semidetr_det_workspace_bytes": (ctypes.c_size_t, [c_int] * 4),
    "semidetr_det_decode_f32": (c_int, [c_void_p] * 5 + [c_int] * 4 + [c_void_p, ctypes.c_size_t] + [c_void_p] * 4),
    # cross-view consistency loss (consis_loss.py); the parameter block (semidetr_consis_loss, consis_loss._Params) is a host pointer
    "semidetr_consis_loss_workspace_bytes": (ctypes.c_size_t, [c_int] * 4),
    "semidetr_consis_loss_forward_f32": (c_int, [c_void_p, c_void_p, c_void_p, ctypes.c_size_t, c_void_p]),
    "semidetr_consis_loss_backward_f32": (c_int, [c_void_p, c_void_p, c_void_p, ctypes.c_size_t, c_void_p]),
    # decoder self-attention core (self_attn.py); the parameter block (semidetr_self_attn, self_attn._Params) is a host pointer
    "semidetr_self_attn_workspace_bytes": (ctypes.c_size_t, [c_int] * 4),
    "semidetr_self_attn_forward_f32": (c_int, [c_void_p, c_void_p, c_void_p, ctypes.c_size_t]),
    "semidetr_self_attn_backward_f32": (c_int, [c_void_p, c_void_p, c_void_p, ctypes.c_size_t]),
    # residual add + LayerNorm + positional add (add_norm.py); the parameter block (semidetr_add_norm, add_norm._Params) is a host pointer
    "semidetr_add_norm_workspace_bytes": (ctypes.c_size_t, [c_int64]),
    "semidetr_add_norm_forward_f32": (c_int, [c_void_p, c_void_p, c_void_p, ctypes.c_size_t]),
    "semidetr_add_norm_backward_f32": (c_int, [c_void_p, c_void_p, c_void_p, ctypes.c_size_t]),
}

# include/semidetr_hip_experiments.h: only in libsemidetr_hip_exp.so
EXPERIMENT_SIGNATURES = {
    "semidetr_msda_set_variant": (None, [c_int, c_int]),
    "semidetr_debug_counters": (c_int, [c_void_p, c_int]),
    "semidetr_stream_copy_f32": (c_int, [c_void_p, c_void_p, c_void_p, c_int64, c_int]),
}

_lib = None


class NativeLibraryError(RuntimeError):
    pass


def lib():
    """Load the shared library (once).  Raises ``NativeLibraryError`` when it is not built."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise NativeLibraryError(
                f"{LIB_PATH} not found: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                "or `make -C semi-detr_amd/csrc` (hipcc --offload-arch=gfx950). There is no CPU fallback.")
        handle = ctypes.CDLL(LIB_PATH)
        table = dict(SIGNATURES, **EXPERIMENT_SIGNATURES) if EXPERIMENTS else SIGNATURES
        for name, (res, args) in table.items():
            fn = getattr(handle, name)       # AttributeError if the .so is stale / symbol missing
            fn.restype, fn.argtypes = res, args
        _lib = handle
    return _lib


def check(rc, what):
    """Turn a C-ABI status into a RuntimeError (what the reference's AT_ASSERTM / launch failures give)."""
    if rc != 0:
        msg = lib().semidetr_last_error().decode(errors="replace")
        raise RuntimeError(f"{what} failed (code {rc}): {msg}")


def current_stream_ptr():
    return c_void_p(torch.cuda.current_stream().cuda_stream)


# ---------------------------------------------------------------------------------------------
# the one call path of the host mirrors
# ---------------------------------------------------------------------------------------------
_NO_GUARD = contextlib.nullcontext()
_Tensor = torch.Tensor              # bound once: ptr_args tests every argument of every launch
_functions = {}                     # name -> (library handle, function): looked up and checked once per handle


def device_guard(dev):
    """Device guard only where ``dev`` is not the current device (entering ``torch.cuda.device`` costs more than a launch).
    A ``dev`` without an index is the current device."""
    if dev.index is None or dev.index == torch.cuda.current_device():
        return _NO_GUARD
    return torch.cuda.device(dev)


def ptr_args(args):
    """Arguments of a C-ABI call: a tensor becomes its data pointer, ``None`` stays ``None`` (NULL for a ``c_void_p``), anything
    else (Python numbers, ctypes instances, ``ctypes.byref(...)``, ctypes arrays) is left to the argtypes of ``SIGNATURES``."""
    return [c_void_p(a.data_ptr()) if isinstance(a, _Tensor) else a for a in args]


def _function(name):
    hit = _functions.get(name)
    if hit is not None and hit[0] is _lib:
        return hit[1]
    if name not in SIGNATURES and not (EXPERIMENTS and name in EXPERIMENT_SIGNATURES):
        raise AttributeError(f"{name} is not a function of the C ABI (_lib.SIGNATURES)")
    fn = getattr(lib(), name)
    _functions[name] = (_lib, fn)
    return fn


def calls(dev, *launches):
    """Launches back to back, each a ``(name, *args)``: ``name(stream, *args)`` on the current stream of ``dev`` with ``dev``
    current, under one guard decision and one stream lookup.  Every name is resolved before the first launch; a non-zero status
    raises (``check``) before the next one.  Every entry point that launches takes ``void *stream`` first; the size queries are
    plain ``lib().f(...)`` calls."""
    fns = [_function(launch[0]) for launch in launches]
    with device_guard(dev):
        stream = c_void_p(torch.cuda.current_stream(dev).cuda_stream)
        for fn, launch in zip(fns, launches):
            rc = fn(stream, *ptr_args(launch[1:]))
            if rc:
                check(rc, launch[0])


def call(name, dev, *args):
    """One launch: ``calls(dev, (name, *args))``."""
    calls(dev, (name,) + args)


def small_to_device(values, dtype, dev):
    """Small host list -> device tensor without a stream synchronisation (pinned staging + async copy); a plain
    ``torch.tensor(list, device=...)`` is a blocking copy that drains the stream on every call."""
    host = torch.tensor(values, dtype=dtype)
    if dev.type == "cuda":
        return host.pin_memory().to(dev, non_blocking=True)
    return host.to(dev)


def offsets(counts, dev):
    """Exclusive prefix sum of ``counts`` as (host list, int32 device tensor), one entry more than ``counts``."""
    offs = [0]
    for c in counts:
        offs.append(offs[-1] + int(c))
    return offs, small_to_device(offs, torch.int32, dev)


FORWARD_POLICIES = {"adaptive": 0, "patch": 1, "window": 2}


def set_forward_policy(policy):
    """Which kernel runs the encoder self-attention forward: "adaptive" (default: chosen from how far the samples of the
    previous launches reached), "patch" or "window" (include/semidetr_hip.h, semidetr_msda_set_forward_policy)."""
    check(lib().semidetr_msda_set_forward_policy(FORWARD_POLICIES.get(policy, policy)), "semidetr_msda_set_forward_policy")


def forward_policy_state(slot=0):
    """{'policy', 'mode' (0 patch / 1 window), 'far_fraction' (-1: no count received yet), 'updates'} of the current device and
    call-site slot (0 = the slot of callers that name none; MSDeformAttn instances hold theirs in ``policy_slot``)."""
    pol, mode, upd, frac = c_int(), c_int(), ctypes.c_uint(), ctypes.c_float()
    check(lib().semidetr_msda_forward_policy_state_slot(int(slot), ctypes.byref(pol), ctypes.byref(mode), ctypes.byref(frac),
                                                        ctypes.byref(upd)), "semidetr_msda_forward_policy_state_slot")
    return {"policy": pol.value, "mode": mode.value, "far_fraction": frac.value, "updates": upd.value}


def set_variant(fwd, bwd):
    """Force a kernel variant (experiments build only).  (0, 0) is always accepted: the product library has no variants."""
    if EXPERIMENTS:
        lib().semidetr_msda_set_variant(int(fwd), int(bwd))
    elif (fwd, bwd) != (0, 0):
        raise NativeLibraryError("kernel variants exist only in the experiments build: set SEMIDETR_EXPERIMENTS=1 "
                                 "(libsemidetr_hip_exp.so) before importing semi_detr_amd")
