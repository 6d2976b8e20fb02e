"""Shared helpers of the set-loss fixture tests: tests/golden/set_loss.npz (written by tools/gen_set_loss_golden.py from
the reference's own ``loss()``) read per case, the loss-dict key -> (segment row, term) map of ``loss()``, and the
float64 restatement (set_loss_ref64.py) evaluated on a case's stored targets."""
import os

import numpy as np

import set_loss_ref64 as R

FIX = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "set_loss.npz"))
NAMES = [str(n) for n in FIX["names"]]
TERMS = ("loss_cls", "loss_bbox", "loss_iou", "loss_bbox_xy", "loss_bbox_hw")
INPUTS = ("all_cls", "all_box", "enc_cls", "enc_box", "dn_cls", "dn_box")


def case(name):
    c = {k.split(".", 1)[1]: FIX[k] for k in FIX.files if k.startswith(name + ".")}
    c["keys"] = [str(k) for k in c["keys"]]
    c["nl"], c["B"], c["Q"] = c["all_cls"].shape[:3]
    c["wh"] = c["img_hw"][:, ::-1].astype(np.float64)
    offs = np.concatenate([[0], np.cumsum(c["gt_counts"])])
    c["gt_list"] = [c["gt_boxes"][offs[b]:offs[b + 1]] for b in range(c["B"])]
    c["lab_list"] = [c["gt_labels"][offs[b]:offs[b + 1]] for b in range(c["B"])]
    return c


def key_rows(keys, nl):
    """loss-dict key -> (row, term): rows are the decoder layers, then the encoder, then the dn layers."""
    out = {}
    for k in keys:
        layer, name = (int(k[1:k.index(".")]), k[k.index(".") + 1:]) if k.startswith("d") and "." in k else (None, k)
        if name.startswith("enc_"):
            out[k] = (nl, TERMS.index(name[4:]))
        elif name.startswith("dn_"):
            out[k] = (nl + 1 + (nl - 1 if layer is None else layer), TERMS.index(name[3:]))
        else:
            out[k] = (nl - 1 if layer is None else layer, TERMS.index(name))
    return out


def ref64(c):
    """(values in key order, {input name: gradient}) of the restatement on the case's stored targets."""
    nl, B, Q = c["nl"], c["B"], c["Q"]
    warm = bool(c["warm_up"])
    kind = R.WARMUP if warm else R.MATCHED
    rows = key_rows(c["keys"], nl)
    T = 2 * nl + 1
    coef = np.zeros((T, 5))
    for k, cf in zip(c["keys"], c["coef"]):
        coef[rows[k]] = cf
    sh = lambda a, n: a.reshape((n, B, Q) + a.shape[2:])  # noqa: E731
    losses, grads = np.zeros((T, 5)), {}
    parts = [("all", slice(0, nl * B), nl, 0), ("enc", slice(nl * B, (nl + 1) * B), 1, nl)]
    for name, sl, n, t0 in parts:
        x = c[name + "_cls"] if name == "all" else c["enc_cls"][None]
        b = c[name + "_box"] if name == "all" else c["enc_box"][None]
        m = sh(c["norm_metrics"][sl], n) if warm else None
        args = (kind, x, b, sh(c["labels"][sl], n), None if warm else sh(c["label_weights"][sl], n),
                sh(c["bbox_targets"][sl], n), sh(c["bbox_weights"][sl], n), c["wh"])
        st = R.segment(*args, metrics=m)
        lo, sc = R.finalize(kind, st, R.norm_inputs(kind, st, B * Q), 2.0, 5.0, 2.0)
        _, gx, gb = R.segment(*args, metrics=m, coef=sc * coef[t0:t0 + n])
        losses[t0:t0 + n] = lo
        grads[name + "_cls"], grads[name + "_box"] = (gx, gb) if name == "all" else (gx[0], gb[0])
    sp, groups = int(c["single_pad"]), int(c["groups"])
    lab, lw, tg, bw = R.dn_targets(c["gt_list"], c["lab_list"], sp, groups, c["wh"], 80)
    rep = lambda a: np.broadcast_to(a, (nl,) + a.shape)  # noqa: E731
    args = (R.DN, c["dn_cls"], c["dn_box"], rep(lab), rep(lw), rep(tg), rep(bw), c["wh"])
    st = R.segment(*args)
    lo, sc = R.finalize(R.DN, st, R.norm_inputs(R.DN, st, B * sp * groups), 2.0, 5.0, 2.0)
    _, grads["dn_cls"], grads["dn_box"] = R.segment(*args, coef=sc * coef[nl + 1:])
    losses[nl + 1:] = lo
    return np.asarray([losses[rows[k]] for k in c["keys"]]), grads
