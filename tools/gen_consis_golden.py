#!/usr/bin/env python
"""Generate tests/golden/consis_loss.npz from the REFERENCE's own consistency-loss loop: the ``for layer_id ...`` statement of
``DinoDetrSSOD.unsup_loss`` (detr_ssod/models/dino_detr_ssod.py:472-481) is taken out of the file with ``ast`` at run time and
executed on stand-in locals (the module itself imports mmcv and mmdet).  Runs on the CPU where the reference tree exists; what
it writes is data.

    python tools/gen_consis_golden.py

Every case of ``consis_cases.FIXTURE_CASES`` runs twice, in float32 and in float64 (inputs drawn in float32 and up-cast).  ``hs``
is built as the reference builds it: per layer a ``(Q, B, D)`` buffer, ``hs[l]`` its ``transpose(0, 1)``.

Per case ``<case>.``: the inputs ``buf_v1`` / ``buf_v2`` (L, Q, B, D) float32, ``bid`` float32, ``idx`` int64, ``weights``
float32, ``pad_size``, ``upstream`` (the c_l of the differentiated scalar ``sum_l c_l loss_l``); recorded: ``loss64`` / ``loss32``
(L,), ``grad64`` / ``grad32`` (L, K, D) = the gradient w.r.t. ``hs_v1[l]`` at the selected rows, ``rest64`` / ``rest32`` (L,) =
sum |gradient| over every other row (the checksum of the rest), ``grad_v2_abs`` = sum |gradient| w.r.t. ``hs_v2`` (detached: 0).

The shape of ``loss_weights``.  These runs hand the loop the weights as a ``(K,)`` vector, for which its ``unsqueeze(-1)`` weights
row k by w_k: the per-row statement that the kernel implements.  ``prepare_unsup_cdn`` produces a ``(K, 1)`` column, for which the
same expression broadcasts ``(K, D) * (K, 1, 1)`` to ``(K, K, D)`` and the loop returns mean(w) times the UNWEIGHTED mean: the two
agree exactly where the weights are uniform (every image has a pseudo box, or past the warm-up) and differ where a batch mixes
images with and without pseudo boxes.  ``loss64_column`` / ``grad64_column`` record the float64 run with the column, for
``uniform_weights`` (agreement) and ``image_weight_zero`` (the difference), so that the tests pin both facts.
"""
import ast
import os
import sys
import textwrap

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle.gen_golden import REF  # noqa: E402
sys.path.insert(0, os.path.join(ROOT, "tests"))
import consis_cases  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "consis_loss.npz")
SRC = REF + "/detr_ssod/models/dino_detr_ssod.py"


def loop_source():
    src = open(SRC).read()
    tree = ast.parse(src)
    cls = next(n for n in ast.walk(tree) if isinstance(n, ast.ClassDef) and n.name == "DinoDetrSSOD")
    fn = next(n for n in cls.body if isinstance(n, ast.FunctionDef) and n.name == "unsup_loss")
    loops = [n for n in ast.walk(fn) if isinstance(n, ast.For) and getattr(n.target, "id", None) == "layer_id"
             and "consis_loss" in ast.get_source_segment(src, n)]
    assert len(loops) == 1, len(loops)
    return textwrap.dedent(ast.get_source_segment(src, loops[0], padded=True))


def run(case, code, f64, column=False):
    dt = torch.float64 if f64 else torch.float32
    bufs1 = [torch.from_numpy(b).to(dt).requires_grad_(True) for b in case["buf_v1"]]
    bufs2 = [torch.from_numpy(b).to(dt).requires_grad_(True) for b in case["buf_v2"]]
    env = dict(torch=torch, F=F, losses={}, hs_v1=[b.transpose(0, 1) for b in bufs1], hs_v2=[b.transpose(0, 1) for b in bufs2],
               pad_size=int(case["pad_size"]), known_bid=torch.from_numpy(case["bid"]),
               map_known_indice=torch.from_numpy(case["idx"]), loss_weights=torch.from_numpy(case["weights"]).to(dt).reshape((-1, 1) if column else (-1,)))
    exec(code, env)
    losses = [env["losses"][f"consis_loss.d{l}"] for l in range(len(bufs1))]
    total = sum(float(c) * v for c, v in zip(case["upstream"], losses))
    total.backward()
    b, q = case["bid"].astype(np.int64), case["idx"]
    rows, rest = [], []
    for buf in bufs1:
        g = buf.grad.transpose(0, 1).numpy().copy()                  # (B, Q, D)
        rows.append(g[b, q].copy())
        g[b, q] = 0
        rest.append(np.abs(g).sum())
    v2 = sum(0.0 if buf.grad is None else float(buf.grad.abs().sum()) for buf in bufs2)
    return np.array([float(v.detach()) for v in losses], np.float64 if f64 else np.float32), np.stack(rows), np.array(rest), v2


def main():
    code = compile(loop_source(), SRC, "exec")
    out = {}
    for name, build in consis_cases.FIXTURE_CASES.items():
        case = build()
        for k in ("buf_v1", "buf_v2"):
            out[f"{name}.{k}"] = np.stack(case[k])
        for k in ("bid", "idx", "weights", "upstream"):
            out[f"{name}.{k}"] = case[k]
        out[f"{name}.pad_size"] = np.int64(case["pad_size"])
        v2 = 0.0
        for tag, f64 in (("32", False), ("64", True)):
            loss, rows, rest, g2 = run(case, code, f64)
            assert loss.dtype == (np.float64 if f64 else np.float32) and rows.dtype == loss.dtype
            out[f"{name}.loss{tag}"], out[f"{name}.grad{tag}"], out[f"{name}.rest{tag}"] = loss, rows, rest
            v2 += g2
        out[f"{name}.grad_v2_abs"] = np.float64(v2)
        if name in ("uniform_weights", "image_weight_zero"):
            out[f"{name}.loss64_column"], out[f"{name}.grad64_column"], _, _ = run(case, code, True, column=True)
    np.savez_compressed(OUT, **out)
    size = os.path.getsize(OUT)
    assert size < (1 << 20), size
    print(f"wrote {OUT}: {len(out)} arrays, {size} bytes")


if __name__ == "__main__":
    main()
