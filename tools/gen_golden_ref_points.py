#!/usr/bin/env python3
"""Writes tests/golden/ref_points.npz: the reference's own ``inverse_sigmoid`` and ``gen_sineembed_for_position``
(detr_od/models/utils/transformer.py:435-451, 467-493; the sources are taken from the file with ``ast`` at run time and
executed -- the module itself imports mmcv, cv2 and timm, which are absent) on small inputs, evaluated in float64 on the CPU.
The fixture is data (inputs + expected outputs); nothing of the reference's source travels.  tests/test_ref_points_ref.py
compares tests/ref_points_torch_restated.py against the fixture everywhere, and against the functions themselves where the
reference checkout is present.

    python tools/gen_golden_ref_points.py [--reference /path/to/checkout]
"""
import argparse
import ast
import math
import os
import textwrap

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = os.environ.get("SEMIDETR_REFERENCE", "/root/reference")
SRC = "detr_od/models/utils/transformer.py"
OUT = os.path.join(ROOT, "tests", "golden", "ref_points.npz")


def _function_source(path, name):
    src = open(path).read()
    for node in ast.walk(ast.parse(src)):
        if isinstance(node, ast.FunctionDef) and node.name == name:
            return textwrap.dedent(ast.get_source_segment(src, node, padded=True))
    raise KeyError(name)


def load_reference(ref=REF):
    """(inverse_sigmoid, gen_sineembed_for_position) of the checkout at ``ref``, or ``None`` where it is absent"""
    path = os.path.join(ref, SRC)
    if not os.path.exists(path):
        return None
    ns = {"torch": torch, "math": math}
    for name in ("inverse_sigmoid", "gen_sineembed_for_position"):
        exec(_function_source(path, name), ns)
    return ns["inverse_sigmoid"], ns["gen_sineembed_for_position"]


def inputs():
    """the fixture's inputs: coordinates with the kinks of inverse_sigmoid and of the embedding, and values outside [0, 1]"""
    rng = np.random.default_rng(42)
    eps = float(np.float32(1e-5))
    special = np.asarray([0.0, 1.0, 0.5, 0.25, eps, 1.0 - eps, -0.25, 1.5, 1e-7, 1.0 - 1e-7], np.float32)
    x = np.concatenate([special, rng.random(54).astype(np.float32)]).reshape(8, 2, 4)
    return {"x": x, "pos4": x[:5].copy(), "pos2": x[3:, :, :2].copy()}


def outputs(fns, data):
    inverse_sigmoid, gen_sineembed = fns
    x = torch.from_numpy(data["x"]).double()
    return {"inv": inverse_sigmoid(x).numpy(), "inv_eps3": inverse_sigmoid(x, eps=1e-3).numpy(),
            "embed4": gen_sineembed(torch.from_numpy(data["pos4"]).double()).numpy(),
            "embed2": gen_sineembed(torch.from_numpy(data["pos2"]).double()).numpy()}


def main():
    ap = argparse.ArgumentParser(description=__doc__)
    ap.add_argument("--reference", default=REF)
    args = ap.parse_args()
    fns = load_reference(args.reference)
    if fns is None:
        raise SystemExit(f"no reference checkout at {args.reference}")
    data = inputs()
    data.update(outputs(fns, data))
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    np.savez_compressed(OUT, **data)
    print(f"wrote {OUT}: " + ", ".join(f"{k}{list(v.shape)}" for k, v in data.items()))


if __name__ == "__main__":
    main()
