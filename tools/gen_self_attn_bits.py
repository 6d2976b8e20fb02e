#!/usr/bin/env python
"""Record tests/golden/self_attn_bits.json: a sha256 of the raw bytes of ``out``, ``lse``, ``dq``, ``dk`` and ``dv`` that the
self-attention's four C-ABI entry points write on the GPU, per case, element type and gradient subset
(``tests/self_attn_abi.py``: ``BITS_CASES`` in fp32, fp16 and bf16 through ``run_abi``, NaN-filled buffers, the case's own
layout).  tests/test_gpu_self_attn_bits.py asserts that the built library reproduces every digest, so a change of the kernels
that is meant to keep the bits is checked against what the library gave BEFORE it: build the commit to compare with in a second
checkout and record from its library,

    python tools/gen_self_attn_bits.py --commit <hash of that commit> --lib <its checkout>/semi-detr_amd/csrc/libsemidetr_hip.so

The digests pin this hardware's MFMA summation (MI355X, gfx950) and the compiler's choice of fmas; a deliberate change of the
numerics contract records them again from the new library (no ``--lib``: the one of this tree).  Needs a GPU.
"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

OUT = os.path.join(ROOT, "tests", "golden", "self_attn_bits.json")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--commit", required=True, help="the commit whose library is recorded (written into the file)")
    ap.add_argument("--lib", default=None, help="libsemidetr_hip.so to record from (default: the one of this tree)")
    ap.add_argument("--out", default=OUT)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "the digests are those of the GPU"
    from semi_detr_amd import _lib
    if a.lib:
        _lib.LIB_PATH = os.path.abspath(a.lib)          # before the first call loads it
    import self_attn_abi as abi
    digests = {}
    for dt in abi.DTYPES:
        digests.update(abi.bits(dt))
    rec = {"recorded_from": f"libsemidetr_hip.so of commit {a.commit}", "device": torch.cuda.get_device_name(0),
           "torch": torch.__version__, "digests": digests}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(rec, f, indent=1, sort_keys=True)
        f.write("\n")
    print(f"wrote {a.out}: {len(digests)} runs from {rec['recorded_from']} on {rec['device']}")


if __name__ == "__main__":
    main()
