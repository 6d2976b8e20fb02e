"""GPU: every byte the self-attention's four C-ABI entry points write is what tests/golden/self_attn_bits.json records
(tools/gen_self_attn_bits.py; the file names the commit whose library produced it): a sha256 of ``out``, ``lse``, ``dq``, ``dk``
and ``dv`` per case, element type (fp32, fp16, bf16) and gradient subset of ``self_attn_abi.BITS_CASES``, through the C ABI into
NaN-filled buffers, so an unasked gradient's untouched fill is part of the digest.

The digests pin this hardware's MFMA summation (the order and rounding of the additions inside ``v_mfma_f32_32x32x16_*`` are not
documented) and the compiler's contraction of the VALU arithmetic around it: they hold on the MI355X with the toolchain the
library is built with, and say nothing about another GPU.  A change that restructures the kernels keeps them; a deliberate
change of the numerics contract (include/semidetr_hip.h) regenerates them with the tool and says so."""
import json
import os

import pytest

import self_attn_abi as abi

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "self_attn_bits.json")


@pytest.mark.parametrize("dt", abi.DTYPES)
def test_every_output_byte_is_the_recorded_one(dt):
    with open(GOLDEN) as f:
        rec = json.load(f)
    want = {k: v for k, v in rec["digests"].items() if k.split("/")[1] == dt}
    got = abi.bits(dt)
    assert set(got) == set(want) and len(got) == len(abi.BITS_CASES) + 2, "the recorded runs are not the runs of BITS_CASES"
    bad = [(k, n) for k in sorted(got) for n in sorted(want[k]) if got[k].get(n) != want[k][n]]
    bad += [(k, "results") for k in got if set(got[k]) != set(want[k])]
    assert not bad, f"bytes differ from {rec['recorded_from']}: {bad}"
