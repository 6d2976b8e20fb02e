"""CPU: the float64 restatement (set_loss_ref64.py), fed the targets the reference's own ``get_targets`` produced,
reproduces every loss value and the gradients w.r.t. all six score / box inputs of the reference's own ``loss()``
(tests/golden/set_loss.npz, tools/gen_set_loss_golden.py) to 1e-12 relative, and the fixture's keys come in the order
``loss()`` builds them."""
import numpy as np
import pytest

import set_loss_fixture as F


def _keys(nl):
    ks = ["enc_" + t for t in F.TERMS] + list(F.TERMS) + ["dn_" + t for t in F.TERMS]
    for i in range(nl - 1):
        ks += [f"d{i}.{t}" for t in F.TERMS] + [f"d{i}.dn_{t}" for t in F.TERMS]
    return ks


@pytest.mark.parametrize("name", F.NAMES)
def test_ref64_reproduces_reference_fixture(name):
    c = F.case(name)
    assert c["keys"] == _keys(c["nl"])
    vals, grads = F.ref64(c)
    np.testing.assert_allclose(vals, c["values"], rtol=1e-12, atol=1e-14)
    for k in F.INPUTS:
        g, want = grads[k], c["grad_" + k]
        # warm-up TAL: 1 - sigmoid(x) at the larger logits keeps fewer digits in fp64 on either side (test_set_loss_ref)
        atol = (1e-9 if c["warm_up"] and k.endswith("cls") else 1e-12) * max(np.abs(want).max(), 1e-300)
        np.testing.assert_allclose(g, want, rtol=1e-12, atol=atol, err_msg=k)


def test_fixture_covers_the_cases():
    c = {n: F.case(n) for n in F.NAMES}
    assert bool(c["warm_up"]["warm_up"]) and bool(c["hungarian_pseudo"]["is_pseudo_label"])
    assert (c["hungarian"]["gt_counts"] == 0).any()                               # an image without ground truth
    assert c["q_lt_g"]["Q"] < c["q_lt_g"]["gt_counts"].max()                       # Q < G
    z = c["no_gt"]
    assert not (z["bbox_weights"] > 0).any()                                        # GIoULoss's early return
    assert max(np.abs(c["hungarian"]["all_cls"]).max(), np.abs(c["hungarian"]["dn_cls"]).max()) >= 30
