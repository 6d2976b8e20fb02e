"""The cross-view consistency loss of DinoDetrSSOD.unsup_loss (detr_ssod/models/dino_detr_ssod.py:463-481) restated with torch
operators: the baseline of tools/consis_loss_probe.py and of the agreement test.  It is never the code under test.

Test helper (not a conftest; imported by name like dn_torch_restated.py).  The same operator sequence per decoder layer as the
reference runs: slice to the pad, two advanced-index gathers, two F.normalize, mse_loss without reduction, weights, mean, x 10.
The weights multiply as a (K, 1) column, row k by w_k: the per-row statement of tests/consis_ref64.py (for a (K, 1) input the
reference's ``unsqueeze(-1)`` would broadcast to (K, K, D) instead; that only costs the baseline more).
"""
import torch
import torch.nn.functional as F


def consistency_loss(hs_v1, hs_v2, dn_meta, warm_up=True, scale=10):
    """-> {"consis_loss.d<l>": 0-d tensor}; ``hs_v1`` / ``hs_v2`` lists (or stacked tensors) of (B, Q, D)."""
    pad = dn_meta["pad_size_1"]
    rows_b, rows_q = dn_meta["known_bid_1"], dn_meta["map_known_indice_1"]
    weights = dn_meta["loss_weights"]
    if not warm_up:
        weights = torch.zeros_like(weights)
    out = {}
    for layer in range(len(hs_v1)):
        student, teacher = hs_v1[layer][:, :pad, ...], hs_v2[layer][:, :pad, ...]
        a = student[rows_b.long(), rows_q]
        b = teacher[rows_b.long(), rows_q]
        per_elem = F.mse_loss(F.normalize(a, p=2, dim=-1), F.normalize(b, p=2, dim=-1).detach(), reduction="none")
        out[f"consis_loss.d{layer}"] = scale * (per_elem * weights.reshape(-1, 1)).mean()
    return out
