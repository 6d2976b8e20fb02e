"""Inputs of the consistency-loss tests (tests/test_consis_ref.py, tests/test_gpu_consis_loss.py), of the fixture generator
(tools/gen_consis_golden.py) and of the probe.  Test helper (not a conftest; imported by name like loss_cases.py).  Numpy only.

A case holds what the reference holds at that point: per view and decoder layer a ``(Q, B, D)`` float32 buffer whose
``transpose(0, 1)`` is ``hs[l]`` (transformer.py:1042-1043), and the ``dn_meta`` entries of ``prepare_unsup_cdn``: ``bid`` (K,)
float32, ``idx`` (K,) int64 with ``idx = i + single_pad * g`` over the 5 groups, ``weights`` (K,) float32, ``pad_size``; plus
``upstream`` (L,) float32, the coefficient of each layer's loss in the scalar that is differentiated (0 = that loss is unused).
Rows are LayerNorm-like (zero mean, unit variance, an affine of about 1 +- 0.1) so that every norm is far from eps.
"""
import numpy as np

F = np.float32
GROUPS = 5


def layout(counts, groups=GROUPS):
    """known_bid, map_known_indice, single_pad, pad_size as the reference lays the consistency queries out"""
    single = max(counts)
    bid = np.concatenate([np.full(n, b) for b, n in enumerate(counts)])
    within = np.concatenate([np.arange(n) for n in counts])
    return (np.tile(bid, groups).astype(F), np.concatenate([within + single * g for g in range(groups)]).astype(np.int64),
            single, single * groups)


def _ln_rows(rng, shape):
    x = rng.standard_normal(shape)
    x = (x - x.mean(-1, keepdims=True)) / x.std(-1, keepdims=True)
    D = shape[-1]
    return (x * (1 + 0.1 * rng.standard_normal(D)) + 0.1 * rng.standard_normal(D)).astype(F)


def make(L, counts, extra_q, D, seed, weights="mixed", upstream=None, groups=GROUPS, eps=1e-12, scale=10.0):
    rng = np.random.default_rng(seed)
    B = len(counts)
    bid, idx, single, pad = layout(counts, groups)
    Q, K = pad + extra_q, len(bid)
    buf1 = [_ln_rows(rng, (Q, B, D)) for _ in range(L)]
    buf2 = [_ln_rows(rng, (Q, B, D)) * F(0.6) + b * F(0.8) for b in buf1]      # the other view: correlated, not equal
    if weights == "mixed":
        w = rng.choice(np.array([0.25, 0.5, 1.0, 1.0, 1.5, 2.0], F), K).astype(F)
    elif weights == "ones":
        w = np.ones(K, F)
    else:
        w = np.asarray(weights, F)
    if upstream is None:
        upstream = (0.5 + rng.random(L)).astype(F)
    return dict(buf_v1=buf1, buf_v2=buf2, bid=bid, idx=idx, weights=w, pad_size=pad, upstream=np.asarray(upstream, F),
                eps=eps, scale=scale, single_pad=single)


def problem(case, weights="case"):
    """the case as tests/consis_ref64.py reads it: hs[l] the (B, Q, D) transposed views"""
    return dict(hs_v1=[b.transpose(1, 0, 2) for b in case["buf_v1"]], hs_v2=[b.transpose(1, 0, 2) for b in case["buf_v2"]],
                bid=case["bid"], idx=case["idx"], weights=case["weights"] if isinstance(weights, str) else weights,
                pad_size=case["pad_size"], scale=case["scale"], eps=case["eps"], upstream=case["upstream"])


def ordinary():
    """L = 6, B = 2, counts (3, 1): single_pad 3, pad 15, K = 20, Q = 15 + 8 + 10, D = 256; layer 4's loss is unused"""
    up = np.array([1.0, 0.5, 2.0, 0.75, 0.0, 1.25], F)
    return make(6, (3, 1), 18, 256, 11, upstream=up)


def small_ordinary():
    """the fixture's ordinary case: the same layout with two layers and one query past the pad"""
    return make(2, (3, 1), 1, 256, 12, upstream=np.array([1.0, 0.5], F))


def k1():
    c = make(2, (1,), 4, 256, 13, groups=1)
    assert len(c["bid"]) == 1
    return c


def k_odd():
    """K = 15: the last workgroup of a layer holds three rows"""
    return make(3, (2, 1), 2, 256, 14)


def k1500():
    """five groups of 300: 375 partial slots per layer, more than one per lane of the reducing wave"""
    return make(2, (180, 120), 7, 256, 15)


def d64():
    return make(2, (3, 1), 3, 64, 16)


def d36():
    """nine float4 chunks: the tail of the row loop, most lanes idle"""
    return make(2, (2, 2), 3, 36, 17)


def d1024():
    """four chunks per lane: the lane's running sum"""
    return make(1, (2, 1), 1, 1024, 18)


def image_weight_zero(L=2):
    """image 1 has weight 0 (the stand-in box of an image without pseudo boxes)"""
    c = make(L, (3, 2), 3, 256, 19, weights="ones")
    c["weights"] = np.where(c["bid"] == 1, F(0), F(1)).astype(F)
    return c


def below_eps(L=2):
    """selected rows of hs_v1 under the clamp: a zero row, a row of norm about 1e-13, a row whose squares flush to zero"""
    c = make(L, (3, 1), 3, 256, 20)
    for buf in c["buf_v1"]:
        buf[0, 0, :] = 0                                    # (b 0, q 0)
        buf[1, 0, :] = F(1e-13 / 16) * np.sign(buf[1, 0, :])
        buf[2, 0, :] = F(1e-25)
    return c


def exact_tie():
    """eps = 2^-40 and a selected row with the single non-zero element 2^-40: its square, the row sum and sqrtf are exact, so the
    norm EQUALS eps and torch's >= decides"""
    c = make(1, (2, 1), 2, 256, 21, eps=2.0 ** -40)
    c["buf_v1"][0][1, 0, :] = 0
    c["buf_v1"][0][1, 0, 7] = F(2.0 ** -40)
    return c


def out_of_range():
    """one pair points past the pad but inside the tensor"""
    c = make(2, (3, 1), 6, 256, 22)
    c["idx"][5] = c["pad_size"] + 2
    return c


def identical_views():
    c = make(2, (3, 1), 3, 256, 23)
    c["buf_v2"] = [b.copy() for b in c["buf_v1"]]
    return c


def uniform_weights():
    """all weights 1, the usual batch (every image has a pseudo box)"""
    return make(1, (2, 2), 1, 64, 24, weights="ones")


FIXTURE_CASES = dict(small_ordinary=small_ordinary, d64=d64, d36=d36, below_eps=lambda: below_eps(1),
                     image_weight_zero=lambda: image_weight_zero(1), uniform_weights=uniform_weights)
