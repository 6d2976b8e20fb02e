"""The selection primitives of csrc/select.h through two of their users.  With one class, semidetr_qsel_topk_f32 and
semidetr_det_decode_f32 are the same function of a logit vector: the k largest by (order_key descending, index ascending),
sorted.  Both are held against numpy.lexsort over a restatement of order_key, on inputs where the tie rule decides: four
distinct logit values, so the k-th key has hundreds of equals, some beyond the 8192-candidate chunk boundary of the decode,
plus +0 / -0, +-inf and NaNs of both signs."""
import ctypes
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
B = 2
CHUNK = 8192                       # candidates per workgroup of det_chunk_select_kernel
LEVELS = np.asarray([-1.5, -0.5, 0.5, 1.5], np.float32)
P = ctypes.c_void_p


def order_key(x):
    """csrc/select.h: the unsigned integer that orders like the float, NaN of either sign above +inf, -0 == +0."""
    bits = np.where(x == 0, 0, x.view(np.uint32)).astype(np.int64)
    key = np.where(bits & 0x80000000, ~bits & 0xFFFFFFFF, bits | 0x80000000)
    return np.where(np.isnan(x), 0xFFFFFFFF, key)


def expected(logits, k):
    key = order_key(logits)
    index = np.arange(logits.shape[1])
    return np.stack([np.lexsort((index, -row))[:k] for row in key])


def _specials():
    nan = np.asarray([0x7FC00000, 0xFFC00000, 0x7F800001, 0xFF800123], np.uint32).view(np.float32)      # +NaN, -NaN, payloads
    return np.concatenate([nan, np.asarray([0.0, -0.0, 0.0, np.inf, -np.inf, -0.0, np.inf, -np.inf, np.inf], np.float32)])


@functools.lru_cache(maxsize=None)
def inputs(n):
    """(B, n) logits of four values + the specials, never modified.  Row 0 holds extra entries of the top value, so a selection
    of 2048 ends inside the first chunk and leaves hundreds of equals behind on both sides of the boundary.  In row 1 the
    2048-th key in order is the fifth entry of the top value BEHIND the boundary: the selection has to take the first chunk's
    equals and exactly five of the second's, in index order."""
    rng = np.random.default_rng(n)
    x = LEVELS[rng.integers(0, 4, (B, n))]
    if n == 1:
        x[1, 0] = -0.0
        x.setflags(write=False)
        return x
    x[0, 4000:4400] = LEVELS[3]
    sp = _specials()
    for b in range(B):
        at = rng.choice(n - 48, len(sp) - 4, replace=False)                 # anywhere in the first chunk ...
        x[b, at] = sp[:-4]
        x[b, n - 40:n - 36] = sp[-4:]                                       # ... and -0, +inf, -inf, +inf in the second
        x[b, n - 30:n - 10] = LEVELS[3]
    top = (x[1] == LEVELS[3])
    above = int((order_key(x[1]) > order_key(LEVELS[3:])[0]).sum())
    first = np.flatnonzero(top[:CHUNK])
    assert len(first) > 2048 - above - 5 > 1000 and top[CHUNK:].sum() >= 20
    x[1, rng.choice(first, len(first) - (2048 - above - 5), replace=False)] = LEVELS[2]
    x.setflags(write=False)
    return x


def qsel(logits, k):
    import semi_detr_amd
    lib = semi_detr_amd._lib.lib()
    N, S = logits.shape
    lg = torch.from_numpy(logits.copy()).to(DEV)
    nbytes = lib.semidetr_qsel_topk_workspace_bytes(N, S)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=DEV)
    idx = torch.full((N, k), -7, dtype=torch.int64, device=DEV)
    inv = torch.full((N, S), -7, dtype=torch.int32, device=DEV)
    rc = lib.semidetr_qsel_topk_f32(P(torch.cuda.current_stream().cuda_stream), P(lg.data_ptr()), N, S, 1, k, P(ws.data_ptr()),
                                    nbytes, P(idx.data_ptr()), P(inv.data_ptr()))
    assert rc == 0, lib.semidetr_last_error()
    return idx.cpu().numpy(), inv.cpu().numpy()


def decode(logits, k):
    """Flat indices of the decode: the boxes carry the query number (cx = q / 16384, w = h = 0, W = 16384: x1 = q exactly)."""
    import semi_detr_amd
    lib = semi_detr_amd._lib.lib()
    N, Q = logits.shape
    lg = torch.from_numpy(logits.copy()).to(DEV)
    tag = torch.zeros(N, Q, 4, device=DEV)
    tag[..., 0] = torch.arange(Q, device=DEV, dtype=torch.float32) / 16384
    hw = torch.full((N, 2), 16384.0, device=DEV)
    nbytes = lib.semidetr_det_workspace_bytes(N, Q, 1, k)
    assert nbytes > 0
    ws = torch.full((nbytes // 8,), -1, dtype=torch.int64, device=DEV)
    dets = torch.full((N, k, 5), -7.0, device=DEV)
    labels = torch.full((N, k), -7, dtype=torch.int64, device=DEV)
    rc = lib.semidetr_det_decode_f32(P(torch.cuda.current_stream().cuda_stream), P(lg.data_ptr()), P(tag.data_ptr()),
                                     P(hw.data_ptr()), None, N, Q, 1, k, P(ws.data_ptr()), nbytes, P(dets.data_ptr()),
                                     P(labels.data_ptr()), None, None)
    assert rc == 0, lib.semidetr_last_error()
    assert not labels.any()
    return dets[..., 0].cpu().numpy().astype(np.int64)


def test_order_key_restatement():
    x = np.concatenate([_specials(), LEVELS, np.asarray([1e-45, -1e-45, 3.4e38, -3.4e38], np.float32)])
    key = order_key(x)
    fin = ~np.isnan(x)
    assert (key[~fin] == 0xFFFFFFFF).all() and (key[fin] < 0xFFFFFFFF).all()
    a, b = np.meshgrid(np.flatnonzero(fin), np.flatnonzero(fin))
    assert np.array_equal(key[a] < key[b], x[a] < x[b]) and np.array_equal(key[a] == key[b], x[a] == x[b])


@pytest.mark.parametrize("n,k", [(1, 1), (8240, 64), (8240, 2048)])
def test_query_select_and_decode_agree_with_the_total_order(n, k):
    x = inputs(n)
    want = expected(x, k)
    if n > 1:           # the tie rule decides: the k-th key has hundreds of equals inside and outside the selection
        key = order_key(x)
        kth = key[np.arange(B), want[:, -1]]
        equal = key == kth[:, None]
        taken = np.stack([np.isin(np.arange(n), w) for w in want])
        assert ((equal & taken).sum(1) >= 50).all() and ((equal & ~taken).sum(1) >= 15).all()
        if k == 2048:
            assert (equal & taken)[0, CHUNK:].sum() == 0 and (equal & ~taken)[0, :CHUNK].sum() >= 200
            assert (equal & taken)[1, CHUNK:].sum() == 5 and (equal & ~taken)[1, CHUNK:].sum() >= 15
    idx, inv = qsel(x, k)
    flat = decode(x, k)
    assert np.array_equal(idx, flat)
    assert np.array_equal(idx, want)
    want_inv = np.full((B, n), -1, np.int32)
    want_inv[np.arange(B)[:, None], want] = np.arange(k, dtype=np.int32)[None]
    assert np.array_equal(inv, want_inv)
