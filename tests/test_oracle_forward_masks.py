"""oracle.forward_masks, the Python-only twin of ipsr_forward_masks: the capacity layout assembled from batch-of-one `forward` calls.

CPU only.  The layout is checked three ways on a p = 1 and a p = 3 shape (signed features, so that the survivor half of the index is
not empty): with every count at the capacity it IS `forward` on the batch; with mixed counts every sample is its batch-of-one
`forward`, zero rows and sentinel slots around it; and the C backward reads the capacity layout with M = Mcap to the batch-of-one
gradient.
"""
import numpy as np
import pytest

from oracle import ipsr_oracle as orc
from test_gpu_parity import used_index, used_index_cap

SHAPES = [
    # id,       B, C,  h, w, p, Mcap, mixed counts
    ("p1_6x7",  4, 12, 6, 7, 1, 9,    [0, 9, 4, 1]),
    ("p3_7x8",  3, 5,  7, 8, 3, 7,    [7, 0, 3]),
]


def _inputs(B, C, h, w, p, Mcap, seed):
    rs = np.random.RandomState(seed)
    Np = (h - p + 1) * (w - p + 1)
    x = rs.standard_normal((B, C, h, w)).astype(np.float32)
    ref = rs.standard_normal((B, C, h, w)).astype(np.float32)
    g = rs.standard_normal((B, C, h, w)).astype(np.float32)
    rows = np.stack([np.sort(rs.choice(Np, Mcap, replace=False)) for _ in range(B)]).astype(np.int32)
    return x, ref, g, rows, Np


def _backward(g, M, bidx, tw, p):
    return orc.backward_patch(g, M, bidx, tw, p)


@pytest.mark.parametrize("B,C,h,w,p,Mcap,mixed", [s[1:] for s in SHAPES], ids=[s[0] for s in SHAPES])
def test_full_counts_are_forward_on_the_batch(B, C, h, w, p, Mcap, mixed):
    x, ref, g, rows, Np = _inputs(B, C, h, w, p, Mcap, seed=Mcap)
    shared = rows[0]
    fo = orc.forward(x, ref, shared, patch=p)
    for mpi in (shared, np.broadcast_to(shared, (B, Mcap)).copy()):                 # the shared form and one row per sample
        fm = orc.forward_masks(x, ref, mpi, np.full(B, Mcap), Mcap, patch=p)
        for a, b in zip(fm[:4], fo[:4]):
            assert a.dtype == b.dtype and a.shape == b.shape
            np.testing.assert_array_equal(a, b)
        assert fm.bwd_index.shape == fo.bwd_index.shape
        want = used_index(fo.bwd_index, Np, Mcap)
        assert sum(int(u[2 * Np + 1 - Mcap + Np]) for u in want) > 0, "the shape should have truncation survivors"
        for a, b in zip(used_index_cap(fm.bwd_index, Np, [Mcap] * B, Mcap), want):
            np.testing.assert_array_equal(a, b)
        np.testing.assert_array_equal(_backward(g, Mcap, fm.bwd_index, 0.75, p), _backward(g, Mcap, fo.bwd_index, 0.75, p))


@pytest.mark.parametrize("B,C,h,w,p,Mcap,mixed", [s[1:] for s in SHAPES], ids=[s[0] for s in SHAPES])
def test_mixed_counts_are_batch_of_one_forwards(B, C, h, w, p, Mcap, mixed):
    x, ref, g, rows, Np = _inputs(B, C, h, w, p, Mcap, seed=Mcap + 1)
    assert 0 in mixed and Mcap in mixed
    counts = np.asarray(mixed)
    fm = orc.forward_masks(x, ref, rows, counts, Mcap, patch=p)
    assert fm.attn_rows.shape == (B, Mcap, Np) and fm.bwd_index.shape == (B, orc.bwd_index_ints(Np, Mcap))
    gin = _backward(g, Mcap, fm.bwd_index, 0.5, p)
    used = used_index_cap(fm.bwd_index, Np, counts, Mcap)
    capB = Mcap * (Mcap + 1) // 2
    for b, m in enumerate(mixed):
        f1 = orc.forward(x[b:b + 1], ref[b:b + 1], rows[b, :m], patch=p)
        np.testing.assert_array_equal(fm.out[b], f1.out[0])
        np.testing.assert_array_equal(fm.ind[b], f1.ind[0])
        np.testing.assert_array_equal(fm.vmax[b], f1.vmax[0])
        np.testing.assert_array_equal(fm.attn_rows[b, :m], f1.attn_rows[0])
        assert not fm.attn_rows[b, m:].any()
        np.testing.assert_array_equal(used[b], used_index(f1.bwd_index, Np, m)[0])
        # everything outside the used part is the sentinel
        nb = int(fm.bwd_index[b, 3 * Np + 1])
        assert (fm.bwd_index[b] == orc.INDEX_SENTINEL).sum() == m + 2 * (capB - nb)
        np.testing.assert_array_equal(gin[b], _backward(g[b:b + 1], m, f1.bwd_index, 0.5, p)[0])
        if p == 1:
            np.testing.assert_array_equal(gin[b], orc.backward(g[b:b + 1], rows[b, :m], f1.attn_rows, f1.bwd_index, 0.5)[0])
    # the same through `backward` (p = 1 only): M is the length of the index it is handed, i.e. the capacity
    if p == 1:
        np.testing.assert_array_equal(orc.backward(g, rows[0], fm.attn_rows, fm.bwd_index, 0.5), gin)
    # counts outside [0, Mcap] are clamped, and a shared index row serves every sample
    over = orc.forward_masks(x, ref, rows, counts + (counts == Mcap) * 5 - (counts == 0) * 3, Mcap, patch=p)
    for a, b in zip(over, fm):
        np.testing.assert_array_equal(a, b)
    sh = orc.forward_masks(x, ref, rows[0], counts, Mcap, patch=p, want_attn=False)
    assert sh.attn_rows is None
    for b, m in enumerate(mixed):
        np.testing.assert_array_equal(sh.out[b], orc.forward(x[b:b + 1], ref[b:b + 1], rows[0, :m], patch=p).out[0])
