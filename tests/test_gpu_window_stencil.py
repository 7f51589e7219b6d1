"""The LDS-tiled window stencil (csrc/window_stencil.hip) against the streaming kernel it stands in for and against the CPU oracle.

`ipsr_debug_set_option(8, v)` chooses the kernel behind the window arg-max of a shift_sz > 1 forward: 1 = the streaming kernel
everywhere, 2 = the LDS-tiled kernel wherever its envelope allows.  Every case first asks `ops.window_corr_plan` that option 2
really reaches the tiled kernel (or, for the fallback case, really does not), then runs `ops.forward(..., want_attn=True)` under
both options: `ind`, `vmax`, `out` and the attention rows are equal bit for bit, and equal to `oracle.ipsr_oracle.forward`
(the sparse index too).  Nothing here has a tolerance: both kernels form every correlation by the same fp32 expressions in the same
order, and the arg-max order (larger value, NaN above everything, lower index on ties) is total, so the partition of the candidates
over threads and k-row ranges cannot show.

The shapes (tests/window_stencil_plan.py: GPU_CASES) are the smallest at which the kernel takes each of its paths.  The order-rule
data runs on the shape whose candidates are split over threads, waves AND k-row ranges.  There the oracle comparison is `ind` and
`vmax`, what the stencil produces (and `out` / the attention rows where the data is finite); all four are compared bit for bit
between the two kernels.  The NaN / inf data runs with an empty mask: a NaN window wins every column, the recurrence over masked
positions is not defined on NaN weights, and the oracle does not survive it.  `wider_than_a_wave` is also the case with one LDS
buffer (its blocks are too large for two workgroups of two buffers per CU); the others run on two.
"""
import numpy as np
import pytest
import torch

import window_stencil_plan as W
from oracle import ipsr_oracle as orc
from test_gpu_parity import assert_index_equal

pytestmark = pytest.mark.gpu

OPTION = 8
ORDER_SHAPE = W.GPU_CASES["many_per_thread_split"]


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    from deepinpainting_amd import ops as _ops
    yield _ops
    set_option(0)


def set_option(v):
    from deepinpainting_amd import _lib
    _lib.check(_lib.lib().ipsr_debug_set_option(OPTION, v), "ipsr_debug_set_option")


def dev(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a))
    return (t.to(dtype) if dtype is not None else t).cuda()


def host(t):
    return t.cpu().numpy()


def bits(t):
    return t.contiguous().view(torch.int32)


def hole(h, w, p):
    feat = np.zeros((h, w), np.uint8)
    feat[h // 2:h // 2 + 2, w // 2:w // 2 + 2] = 1
    mpi = orc.index_prep(feat, patch=p).mask_point_idx
    assert len(mpi) > 0
    return mpi


def both_kernels(ops, shape, x, ref, mpi, expect=W.LDS_TILED, **kw):
    """-> (forward under option 1, forward under option 2), after checking through the query which kernel option 2 reaches."""
    B, _, h, w, p = shape
    runs = {}
    try:
        for v in (1, 2):
            set_option(v)
            plan = ops.window_corr_plan(B, h, w, p)
            assert plan["variant"] == (expect if v == 2 else W.STREAMING), (shape, v, plan)
            assert plan == W.plan(B, h, w, p, v)
            runs[v] = ops.forward(dev(x), dev(ref), mpi, patch=p, want_attn=True, **kw)
            torch.cuda.synchronize()
    finally:
        set_option(0)
    a, b = runs[1], runs[2]
    for name in ("ind", "vmax", "out", "attn_rows"):
        s, t = getattr(a, name), getattr(b, name)
        assert s.shape == t.shape and torch.equal(bits(s), bits(t)), "%s: %s differs between the streaming and the LDS-tiled kernel" % (shape, name)
    return a, b


def equal_with_nans(got, want, what):
    np.testing.assert_array_equal(np.isnan(got), np.isnan(want), err_msg=what)
    np.testing.assert_array_equal(got[~np.isnan(want)], want[~np.isnan(want)], err_msg=what)


def assert_equals_oracle(f, fo, shape, M):
    B, _, h, w, p = shape
    Np = (h - p + 1) * (w - p + 1)
    ind = host(f.ind)
    assert ind.min() >= 0 and ind.max() < Np
    np.testing.assert_array_equal(ind, fo.ind)
    np.testing.assert_array_equal(host(f.vmax), fo.vmax)
    np.testing.assert_array_equal(host(f.out), fo.out)
    np.testing.assert_array_equal(host(f.attn_rows), fo.attn_rows)
    assert_index_equal(f.bwd_index, fo.bwd_index, Np, M)


def features(shape, seed):
    B, C, h, w, _ = shape
    rs = np.random.RandomState(seed)
    return np.abs(rs.standard_normal((B, C, h, w))).astype(np.float32), rs.rand(B, C, h, w).astype(np.float32)


@pytest.mark.parametrize("cid", list(W.GPU_CASES))
def test_tiled_equals_streaming_and_oracle(ops, cid):
    shape = W.GPU_CASES[cid]
    B, C, h, w, p = shape
    x, ref = features(shape, sum(shape))
    mpi = hole(h, w, p)
    _, f = both_kernels(ops, shape, x, ref, dev(mpi, torch.int32))
    assert_equals_oracle(f, orc.forward(x, ref, mpi, patch=p), shape, len(mpi))


def test_outside_the_envelope_the_streaming_kernel_runs(ops):
    shape = W.FALLBACK_CASE
    B, C, h, w, p = shape
    x, ref = features(shape, 120)
    mpi = hole(h, w, p)
    _, f = both_kernels(ops, shape, x, ref, dev(mpi, torch.int32), expect=W.STREAMING)
    assert_equals_oracle(f, orc.forward(x, ref, mpi, patch=p), shape, len(mpi))


def test_the_plan_of_the_cases(ops):
    """The split > 1 case and the no-merge case are what their names say, under the option the other tests use."""
    try:
        set_option(2)
        plans = {cid: ops.window_corr_plan(B, h, w, p) for cid, (B, _, h, w, p) in W.GPU_CASES.items()}
    finally:
        set_option(0)
    assert plans["many_per_thread_split"]["split"] > 1 and plans["one_range_no_merge"]["split"] == 1


# ---- the order rule -------------------------------------------------------------------------------------------------------------------
def order_data(kind):
    B, C, h, w, p = ORDER_SHAPE
    rs = np.random.RandomState(len(kind) * 977 + 5)
    if kind == "integers":                    # exact sums; the right half repeats the left, so every window has a twin: real ties
        x = rs.randint(0, 4, (B, C, h, w)).astype(np.float32)
        x[:, :, :, w // 2:w // 2 + w // 2] = x[:, :, :, :w // 2]
        ref = rs.randint(0, 4, (B, C, h, w)).astype(np.float32)
    elif kind == "constant":                  # every window is the same patch: every column is one tie over all k'
        x = np.ones((B, C, h, w), np.float32)
        ref = rs.rand(B, C, h, w).astype(np.float32)
    elif kind == "nan_inf":                   # windows over the planted positions score NaN (or +-inf) in every column
        x, ref = features(ORDER_SHAPE, 3)
        x[0, 3, h - 4, w - 5] = np.nan
        x[0, 1, 10, 11] = np.inf
        x[0, 2, 20, 6] = -np.inf
    elif kind == "ninf_columns":              # a -inf reference position: every window over it is a -inf column
        x, ref = features(ORDER_SHAPE, 4)
        x += 0.125                            # strictly positive: no 0 * inf
        ref[0, :, 7, 9] = -np.inf
        ref[0, :, 30, 2] = -np.inf
    else:
        raise ValueError(kind)
    return x, ref


@pytest.mark.parametrize("kind", ["integers", "constant", "nan_inf", "ninf_columns"])
def test_order_rule(ops, kind):
    shape = ORDER_SHAPE
    B, C, h, w, p = shape
    nW = w - p + 1
    x, ref = order_data(kind)
    # "nan_inf": every column's winner is a NaN window, and the recurrence over masked positions is not defined on NaN weights (the
    # oracle does not survive it): that layer runs with an empty mask, which leaves the arg-max and the gather by it
    mpi = hole(h, w, p) if kind != "nan_inf" else np.zeros(0, np.int64)
    fo = orc.forward(x, ref, mpi, patch=p)
    if kind == "constant":
        assert (fo.ind == 0).all()
    if kind == "ninf_columns":
        cols = [qy * nW + qx for (py, px) in ((7, 9), (30, 2)) for qy in range(max(0, py - p + 1), min(h - p, py) + 1)
                for qx in range(max(0, px - p + 1), min(nW - 1, px) + 1)]
        assert len(cols) == 2 * p * p and (fo.vmax[0, cols] == -np.inf).all() and (fo.ind[0, cols] == 0).all()
    if kind == "nan_inf":
        # a window over a planted position scores NaN in every column (inf * 0 for the infinities): the first of them wins everywhere
        first = min((py - p + 1) * nW + px - p + 1 for py, px in ((h - 4, w - 5), (10, 11), (20, 6)))
        assert np.isnan(fo.vmax).all() and (fo.ind == first).all()
    _, f = both_kernels(ops, shape, x, ref, dev(mpi, torch.int32))
    ind = host(f.ind)
    assert ind.min() >= 0 and ind.max() < (h - p + 1) * nW
    np.testing.assert_array_equal(ind, fo.ind)
    equal_with_nans(host(f.vmax), fo.vmax, kind)
    if kind in ("integers", "constant"):
        np.testing.assert_array_equal(host(f.out), fo.out)
        np.testing.assert_array_equal(host(f.attn_rows), fo.attn_rows)


# ---- the other two forward entries ----------------------------------------------------------------------------------------------------
def test_per_sample_mask_entry(ops):
    """ipsr_forward_masks: one shared index and full counts, so the oracle's plain forward is the reference."""
    shape = W.GPU_CASES["batch"]
    B, C, h, w, p = shape
    x, ref = features(shape, 77)
    mpi = hole(h, w, p)
    counts = torch.full((B,), len(mpi), dtype=torch.int32).cuda()
    _, f = both_kernels(ops, shape, x, ref, dev(mpi, torch.int32), counts=counts)
    assert_equals_oracle(f, orc.forward(x, ref, mpi, patch=p), shape, len(mpi))


def test_bf16_correlation_entry(ops):
    """ipsr_forward_bf16corr on integers in [0, 3] (sums <= 9 * 64 * 9): exact on the bf16 matrix cores, so equal to the fp32 oracle."""
    shape = (1, 64, 6, 6, 3)
    B, C, h, w, p = shape
    rs = np.random.RandomState(64)
    x = rs.randint(0, 4, (B, C, h, w)).astype(np.float32)
    ref = rs.randint(0, 4, (B, C, h, w)).astype(np.float32)
    mpi = hole(h, w, p)
    _, f = both_kernels(ops, shape, x, ref, dev(mpi, torch.int32), corr="bf16")
    assert_equals_oracle(f, orc.forward(x, ref, mpi, patch=p), shape, len(mpi))
