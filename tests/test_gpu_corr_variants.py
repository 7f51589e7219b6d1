"""The correlation / arg-max kernels of csrc/corr_argmax.hip in every launch variant and k-split plan, the window arg-max of
shift_sz > 1, and the two small neighbours (csrc/innercos.hip, the index kernel of csrc/mask_ops.hip), bit for bit against the CPU oracle.

Every case goes through the `ops` wrappers.  tests/corr_plan.py restates the launchers and holds the case tables;
tests/test_corr_plan.py proves without a GPU that the restatement gives the library's byte counts and that the tables reach every
row below, and each test here asserts its own row again (`P.check_case`) before it compares numbers.

  variant                                                                  selected at                                  case ids
  -----------------------------------------------------------------------  -------------------------------------------  ----------------------------------------
  corr_argmax_fast_kernel<false>                                           launch_corr_argmax                           fast_ring_exact, fast_ring_wraps, fast_kpw2_uneven
                                                                                                                        fast_kpw3_uneven, fast_kpw4_four_splits, layer_kpw2_in_consumer_merge
  corr_argmax_fast_kernel<true>                                            launch_corr_argmax                           fast_one_tile, fast_two_stages, fast_kpw2_even
                                                                                                                        win_p2
  corr_argmax_kernel<false>                                                launch_corr_argmax                           generic_n_ragged_negative, generic_kpw2_uneven, generic_kpw3_uneven
                                                                                                                        generic_kpw4
  corr_argmax_kernel<true>                                                 launch_corr_argmax                           generic_single, generic_tiny, generic_c_ragged_full_tiles
                                                                                                                        generic_kpw2_even, win_one_slice, win_two_slices_short_last
                                                                                                                        win_16_slices, win_batch_limited, win_empty_last_slice
  pack_bf16_k8_kernel                                                      launch_bf16                                  bf16_one_tile, bf16_kpw2_uneven, win_bf16_full_tiles
                                                                                                                        win_bf16_ragged
  corr_argmax_bf16_kernel<false,false>                                     launch_bf16 (launch_corr_argmax_bf16)        bf16_one_tile, bf16_kpw2_uneven
  corr_argmax_bf16_kernel<false,true>                                      launch_bf16 (launch_corr_R_bf16)             win_bf16_full_tiles
  corr_argmax_bf16_kernel<true,true>                                       launch_bf16 (launch_corr_R_bf16)             win_bf16_ragged
  window_corr_argmax_kernel                                                launch_window_corr_argmax                    win_one_slice, win_two_slices_short_last, win_p2
                                                                                                                        win_16_slices, win_batch_limited, win_empty_last_slice
                                                                                                                        win_bf16_full_tiles, win_bf16_ragged
  argmax_merge_kernel                                                      finish_argmax                                fast_kpw4_four_splits, generic_kpw2_even, bf16_kpw2_uneven
                                                                                                                        win_16_slices
  fast kernel: 1 / 2 LDS stages (fewer than the 3 in flight)               corr_argmax_fast_kernel: prologue            fast_one_tile, fast_two_stages
  fast kernel: 3 and 5 stages (at and past the 4-slot ring)                corr_argmax_fast_kernel: stage loop          fast_ring_exact, fast_ring_wraps
  fast kernel: kt_per_wg == 1                                              corr_plan                                    fast_one_tile, fast_two_stages, fast_ring_exact
                                                                                                                        fast_ring_wraps
  fast kernel: kt_per_wg >= 2, even last split                             corr_argmax_fast_kernel: kt_hi, k-tile loop  fast_kpw2_even, layer_kpw2_in_consumer_merge
  fast kernel: kt_per_wg >= 2, uneven last split                           corr_argmax_fast_kernel: kt_hi               fast_kpw2_uneven, fast_kpw3_uneven, fast_kpw4_four_splits
  generic kernel: kt_per_wg == 1                                           corr_plan                                    generic_single, generic_tiny, generic_c_ragged_full_tiles
                                                                                                                        generic_n_ragged_negative
  generic kernel: kt_per_wg >= 2, even last split                          corr_argmax_kernel: kt_hi, k-tile loop       generic_kpw2_even
  generic kernel: kt_per_wg >= 2, uneven last split                        corr_argmax_kernel: kt_hi                    generic_kpw2_uneven, generic_kpw3_uneven, generic_kpw4
  bf16 kernel: kt_per_wg >= 2, uneven last split                           corr_argmax_bf16_kernel: kt_hi, k-tile loop  bf16_kpw2_uneven
  in-consumer merge of the partials (merged_argmax)                        merged_argmax, forward_impl                  layer_kpw2_in_consumer_merge
  window plan: one slice                                                   window_plan                                  win_one_slice
  window plan: every slice sought is launched, short last one              window_plan                                  win_two_slices_short_last, win_p2, win_16_slices
                                                                                                                        win_batch_limited, win_bf16_full_tiles, win_bf16_ragged
  window plan: split limited by the batch (8 < 16 slices)                  window_plan                                  win_batch_limited
  window plan: 64 slices sought, 63 launched (none empty)                  window_plan                                  win_empty_last_slice
  innercos_fused_kernel: scalar path (N % 4 != 0)                          innercos_fused_kernel: `(N & 3) == 0` else   ic_scalar_small, ic_rpb2_ragged_scalar
  innercos_fused_kernel: vector path                                       innercos_fused_kernel: `(N & 3) == 0`        ic_vector_cx_wider, ic_rpb2_ragged_vector, ic_bwd_grid_stride
  innercos_fused_kernel: two launches, 2 rows per block, last block 1 row  launch_innercos_loss: rows per block         ic_rpb2_ragged_scalar, ic_rpb2_ragged_vector
  innercos_fused_kernel: one launch, 9 rows per block                      launch_innercos_loss: with a ticket          ic_rpb2_ragged_scalar, ic_rpb2_ragged_vector
  innercos_backward_kernel: Cx > Cuse (zero-filled channels)               innercos_backward_kernel: `c < Cuse`         ic_vector_cx_wider, ic_rpb2_ragged_scalar, ic_bwd_grid_stride
  innercos_backward_kernel: grid-stride loop (> 2048 x 256 elements)       innercos_backward_kernel: stride loop        ic_bwd_grid_stride
  index_prep_kernel: patch > 1, stride 2, threshold > 1                    mask_ops.hip:88-92, :118                     ip_p2_s1_t2, ip_p3_s2_t1, ip_p3_s1_t9
                                                                                                                        ip_p4_s2_t16, ip_p2_s2_t4, ip_40x40_p3_s1_t5
  index_prep_kernel: two 1024-chunks                                       mask_ops.hip:84                              ip_40x40_p3_s1_t5

The reference everywhere is `oracle.ipsr_oracle`, and every compared output is equal bit for bit: the fp32 matrix-core
instruction is one fmaf chain over ascending channels, which is what the oracle writes.  The bf16 cases (added so that every
reachable instantiation has one) run on small integers: bf16 holds them, every product and partial sum is an integer below 2^24, so
the bf16 matrix cores must give the oracle's fp32 bits as well.  The only tolerance is the InnerCos loss VALUE: kernel and oracle
form the same fp32 terms d*d (no contraction on either side) and add them in fp64 in different orders; for at most 2^22 non-negative
terms two fp64 sums differ by less than 2^-30 relative, and each is rounded once to fp32: the two are within 2 fp32 ulps.

Inputs are x = |randn| and ref = rand unless a case says otherwise ("negative": ref = -rand, every score below zero, so a zero pad
row of a ragged tile or a start value would win if it were let in).  The order-rule data set of four kt_per_wg >= 2 cases copies
patches 0 .. 31 to +32, +64, +128 (the next tile of the same workgroup) and +128 kt_per_wg (the other split), makes every third
reference column one of those patches (so the copies tie AT the maximum), and adds an all -inf, an all NaN and a single +inf
reference column and one NaN patch.
"""
import numpy as np
import pytest
import torch

import corr_plan as P
from oracle import ipsr_oracle as orc
from test_gpu_parity import assert_index_equal

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    from deepinpainting_amd import ops as _ops
    return _ops


def dev(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a))
    return (t.to(dtype) if dtype is not None else t).cuda()


def host(t):
    return t.cpu().numpy()


def _rs(cid, salt=0):
    return np.random.RandomState(sum(cid.encode()) * 131 + len(cid) + salt)


def _equal_with_nans(got, want, what):
    np.testing.assert_array_equal(np.isnan(got), np.isnan(want), err_msg=what)
    np.testing.assert_array_equal(got[~np.isnan(want)], want[~np.isnan(want)], err_msg=what)


# ---- fp32 correlation ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cid", list(P.CORR_CASES))
def test_fp32_correlation(ops, cid):
    """ops.patch_normalize -> ops.corr_argmax against the oracle's: xn, inv, ind, vmax and (where the table asks) S, bit for bit."""
    P.check_case(cid)
    (B, C, N), want_S, negative, _, _, _ = P.CORR_CASES[cid]
    rs = _rs(cid)
    x = np.abs(rs.standard_normal((B, C, N))).astype(np.float32)
    ref = rs.rand(B, C, N).astype(np.float32)
    if negative:
        ref = -ref
    xn_o, inv_o = orc.patch_normalize(x)
    ind_o, vmax_o, S_o = orc.corr_argmax(xn_o, ref, want_S=want_S)
    xn, inv = ops.patch_normalize(dev(x))
    np.testing.assert_array_equal(host(inv), inv_o)
    np.testing.assert_array_equal(host(xn), xn_o)
    ind, vmax, S = ops.corr_argmax(xn, dev(ref), want_S=want_S)
    ind, vmax = host(ind), host(vmax)
    assert ind.min() >= 0 and ind.max() < N
    if want_S:
        np.testing.assert_array_equal(host(S), S_o)
    np.testing.assert_array_equal(ind, ind_o)
    np.testing.assert_array_equal(vmax, vmax_o)
    if negative:
        assert (vmax_o < 0).all() and (vmax < 0).all()


ORDER_CASES = [cid for cid, case in P.CORR_CASES.items() if case[3]]


def order_rule_data(rs, B, C, N, kpw):
    """-> (xn, ref, the columns whose maximum is a tie between the copies of patch q % 32)."""
    far = 128 * kpw
    assert far + 96 <= N
    x = np.abs(rs.standard_normal((B, C, N))).astype(np.float32)
    x[:, :, 32:64] = x[:, :, :32]                  # the other MFMA tile of a wave (generic) / the other wave (fast)
    x[:, :, 64:96] = x[:, :, :32]                  # the other wave (generic) / the other MFMA tile of a wave (fast)
    x[:, :, 128:224] = x[:, :, :96]                # the next k-tile of the same workgroup
    x[:, :, far:far + 96] = x[:, :, :96]           # the first k-tile of the other split
    ref = rs.rand(B, C, N).astype(np.float32)
    cols = np.arange(0, N, 3)
    ref[:, :, cols] = x[:, :, cols % 32]           # <xn_k, x_j> is largest at k = j and at every copy of j
    xn = orc.patch_normalize(x)[0].copy()
    q_ninf, q_nan, q_inf = N - 1, N // 2 + 1, 70
    ref[:, :, q_ninf] = -np.inf
    ref[:, :, q_nan] = np.nan
    ref[:, 5, q_inf] = np.inf
    xn[0, 3, N - 3] = np.nan                       # sample 0 only: a NaN patch in the last k-tile wins every column it is first in
    return xn, ref, np.setdiff1d(cols, (q_ninf, q_nan, q_inf)), (q_ninf, q_nan, q_inf)


@pytest.mark.parametrize("cid", ORDER_CASES)
def test_fp32_correlation_order_rules(ops, cid):
    """Ties across MFMA tiles, waves, the k-tiles of one workgroup and the splits resolve to the lowest patch; -inf, +inf and NaN
    columns and a NaN patch give torch.max's answer (the recipe of test_argmax_is_total_on_nan_and_inf), in range."""
    plan = P.check_case(cid)
    B, C, N = P.CORR_CASES[cid][0]
    ks, kpw, _ = plan["split"]
    assert ks == 2 and kpw >= 2
    xn, ref, tie_cols, (q_ninf, q_nan, q_inf) = order_rule_data(_rs(cid, 1), B, C, N, kpw)
    ind_o, vmax_o, _ = orc.corr_argmax(xn, ref)
    # the data does what it is built for: in the samples without the NaN patch every tie column is won by the lowest of six copies
    np.testing.assert_array_equal(ind_o[1:, tie_cols], np.broadcast_to(tie_cols % 32, (B - 1, len(tie_cols))))
    assert (ind_o[1:, q_ninf] == 0).all() and (ind_o[1:, q_nan] == 0).all() and (vmax_o[1:, q_ninf] == -np.inf).all()
    assert np.isnan(vmax_o[0]).all() and (np.delete(ind_o[0], q_nan) == N - 3).all() and ind_o[0, q_nan] == 0
    ind, vmax, _ = ops.corr_argmax(dev(xn), dev(ref))
    ind, vmax = host(ind), host(vmax)
    assert ind.min() >= 0 and ind.max() < N
    np.testing.assert_array_equal(ind, ind_o)
    _equal_with_nans(vmax, vmax_o, cid)


@pytest.mark.parametrize("cid", list(P.BF16_CASES))
def test_bf16_correlation_on_integers(ops, cid):
    """ops.corr_argmax(corr="bf16") on integers in [0, 3] (sums <= 576): exact on the bf16 matrix cores, so equal to the oracle.
    Every patch occurs twice, so every maximum is a tie and the arg-max is the lower copy."""
    P.check_case(cid)
    B, C, N = P.BF16_CASES[cid][0]
    rs = _rs(cid)
    xi = rs.randint(0, 4, (B, C, N)).astype(np.float32)
    xi[:, :, N // 2:] = xi[:, :, :N // 2]          # every patch twice: half a tile (the other wave) or 1.5 tiles (the other split) apart
    ri = rs.randint(0, 4, (B, C, N)).astype(np.float32)
    ind_o, vmax_o, S_o = orc.corr_argmax(xi, ri, want_S=True)
    assert ((S_o == vmax_o[:, None, :]).sum(1) > 1).all() and ind_o.max() < N // 2     # (every maximum is attained more than once)
    ind, vmax, _ = ops.corr_argmax(dev(xi), dev(ri), corr="bf16")
    np.testing.assert_array_equal(host(ind), ind_o)
    np.testing.assert_array_equal(host(vmax), vmax_o)


# ---- the whole layer: the stage kernel folds the k-split partials itself -----------------------------------------------------------
def _hole(h, w, p=1, side=2):
    feat = np.zeros((h, w), np.uint8)
    feat[h // 2:h // 2 + side, w // 2:w // 2 + side] = 1
    return orc.index_prep(feat, patch=p).mask_point_idx


@pytest.mark.parametrize("cid", list(P.LAYER_CASES))
def test_layer_over_the_in_consumer_merge(ops, cid):
    P.check_case(cid)
    B, C, h, w = P.LAYER_CASES[cid][0]
    rs = _rs(cid)
    x = np.abs(rs.standard_normal((B, C, h, w))).astype(np.float32)
    ref = rs.rand(B, C, h, w).astype(np.float32)
    mpi = _hole(h, w, 1, 4)
    assert len(mpi) == 16
    fo = orc.forward(x, ref, mpi)
    f = ops.forward(dev(x), dev(ref), dev(mpi, torch.int32), want_attn=True)
    torch.cuda.synchronize()
    np.testing.assert_array_equal(host(f.ind), fo.ind)
    np.testing.assert_array_equal(host(f.vmax), fo.vmax)
    np.testing.assert_array_equal(host(f.out), fo.out)
    np.testing.assert_array_equal(host(f.attn_rows), fo.attn_rows)
    assert_index_equal(f.bwd_index, fo.bwd_index, h * w, len(mpi))


# ---- the window arg-max ----------------------------------------------------------------------------------------------------------------
WINDOW_RUNS = [(cid, "bf16 integers" if case[3] else "plain") for cid, case in P.WINDOW_CASES.items()] + [
    ("win_two_slices_short_last", "negative"), ("win_empty_last_slice", "negative"), ("win_16_slices", "constant block")]


@pytest.mark.parametrize("cid,data", WINDOW_RUNS, ids=["%s-%s" % (c, d.replace(" ", "_")) for c, d in WINDOW_RUNS])
def test_window_argmax(ops, cid, data):
    """ops.forward(patch = p) against orc.forward: ind, vmax and out.  "constant block": x is 1 over a 10 x 10 block, so the 64
    windows inside it are the same patch and tie; constant positive windows also correlate best with a positive reference, so the
    tie is at the maximum and the lowest window index must win."""
    plan = P.check_case(cid)
    (B, C, h, w, p), Np, _, bf16 = P.WINDOW_CASES[cid]
    rs = _rs(cid, len(data))
    if bf16:
        x = rs.randint(1, 4, (B, C, h, w)).astype(np.float32)
        ref = rs.randint(0, 4, (B, C, h, w)).astype(np.float32)
    else:
        x = np.abs(rs.standard_normal((B, C, h, w))).astype(np.float32)
        ref = rs.rand(B, C, h, w).astype(np.float32)
    if data == "negative":
        ref = -ref
    if data == "constant block":
        x[:, :, 5:15, 7:17] = 1.0
    mpi = _hole(h, w, p)
    assert 0 < len(mpi) <= 40
    fo = orc.forward(x, ref, mpi, patch=p)
    if data == "negative":
        assert (fo.vmax < 0).all()
    if data == "constant block":
        nW = w - p + 1
        same = np.array([y * nW + xx for y in range(5, 13) for xx in range(7, 15)])
        won = np.isin(fo.ind, same)
        assert won.mean() > 0.2 and (fo.ind[won] == same[0]).all()         # the tie is at the maximum of many columns
    f = ops.forward(dev(x), dev(ref), dev(mpi, torch.int32), patch=p, want_attn=True, corr="bf16" if bf16 else "fp32")
    torch.cuda.synchronize()
    ind = host(f.ind)
    assert ind.min() >= 0 and ind.max() < Np == plan["Np"]
    np.testing.assert_array_equal(ind, fo.ind)
    np.testing.assert_array_equal(host(f.vmax), fo.vmax)
    np.testing.assert_array_equal(host(f.out), fo.out)


# ---- InnerCos ----------------------------------------------------------------------------------------------------------------------------
def _within_2_ulps(a, b):
    return abs(float(a) - float(b)) <= 2 * float(np.spacing(np.float32(b)))


@pytest.mark.parametrize("cid", list(P.IC_CASES))
def test_innercos(ops, cid):
    """The loss in two launches and in one (three calls in a row: the arrival counter must return to zero) within 2 fp32 ulps of the
    oracle's (the module docstring derives the bound); the gradient bit for bit, its channels past Cuse zero."""
    P.check_case(cid)
    B, Cx, Cuse, h, w = P.IC_CASES[cid][0]
    assert B * Cuse * h * w <= 2 ** 22
    rs = _rs(cid)
    x = rs.standard_normal((B, Cx, h, w)).astype(np.float32)
    t = rs.rand(B, Cuse, h, w).astype(np.float32)
    m = (rs.rand(h, w) < 0.6).astype(np.float32)
    strength = 1.3
    want = orc.innercos_loss(x, m, t, strength)
    xd, td, md = dev(x), dev(t), dev(m.reshape(-1))
    loss = ops.innercos_loss(xd, Cuse, md, td, strength).item()
    print("%s: loss %.9g oracle %.9g (%.2f ulps)" % (cid, loss, want, abs(loss - float(want)) / float(np.spacing(np.float32(want)))))
    assert _within_2_ulps(loss, want), (loss, want)
    for i in range(3):
        one = ops.innercos_loss(xd, Cuse, md, td, strength, one_launch=True).item()
        assert _within_2_ulps(one, want), (i, one, want)
    g = host(ops.innercos_loss_backward(xd, Cuse, md, td, strength, torch.full((), 0.37, device="cuda")))
    np.testing.assert_array_equal(g, orc.innercos_loss_backward(x, m, t, strength, 0.37))
    assert not g[:, Cuse:].any() and g[:, :Cuse].any()


# ---- index_prep --------------------------------------------------------------------------------------------------------------------------
def test_index_prep_strides_and_thresholds(ops):
    """`ipsr_index_prep` beyond (patch, 1, 1): one 13 x 17 mask at density 0.4 under six (patch, stride, threshold) triples and a
    40 x 40 one whose 1444 windows take two 1024-chunks.  Two triples flag nothing (M = 0): every index is then -1."""
    masks = {(13, 17): (np.random.RandomState(1317).rand(13, 17) < 0.4).astype(np.uint8),
             (40, 40): (np.random.RandomState(4040).rand(40, 40) < 0.4).astype(np.uint8)}
    counts = []
    for cid, (hw, (patch, stride, thr), _) in P.INDEX_PREP_CASES.items():
        plan = P.check_case(cid)
        feat = masks[hw]
        ip = orc.index_prep(feat, patch, stride, thr)
        flag, mpi, cnt = ops.index_prep(dev(feat), patch, stride, thr)
        M = int(cnt.item())
        counts.append(M)
        assert M == len(ip.mask_point_idx) == int(ip.flag.sum()), cid
        np.testing.assert_array_equal(host(flag), ip.flag, err_msg=cid)
        np.testing.assert_array_equal(host(mpi)[:M], ip.mask_point_idx, err_msg=cid)
        assert (host(mpi)[M:] == -1).all(), cid
        if plan["chunks"] == 2:
            assert ip.mask_point_idx.min() < 1024 <= ip.mask_point_idx.max(), cid     # flagged windows in both chunks
    assert counts.count(0) == 2, counts


def test_every_variant_is_reached():
    """From the restatement: the case tables above cover every entry of REACHABLE, every (kt_per_wg 1 | >= 2 even | >= 2 uneven) x
    (fast | generic) combination, both outcomes of the window plan and every row of the docstring's table."""
    import test_corr_plan as host_checks
    host_checks.test_the_tables_reach_every_variant_and_edge()
    for variant, _, cases in P.REACHABLE:
        assert cases and all(variant in P.case_plan(c)["kernels"] for c in cases), variant
    for variant, _, pred, cases in P.EDGES:
        assert cases and all(pred(P.case_plan(c)) for c in cases), variant
    ran = set(P.CORR_CASES) | set(P.BF16_CASES) | set(P.LAYER_CASES) | {c for c, _ in WINDOW_RUNS} | set(P.IC_CASES) | set(P.INDEX_PREP_CASES)
    assert ran == set(P.ALL_CASE_IDS)
