"""The IPSR layer through ipsr_forward_masks — a padded device index of capacity Mcap and one device count per sample, the entry
the trainer uses (models/IPSR_model.py) — in every launch variant, with counts below the capacity, bit for bit against
oracle.forward_masks.

The host-M entry (test_gpu_layer_limits.py, test_gpu_corr_variants.py, test_gpu_parity.py) always runs with capacity == count.
Here the LDS carves, row strides and the bwd_index layout are sized by the capacity while each sample walks its own count, so the
kernels take the branches listed below.  Every case computes the variant it claims from the launcher's own formula (the
restatements of test_gpu_layer_limits.py) and asserts it before comparing numbers; data-dependent quantities (survivors, long
columns, active columns) are read back from the result.  `gin` comes from ops.backward with M = Mcap.

  row                       what (attention.hip unless said)                                     case id(s)
  ------------------------  -------------------------------------------------------------------  ------------------------------------
  stage_1_partial           attention_stage_kernel<1,partial>, ring body, counts 0..17           rec_c16
  stage_1_full              <1,full> (Cp 512)                                                    rec_c512 (and trainer_shared_index)
  stage_2_full              <2,full> (Cp 1024)                                                   rec_c1024
  stage_3_full              <3,full> (Cp 1536)                                                   rec_c384_p2
  stage_3_partial           <3,partial> (Cp 1176)                                                rec_c130_p3
  stage_4_full              <4,full> (Cp 2048)                                                   rec_c512_p2
  stage_8                   <8> (Cp 2304)                                                        rec_c256_p3
  stage_12                  <12> (Cp 4608)                                                       rec_c512_p3
  stage_16                  <16> (Cp 6912)                                                       rec_c768_p3
  stage_16_ceiling          <16> at Cp 8192, the largest patch admitted                          rec_c2048_p2
  ring_tails                recurrence_body: 0, 1, 2 paired trips; TURN+TAIL and bare-TAIL       rec_c16, rec_c512, rec_c1024,
                            exits, each with a tail of 0..3 steps; a sample with nothing masked  rec_c384_p2, rec_c130_p3
  wide_tails                recurrence_wide_body: odd and even step counts, count 0              rec_c512_p2
  quad_tails                recurrence_quad_body: 0, 1, 2 turns of QD = 4 with every tail        rec_c256_p3, rec_c512_p3, rec_c768_p3,
                                                                                                 rec_c2048_p2
  mce_zero                  attn_compress_kernel: no active column, offj[0] patched to 0         compress_capacity
  mce_exact_below_mc        Mce == mprime, a multiple of 32 below Mc (the offj[Mce] patch)       compress_capacity
  mce_rounded_below_mc      Mce rounded up past mprime, below Mc                                 compress_capacity
  mce_equals_mc             Mce == Mc                                                            compress_capacity
  mce_loop_below_mc         > AC_MAXT columns, Mce < Mc: running total offj[Mc] -> offj[Mce]     compress_capacity
  compress_loops            the > 1024-column loop: one, two and three passes in one launch      compress_capacity
  lds_above_48k             stage ring and compress LDS > 48 KiB, sized by the capacity          compress_capacity
  recon_block_edges         recon_masked_kernel: 64-row blocks empty, exactly full, one row      compress_capacity
                            over; attn_expand_kernel zero rows
  bw_r8_staged              ipsr_backward_kernel<8,staged>, capB from the capacity (backward.hip) bwcap_r8_staged
  bw_r4_staged              <4,staged>                                                           bwcap_r4_staged
  bw_r2_staged              <2,staged>                                                           bwcap_r2_staged
  bw_r2_unstaged            <2,unstaged>                                                         bwcap_r2_unstaged
  bw_r1_staged              <1,staged>                                                           bwcap_r1_staged
  bw_r1_unstaged            <1,unstaged>                                                         bwcap_r1_unstaged, limit_cap6388
  bw_survivors_beyond_bcap  staged, survivors > bcap read from L2                                bwcap_survivors_beyond_bcap
  bw_over_maxlong           more than BW_MAXLONG = 512 long columns                              bwcap_over_maxlong
  shared_index              mpi_stride = 0, Mcap = N, index straight from index_prep (-1 tail)   trainer_shared_index
  per_row_index             mpi_stride = Mcap                                                    trainer_per_row_index + all others
  clamps                    counts > Mcap and < 0 clamp; entries past the count are never read   clamp_counts, unread_tail
  bf16_corr                 corr_bf16 with per-sample counts at p = 1                            bf16_counts
  limit                     N 9600, Mcap 6388: stage LDS exactly 150 KiB, judged by capacity     limit_cap6388
  refusals                  Mcap 6389 / N 9604 / C p^2 8196 refused before the first launch      refuse_cap6389, refuse_n9604,
                                                                                                 refuse_cp8196

compress_capacity asks for the dense attn_rows in a second call restricted to four samples (counts 0, 33, 1025, 2100): eleven
samples of 2100 x 2304 rows are 200 MB to move and compare for no further branch.
"""
import ctypes

import numpy as np
import pytest
import torch

import corr_plan as P
from guarded import Arena
from oracle import ipsr_oracle as orc
from test_gpu_layer_limits import (IPSR_ERR_UNSUPPORTED, KIB, BW_CASES, _nan_fill, active_columns, bw_variant, compress_lds, index_counts,
                                   inputs, proto_inputs, stage_lds, stage_variant)
from test_gpu_parity import stroke_mask, used_index, used_index_cap

pytestmark = pytest.mark.gpu

RING, QD, AC_MAXT, RM_BL = 4, 4, 1024, 64           # attention.hip:63, :303, :580, :707


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    from deepinpainting_amd import ops as _ops
    return _ops


def dev(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a))
    return (t.to(dtype) if dtype is not None else t).cuda()


def assert_index_cap_equal(a, b, N, counts, Mcap):
    for u, v in zip(used_index_cap(a, N, counts, Mcap), used_index_cap(b, N, counts, Mcap)):
        np.testing.assert_array_equal(u, v)


def run_and_compare(ops, x, ref, rows, counts, Mcap, g, tw, patch=1, want_attn=True, fo=None):
    """HIP ipsr_forward_masks + backward vs oracle.forward_masks (`fo` if the caller has it already), everything bit for bit.
    Returns (HIP forward, oracle forward)."""
    B, C, h, w = x.shape
    Np = (h - patch + 1) * (w - patch + 1)
    counts = np.asarray(counts, np.int32)
    if fo is None:
        fo = orc.forward_masks(x, ref, rows, counts, Mcap, patch=patch, want_attn=want_attn)
    gin_o = orc.backward_patch(g, Mcap, fo.bwd_index, tw, patch)
    f = ops.forward(dev(x), dev(ref), dev(rows, torch.int32), patch=patch, want_attn=want_attn, counts=dev(counts))
    gin = ops.backward(dev(g), f.bwd_index, tw, Mcap, patch=patch)
    torch.cuda.synchronize()
    np.testing.assert_array_equal(f.ind.cpu().numpy(), fo.ind)
    np.testing.assert_array_equal(f.vmax.cpu().numpy(), fo.vmax)
    np.testing.assert_array_equal(f.out.cpu().numpy(), fo.out)
    if want_attn:
        np.testing.assert_array_equal(f.attn_rows.cpu().numpy(), fo.attn_rows)
    assert_index_cap_equal(f.bwd_index, fo.bwd_index, Np, counts, Mcap)
    np.testing.assert_array_equal(gin.cpu().numpy(), gin_o)
    return f, fo


def index_rows(rs, B, Np, Mcap):
    """One sorted random subset of the window grid per sample; its first counts[b] entries are the live ones."""
    return np.stack([np.sort(rs.choice(Np, Mcap, replace=False)) for _ in range(B)]).astype(np.int32)


# ---- A. the recurrence bodies, every tail branch ----------------------------------------------------------------------------------
REC_CASES = [
    # id,             C,    h, w, p, instantiation
    ("rec_c16",       16,   8, 8, 1, "<1,partial>"),
    ("rec_c512",      512,  8, 8, 1, "<1,full>"),
    ("rec_c1024",     1024, 8, 8, 1, "<2,full>"),
    ("rec_c384_p2",   384,  7, 9, 2, "<3,full>"),
    ("rec_c130_p3",   130,  8, 8, 3, "<3,partial>"),
    ("rec_c512_p2",   512,  8, 7, 2, "<4,full>"),
    ("rec_c256_p3",   256,  8, 9, 3, "<8>"),
    ("rec_c512_p3",   512,  7, 8, 3, "<12>"),
    ("rec_c768_p3",   768,  8, 8, 3, "<16>"),
    ("rec_c2048_p2",  2048, 5, 6, 2, "<16>"),
]


def rec_body(Cp):
    """attention.hip:568-570: which recurrence body the instantiation runs."""
    nch = -(-Cp // 512)
    return "quad" if nch > 4 else "wide" if nch > 3 else "ring"


def rec_counts(Cp):
    """The issue's count sets: 0..17 for the ring of 4 with two register sets, 0..12 for the wide and quad bodies."""
    return list(range(18)) if rec_body(Cp) == "ring" else list(range(13))


def tail_branches(body, counts):
    """The exits of the step loop that a set of per-sample counts reaches (steps = count - 1)."""
    got = set()
    for m in counts:
        if m <= 0:
            got.add("no_recurrence")                                # attention.hip:567
            continue
        n = m - 1
        if body == "ring":                                          # :236-246
            nfull = n // RING
            got.add(("paired_trips", min(nfull // 2, 2)))
            got.add(("turn+tail" if nfull % 2 else "tail", n % RING))
        elif body == "wide":                                        # :277-291
            got.add("odd" if n % 2 else "even")
        else:                                                       # :379-396
            got.add(("turns", n // QD))
            got.add(("tail", n % QD))
    return got


WANT_TAILS = {
    "ring": {"no_recurrence"} | {("paired_trips", t) for t in range(3)} | {(e, t) for e in ("turn+tail", "tail") for t in range(RING)},
    "wide": {"no_recurrence", "odd", "even"},
    "quad": {"no_recurrence"} | {("turns", t) for t in range(3)} | {("tail", t) for t in range(QD)},
}


@pytest.mark.parametrize("C,h,w,p,want", [c[1:] for c in REC_CASES], ids=[c[0] for c in REC_CASES])
def test_recurrence_bodies_every_tail_in_one_call(ops, C, h, w, p, want):
    Cp = (C * p * p + 7) & ~7
    assert stage_variant(Cp) == want
    body = rec_body(Cp)
    rs = np.random.RandomState(Cp + h)
    counts = rs.permutation(rec_counts(Cp)).astype(np.int32)
    assert tail_branches(body, counts) == WANT_TAILS[body]
    B, Mcap = len(counts), int(counts.max())
    Np = (h - p + 1) * (w - p + 1)
    assert Mcap <= Np
    x = np.abs(rs.standard_normal((B, C, h, w))).astype(np.float32)
    ref = rs.rand(B, C, h, w).astype(np.float32)
    g = rs.standard_normal((B, C, h, w)).astype(np.float32)
    run_and_compare(ops, x, ref, index_rows(rs, B, Np, Mcap), counts, Mcap, g, 0.75, patch=p)


# ---- B. compress / reconstruction sized by the capacity -----------------------------------------------------------------------------
COMPRESS_COUNTS = [0, 1, 32, 33, 63, 64, 65, 1024, 1025, 1056, 2100]
COMPRESS_MCAP = 2100
COMPRESS_ATTN_COUNTS = [0, 33, 1025, 2100]


def mce_relations(counts, Mcap):
    """What attn_compress_kernel's Mce = min(Mc, roundup32(mprime)) (attention.hip:613) is to mprime and Mc, per sample, when
    mprime == count; and the passes of its column loop (:623)."""
    Mc = (Mcap + 31) & ~31
    got = {}
    for m in counts:
        mce = min(Mc, (m + 31) & ~31)
        rel = ("mce_zero" if mce == 0 else "mce_equals_mc" if mce == Mc else
               "mce_exact_below_mc" if mce == m else "mce_rounded_below_mc")
        got.setdefault(rel, []).append(m)
        got.setdefault(("passes", -(-mce // AC_MAXT)), []).append(m)
        if mce > AC_MAXT and mce < Mc:
            got.setdefault("mce_loop_below_mc", []).append(m)
    return got


def recon_blocks(counts):
    """recon_masked_kernel's 64-row blocks (attention.hip:721-722, :784) per count: (full blocks, rows in the last partial block)."""
    return {(m // RM_BL, m % RM_BL) for m in counts}


def test_compress_and_reconstruction_sized_by_the_capacity(ops):
    """compress_capacity: 48x48 map, every masked position its own arg-max column (mprime == count), Mcap = 2100, eleven counts
    in one call.  Forward without the dense rows and backward for all of them; attn_rows for four samples in a second call."""
    h = w = 48
    N, Mcap, C = h * w, COMPRESS_MCAP, 16
    rs = np.random.RandomState(48)
    counts = rs.permutation(COMPRESS_COUNTS).astype(np.int32)
    B = len(counts)
    rec, prep = stage_lds(N, Mcap)
    assert rec > 48 * KIB and rec > prep and compress_lds(Mcap) > 48 * KIB
    rel = mce_relations(counts, Mcap)
    for r in ("mce_zero", "mce_exact_below_mc", "mce_rounded_below_mc", "mce_equals_mc", "mce_loop_below_mc", ("passes", 1), ("passes", 2), ("passes", 3)):
        assert rel.get(r), r
    assert {(0, 0), (0, 63), (1, 0), (1, 1)} <= recon_blocks(counts)        # empty, partial, exactly full, one row over
    parts = [proto_inputs(C, h, w, np.arange(N), [], seed=100 + b) for b in range(B)]
    x, ref, g = (np.concatenate([p_[i] for p_ in parts]) for i in (0, 1, 3))
    rows = index_rows(rs, B, N, Mcap)
    fo = orc.forward_masks(x, ref, rows, counts, Mcap)
    f, _ = run_and_compare(ops, x, ref, rows, counts, Mcap, g, 0.5, want_attn=False, fo=fo)
    for b, m in enumerate(counts):
        assert active_columns(f.ind[b:b + 1], rows[b, :m]) == [m]
    # the dense rows (attn_expand_kernel: rows past the count are zero) for four of the samples, without the index
    # (attn_compress_kernel<false>)
    sel = [int(np.nonzero(counts == m)[0][0]) for m in COMPRESS_ATTN_COUNTS]
    fa = ops.forward(dev(x[sel]), dev(ref[sel]), dev(rows[sel]), want_attn=True, want_index=False, counts=dev(counts[sel]))
    torch.cuda.synchronize()
    np.testing.assert_array_equal(fa.attn_rows.cpu().numpy(), fo.attn_rows[sel])
    np.testing.assert_array_equal(fa.out.cpu().numpy(), fo.out[sel])


# ---- C. the backward's instantiations under a capacity layout -----------------------------------------------------------------------
# one shape per (R, staged) from test_gpu_layer_limits.BW_CASES: "bw_r8_staged_top" -> ("bwcap_r8_staged", C, h, w, (R, staged))
BWCAP_CASES = [("bwcap_" + c[0][3:].rsplit("_", 1)[0],) + tuple(c[1:]) for c in BW_CASES
               if c[0] in ("bw_r8_staged_top", "bw_r4_staged_bottom", "bw_r2_staged_bottom", "bw_r2_unstaged_bottom",
                           "bw_r1_staged_bottom", "bw_r1_unstaged_bottom")]


@pytest.mark.parametrize("C,h,w,want", [c[1:] for c in BWCAP_CASES], ids=[c[0] for c in BWCAP_CASES])
def test_backward_instantiations_under_a_capacity_layout(ops, C, h, w, want):
    N = h * w
    M = int(N * 0.08)
    Mcap, counts = M + 37, [M, M // 3]
    x, ref, mpi, g = inputs("abs", 2, C, h, w, seed=N, M=Mcap)
    rs = np.random.RandomState(N + 1)
    rows = np.stack([mpi, np.sort(rs.choice(N, Mcap, replace=False)).astype(np.int32)])
    assert bw_variant(N, Mcap, 0)[:2] == want, (N, bw_variant(N, Mcap, 0))
    f, _ = run_and_compare(ops, x, ref, rows, counts, Mcap, g, 0.75)
    ic = index_counts(f.bwd_index, N)
    for surv, _ in ic:
        assert bw_variant(N, Mcap, surv)[:2] == want
    assert max(nlong for _, nlong in ic) > 0, "the cooperative long-column phase should run too"


def test_backward_survivors_beyond_bcap_under_a_capacity_layout(ops):
    """bwcap_survivors_beyond_bcap: signed features, counts [1024, 700] of capacity 1100: more survivor entries than BW_BCAP = 2048 in
    sample 0, read from L2 at the capacity's entB_w offset while offsets and one-hot entries stay in LDS."""
    N, Mcap = 32 * 64, 1100
    x, ref, mpi, g = inputs("signed", 2, 16, 32, 64, seed=7, M=Mcap)
    rows = np.stack([mpi, np.sort(np.random.RandomState(8).choice(N, Mcap, replace=False)).astype(np.int32)])
    f, _ = run_and_compare(ops, x, ref, rows, [1024, 700], Mcap, g, 1.0)
    surv = index_counts(f.bwd_index, N)[0][0]
    assert surv > 2048, surv
    assert bw_variant(N, Mcap, surv) == (8, True, False)


def test_backward_more_long_columns_than_maxlong_under_a_capacity_layout(ops):
    """bwcap_over_maxlong: 600 prototype columns with 9-11 one-hot entries each; counts [512, 40] of capacity 600: sample 0 defers
    more than BW_MAXLONG = 512 columns and walks the rest inline."""
    h, w, Pn, Mcap = 48, 128, 600, 600
    N = h * w
    parts = []
    for b in range(2):
        protos = np.random.RandomState(5 + b).choice(N, Pn, replace=False)
        parts.append(proto_inputs(16, h, w, protos[np.arange(N) % Pn], [], seed=6 + b))
    x, ref, g = (np.concatenate([p_[i] for p_ in parts]) for i in (0, 1, 3))
    rows = np.tile(np.arange(Mcap, dtype=np.int32), (2, 1))
    f, _ = run_and_compare(ops, x, ref, rows, [512, 40], Mcap, g, 0.5)
    (surv, nlong), _ = index_counts(f.bwd_index, N)
    assert nlong > 512, nlong
    assert bw_variant(N, Mcap, surv)[:2] == (2, True)


# ---- D. the trainer's own configuration ---------------------------------------------------------------------------------------------
def test_trainer_shared_index_and_one_row_per_sample(ops):
    """trainer_shared_index / trainer_per_row_index: the real layer shape (B 3, C 512, 32x32: <1,full>, the fast correlation kernel
    with k-split partials merged by the consumers) with the index as ipsr_index_prep leaves it — length N, padded with -1 — shared
    by the batch (mpi_stride = 0, Mcap = N, counts = its count for every sample), against the oracle; then the same index as one
    row per sample (mpi_stride = Mcap): identical bits."""
    B, C, h = 3, 512, 32
    N = h * h
    assert stage_variant(C) == "<1,full>" and P.corr_variant(C, N, False)[0] == "fast" and P.corr_plan(B, N)[2] > 1
    rs = np.random.RandomState(35)
    feat = ops.feat_mask(dev(stroke_mask(256, 4242)), 3, 5 / 16.0)
    _, mpi_d, cnt = ops.index_prep(feat, 1, 1, 1)
    M = int(cnt.item())
    mpi = mpi_d.cpu().numpy()
    assert 64 < M < 900 and mpi.shape == (N,) and (mpi[M:] == -1).all()
    x = np.abs(rs.standard_normal((B, C, h, h))).astype(np.float32)
    ref = np.maximum(rs.standard_normal((B, C, h, h)), 0).astype(np.float32)
    g = rs.standard_normal(x.shape).astype(np.float32)
    xd, rd, gd = dev(x), dev(ref), dev(g)
    counts = cnt.expand(B).contiguous()
    fo = orc.forward_masks(x, ref, mpi, [M] * B, N)
    gin_o = orc.backward(g, mpi, fo.attn_rows, fo.bwd_index, 1.0)
    got = []
    for index in (mpi_d, mpi_d.expand(B, N).contiguous()):
        f = ops.forward(xd, rd, index, want_attn=True, counts=counts)
        gin = ops.backward(gd, f.bwd_index, 1.0, N)
        torch.cuda.synchronize()
        got.append((f, gin))
    f, gin = got[0]
    np.testing.assert_array_equal(f.ind.cpu().numpy(), fo.ind)
    np.testing.assert_array_equal(f.vmax.cpu().numpy(), fo.vmax)
    np.testing.assert_array_equal(f.out.cpu().numpy(), fo.out)
    np.testing.assert_array_equal(f.attn_rows.cpu().numpy(), fo.attn_rows)
    assert_index_cap_equal(f.bwd_index, fo.bwd_index, N, [M] * B, N)
    np.testing.assert_array_equal(gin.cpu().numpy(), gin_o)
    f2, gin2 = got[1]
    for a, b in ((f.ind, f2.ind), (f.vmax, f2.vmax), (f.out, f2.out), (f.attn_rows, f2.attn_rows), (gin, gin2)):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    assert_index_cap_equal(f.bwd_index, f2.bwd_index, N, [M] * B, N)


# ---- E. clamps and the unread tail, between guard bands -----------------------------------------------------------------------------
def _guarded_layer(ops, monkeypatch, x, ref, rows, counts, g, tw, Mcap):
    """One forward + backward with every operand between guard bands, NaN-filled outputs and a NaN-filled workspace of exactly the
    queried size -> the results as numpy (index: its used part)."""
    arena = Arena(ws_fill="nan")
    host = dict(x=dev(x), ref=dev(ref), rows=dev(rows, torch.int32), counts=dev(np.asarray(counts, np.int32)), g=dev(g))
    t = {k: arena.guarded_copy(v, k) for k, v in host.items()}
    with arena.installed(monkeypatch):
        f = ops.forward(t["x"], t["ref"], t["rows"], want_attn=True, counts=t["counts"])
        gin = ops.backward(t["g"], f.bwd_index, tw, Mcap)
    torch.cuda.synchronize()
    arena.check_guards()
    assert arena.workspaces, "the call took no workspace from the arena"
    for k, v in host.items():
        assert torch.equal(v.view(torch.int32), t[k].view(torch.int32)), "operand %s was written" % k
    res = dict(out=f.out, ind=f.ind, vmax=f.vmax, attn_rows=f.attn_rows, gin=gin)
    for k in ("out", "vmax", "attn_rows", "gin"):
        assert not torch.isnan(res[k]).any(), "poisoned scratch or an unwritten element in %s" % k
    res = {k: v.cpu().numpy() for k, v in res.items()}
    N = x.shape[2] * x.shape[3]
    res["index"] = np.concatenate(used_index_cap(f.bwd_index, N, counts, Mcap))
    return res


def _same_bits(a, b):
    for k in a:
        np.testing.assert_array_equal(a[k].view(np.int32), b[k].view(np.int32), err_msg=k)


@pytest.fixture(scope="module")
def clamp_case():
    B, C, h, Mcap = 4, 20, 8, 23
    rs = np.random.RandomState(20)
    x = np.abs(rs.standard_normal((B, C, h, h))).astype(np.float32)
    ref = rs.rand(B, C, h, h).astype(np.float32)
    g = rs.standard_normal(x.shape).astype(np.float32)
    rows = index_rows(rs, B, h * h, Mcap)
    counts = [Mcap, 0, 7, 12]
    fo = orc.forward_masks(x, ref, rows, counts, Mcap)
    want = dict(out=fo.out, ind=fo.ind, vmax=fo.vmax, attn_rows=fo.attn_rows, gin=orc.backward_patch(g, Mcap, fo.bwd_index, 0.75, 1),
                index=np.concatenate(used_index_cap(fo.bwd_index, h * h, counts, Mcap)))
    return x, ref, rows, counts, g, Mcap, want


def test_counts_are_clamped_to_the_capacity(ops, monkeypatch, clamp_case):
    """clamp_counts: counts = Mcap + 5 gives the bits of Mcap, counts = -3 the bits of 0 (sample_count, attention.hip:543-548, and
    its copies in the compress / expand / recon kernels)."""
    x, ref, rows, counts, g, Mcap, want = clamp_case
    base = _guarded_layer(ops, monkeypatch, x, ref, rows, counts, g, 0.75, Mcap)
    _same_bits(base, want)
    over = _guarded_layer(ops, monkeypatch, x, ref, rows, [Mcap + 5, -3, 7, 12], g, 0.75, Mcap)
    # (used_index_cap clamps the same way, so the used parts line up)
    _same_bits(over, want)


@pytest.mark.parametrize("junk", [0x7FFFFFFF, -5], ids=["int_max", "minus5"])
def test_index_entries_past_the_count_are_never_read(ops, monkeypatch, clamp_case, junk):
    """unread_tail: include/ipsr_hip.h says entries past counts[b] are ignored: overwriting them changes no output bit."""
    x, ref, rows, counts, g, Mcap, want = clamp_case
    rows = rows.copy()
    for b, m in enumerate(counts):
        rows[b, m:] = junk
    assert (rows == junk).sum() == sum(Mcap - m for m in counts) > 0
    _same_bits(_guarded_layer(ops, monkeypatch, x, ref, rows, counts, g, 0.75, Mcap), want)


# ---- F. the bf16 correlation with per-sample counts ---------------------------------------------------------------------------------
def test_bf16_correlation_per_sample_counts_equal_batch_of_one(ops):
    """bf16_counts: p = 1, C 64, 16x16 (N % 128 == 0), counts {0, 40, 256} of capacity 256.  The oracle has no bf16 twin: the
    reference is the batch-of-one ops.forward(corr="bf16") with a host M, which test_gpu_parity.py and test_gpu_corr_variants.py pin."""
    B, C, h, Mcap = 3, 64, 16, 256
    N = h * h
    assert P.corr_bf16_supported(C, N)
    rs = np.random.RandomState(64)
    x = np.abs(rs.standard_normal((B, C, h, h))).astype(np.float32)
    ref = np.maximum(rs.standard_normal((B, C, h, h)), 0).astype(np.float32)
    g = rs.standard_normal(x.shape).astype(np.float32)
    counts = [40, 0, 256]
    rows = []
    for m in counts:                                   # the live positions first (ascending), then the rest of the grid
        live = np.sort(rs.choice(N, m, replace=False))
        rows.append(np.concatenate([live, np.setdiff1d(np.arange(N), live)]))
    rows = np.stack(rows).astype(np.int32)
    xd, rd, gd, rowsd = dev(x), dev(ref), dev(g), dev(rows)
    fb = ops.forward(xd, rd, rowsd, corr="bf16", counts=dev(np.asarray(counts, np.int32)))
    gb = ops.backward(gd, fb.bwd_index, 0.75, Mcap)
    torch.cuda.synchronize()
    used = used_index_cap(fb.bwd_index, N, counts, Mcap)
    for b, m in enumerate(counts):
        f1 = ops.forward(xd[b:b + 1], rd[b:b + 1], rowsd[b, :m].contiguous(), corr="bf16")
        g1 = ops.backward(gd[b:b + 1], f1.bwd_index, 0.75, m)
        torch.cuda.synchronize()
        for name, a, c in (("out", fb.out[b], f1.out[0]), ("ind", fb.ind[b], f1.ind[0]), ("vmax", fb.vmax[b], f1.vmax[0]), ("gin", gb[b], g1[0])):
            assert torch.equal(a.view(torch.int32), c.view(torch.int32)), "%s of sample %d (count %d)" % (name, b, m)
        np.testing.assert_array_equal(used[b], used_index(f1.bwd_index, N, m)[0])


# ---- G. the limit and the refusals, judged by the capacity --------------------------------------------------------------------------
def test_limit_n9600_capacity_6388(ops):
    """limit_cap6388: N = 9600, Mcap = 6388 (both roles of the stage kernel at exactly 150 KiB), counts [6388, 5]: the first sample is
    the host-M limit case, the second runs five steps inside the same carve; the backward runs <1,unstaged> at the capacity's capB."""
    h, w, C = 96, 100, 8
    N, Mcap = h * w, 6388
    assert stage_lds(N, Mcap) == (150 * KIB, 150 * KIB) and 48 * KIB < compress_lds(Mcap) <= 150 * KIB
    rs = np.random.RandomState(3)
    counts = [Mcap, 5]
    parts = [proto_inputs(C, h, w, np.arange(N), [], seed=4 + b) for b in range(2)]
    x, ref, g = (np.concatenate([p_[i] for p_ in parts]) for i in (0, 1, 3))
    rows = index_rows(rs, 2, N, Mcap)
    f, _ = run_and_compare(ops, x, ref, rows, counts, Mcap, g, 0.25, want_attn=False)
    for b, m in enumerate(counts):
        assert active_columns(f.ind[b:b + 1], rows[b, :m]) == [m]
    for surv, _ in index_counts(f.bwd_index, N):
        assert bw_variant(N, Mcap, surv)[:2] == (1, False)


REFUSALS = [
    # id,               C,    h,  w,   p, Mcap, counts
    ("refuse_cap6389",  8,    96, 100, 1, 6389, [1]),      # recurrence step lists > 150 KiB by the capacity; one position masked
    ("refuse_n9604",    8,    98, 98,  1, 16,   [3]),      # prepare role: 4 * 9604 ints > 150 KiB
    ("refuse_cp8196",   2049, 6,  6,   2, 4,    [2]),      # C*p*p = 8196 > 8192
]


@pytest.mark.parametrize("C,h,w,p,Mcap,counts", [c[1:] for c in REFUSALS], ids=[c[0] for c in REFUSALS])
def test_refusals_by_capacity_write_nothing(ops, C, h, w, p, Mcap, counts):
    from deepinpainting_amd import _lib
    L = _lib.lib()
    Np = (h - p + 1) * (w - p + 1)
    rs = np.random.RandomState(Mcap)
    x = torch.rand(1, C, h, w, device="cuda")
    ref = torch.rand(1, C, h, w, device="cuda")
    mpi = dev(np.sort(rs.choice(Np, Mcap, replace=False))[None], torch.int32)
    cnt = dev(np.asarray(counts, np.int32))
    if p == 1:
        assert max(stage_lds(Np, Mcap)) > 150 * KIB
    else:
        assert stage_variant((C * p * p + 7) & ~7) == "refused"
    with pytest.raises(NotImplementedError):
        ops.forward(x, ref, mpi, patch=p, want_attn=True, counts=cnt)
    out = _nan_fill(torch.empty(1, C, h, w, device="cuda"))
    ind = _nan_fill(torch.empty(1, Np, dtype=torch.int32, device="cuda"))
    vmax = _nan_fill(torch.empty(1, Np, device="cuda"))
    attn = _nan_fill(torch.empty(1, Mcap, Np, device="cuda"))
    bidx = _nan_fill(torch.empty(1, L.ipsr_bwd_index_ints(Np, Mcap), dtype=torch.int32, device="cuda"))
    keep = [t.clone() for t in (out, ind, vmax, attn, bidx)]
    nbytes = L.ipsr_forward_workspace_bytes(1, C, h, w, Mcap, p, 1)
    ws = torch.empty(max(nbytes, 16), dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    rc = L.ipsr_forward_masks(x.data_ptr(), ref.data_ptr(), mpi.data_ptr(), Mcap, cnt.data_ptr(), Mcap, 1, C, h, w, p, 1, out.data_ptr(),
                              ind.data_ptr(), vmax.data_ptr(), attn.data_ptr(), bidx.data_ptr(), ws.data_ptr(), ctypes.c_size_t(nbytes),
                              ops._stream(), 0)
    torch.cuda.synchronize()
    assert rc == IPSR_ERR_UNSUPPORTED, (rc, L.ipsr_last_error())
    for name, a, b in zip(("out", "ind", "vmax", "attn_rows", "bwd_index"), (out, ind, vmax, attn, bidx), keep):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32)), "%s was written by a refused call" % name


# ---- H. every row of the table has a case that reaches it ---------------------------------------------------------------------------
def _rec(cid):
    C, h, w, p, want = next(c[1:] for c in REC_CASES if c[0] == cid)
    Cp = (C * p * p + 7) & ~7
    return Cp, stage_variant(Cp), rec_body(Cp), tail_branches(rec_body(Cp), rec_counts(Cp))


def _bwcap(cid):
    C, h, w, want = next(c[1:] for c in BWCAP_CASES if c[0] == cid)
    return bw_variant(h * w, int(h * w * 0.08) + 37, 0)[:2]


_COMPRESS_REL = mce_relations(COMPRESS_COUNTS, COMPRESS_MCAP)

# row -> (case ids, what the launchers' formulas must give for each of them).  The data-dependent rows (survivors beyond bcap, more
# than BW_MAXLONG long columns) are asserted from the results inside their own tests; here their (R, staged) half is restated.
ROWS = {
    "stage_1_partial": (["rec_c16"], lambda c: _rec(c)[1] == "<1,partial>"),
    "stage_1_full": (["rec_c512"], lambda c: _rec(c)[1] == "<1,full>"),
    "stage_2_full": (["rec_c1024"], lambda c: _rec(c)[1] == "<2,full>"),
    "stage_3_full": (["rec_c384_p2"], lambda c: _rec(c)[1] == "<3,full>"),
    "stage_3_partial": (["rec_c130_p3"], lambda c: _rec(c)[1] == "<3,partial>"),
    "stage_4_full": (["rec_c512_p2"], lambda c: _rec(c)[1] == "<4,full>"),
    "stage_8": (["rec_c256_p3"], lambda c: _rec(c)[1] == "<8>"),
    "stage_12": (["rec_c512_p3"], lambda c: _rec(c)[1] == "<12>"),
    "stage_16": (["rec_c768_p3"], lambda c: _rec(c)[1] == "<16>" and _rec(c)[0] < 8192),
    "stage_16_ceiling": (["rec_c2048_p2"], lambda c: _rec(c)[1] == "<16>" and _rec(c)[0] == 8192),
    "ring_tails": (["rec_c16", "rec_c512", "rec_c1024", "rec_c384_p2", "rec_c130_p3"],
                   lambda c: _rec(c)[2] == "ring" and _rec(c)[3] == WANT_TAILS["ring"]),
    "wide_tails": (["rec_c512_p2"], lambda c: _rec(c)[2] == "wide" and _rec(c)[3] == WANT_TAILS["wide"]),
    "quad_tails": (["rec_c256_p3", "rec_c512_p3", "rec_c768_p3", "rec_c2048_p2"],
                   lambda c: _rec(c)[2] == "quad" and _rec(c)[3] == WANT_TAILS["quad"]),
    "mce_zero": (["compress_capacity"], lambda c: _COMPRESS_REL.get("mce_zero") == [0]),
    "mce_exact_below_mc": (["compress_capacity"], lambda c: {32, 64, 1024, 1056} <= set(_COMPRESS_REL.get("mce_exact_below_mc", []))),
    "mce_rounded_below_mc": (["compress_capacity"], lambda c: {1, 33, 63, 65, 1025} <= set(_COMPRESS_REL.get("mce_rounded_below_mc", []))),
    "mce_equals_mc": (["compress_capacity"], lambda c: _COMPRESS_REL.get("mce_equals_mc") == [2100]),
    "mce_loop_below_mc": (["compress_capacity"], lambda c: {1025, 1056} <= set(_COMPRESS_REL.get("mce_loop_below_mc", []))),
    "compress_loops": (["compress_capacity"], lambda c: all(_COMPRESS_REL.get(("passes", n)) for n in (1, 2, 3))),
    "lds_above_48k": (["compress_capacity"], lambda c: stage_lds(48 * 48, COMPRESS_MCAP)[0] > 48 * KIB < compress_lds(COMPRESS_MCAP)),
    "recon_block_edges": (["compress_capacity"], lambda c: {(0, 0), (0, 63), (1, 0), (1, 1)} <= recon_blocks(COMPRESS_COUNTS)
                          and set(COMPRESS_ATTN_COUNTS) <= set(COMPRESS_COUNTS) and min(COMPRESS_ATTN_COUNTS) == 0),
    "bw_r8_staged": (["bwcap_r8_staged"], lambda c: _bwcap(c) == (8, True)),
    "bw_r4_staged": (["bwcap_r4_staged"], lambda c: _bwcap(c) == (4, True)),
    "bw_r2_staged": (["bwcap_r2_staged"], lambda c: _bwcap(c) == (2, True)),
    "bw_r2_unstaged": (["bwcap_r2_unstaged"], lambda c: _bwcap(c) == (2, False)),
    "bw_r1_staged": (["bwcap_r1_staged"], lambda c: _bwcap(c) == (1, True)),
    "bw_r1_unstaged": (["bwcap_r1_unstaged", "limit_cap6388"],
                       lambda c: (bw_variant(9600, 6388, 0)[:2] if c == "limit_cap6388" else _bwcap(c)) == (1, False)),
    "bw_survivors_beyond_bcap": (["bwcap_survivors_beyond_bcap"], lambda c: bw_variant(32 * 64, 1100, 2049) == (8, True, False)),
    "bw_over_maxlong": (["bwcap_over_maxlong"], lambda c: bw_variant(48 * 128, 600, 0)[:2] == (2, True)),
    "shared_index": (["trainer_shared_index"], lambda c: stage_variant(512) == "<1,full>"),
    "per_row_index": (["trainer_per_row_index"], lambda c: True),
    "clamps": (["clamp_counts", "unread_tail"], lambda c: True),
    "bf16_corr": (["bf16_counts"], lambda c: P.corr_bf16_supported(64, 256)),
    "limit": (["limit_cap6388"], lambda c: stage_lds(9600, 6388) == (150 * KIB, 150 * KIB)),
    "refusals": (["refuse_cap6389", "refuse_n9604", "refuse_cp8196"],
                 lambda c: {"refuse_cap6389": max(stage_lds(9600, 6389)) > 150 * KIB >= max(stage_lds(9600, 1)),
                            "refuse_n9604": max(stage_lds(9604, 16)) > 150 * KIB,
                            "refuse_cp8196": stage_variant((2049 * 4 + 7) & ~7) == "refused"}[c]),
}

# the ids the tests above run under: parametrised ids, and the ids the single-case tests name in their docstrings
RUN_IDS = ([c[0] for c in REC_CASES] + [c[0] for c in BWCAP_CASES] + [c[0] for c in REFUSALS] +
           ["compress_capacity", "bwcap_survivors_beyond_bcap", "bwcap_over_maxlong", "trainer_shared_index", "trainer_per_row_index",
            "clamp_counts", "unread_tail", "bf16_counts", "limit_cap6388"])


def test_every_variant_is_reached():
    """Every row of the table at the top has at least one case, every case it names is one the tests above run and reaches the row
    by the launcher's own formula, every case serves a row, and the table in the docstring is this one."""
    assert len(set(RUN_IDS)) == len(RUN_IDS)
    named = set()
    for row, (cases, reaches) in ROWS.items():
        assert cases, row
        for cid in cases:
            assert cid in RUN_IDS, (row, cid)
            assert reaches(cid), (row, cid)
            named.add(cid)
    assert named == set(RUN_IDS), set(RUN_IDS) ^ named
    doc = [ln.split() for ln in __doc__.splitlines() if ln.startswith("  ")]
    doc_rows = [t[0] for t in doc if t and t[0] in ROWS]
    assert doc_rows == list(ROWS), "the docstring table and ROWS list different rows"
    words = {t.strip(",") for ln in doc for t in ln}
    assert set(RUN_IDS) <= words, set(RUN_IDS) - words
    # the six backward instantiations, the ten stage instantiations (nine distinct kernels, <16> twice) are all there
    assert {_bwcap(c[0]) for c in BWCAP_CASES} == {(8, True), (4, True), (2, True), (2, False), (1, True), (1, False)}
    assert [_rec(c[0])[1] for c in REC_CASES] == [c[5] for c in REC_CASES] and len(REC_CASES) == 10
