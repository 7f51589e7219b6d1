"""The IPSR layer at its documented limits (DESIGN.md §8 "Limits"), bit for bit against the CPU oracle.

Every launch variant below is chosen by the launcher from N, M and the patch length, never by the training steps' shapes, so a
retune could move real layers onto it unnoticed.  Each case computes the variant it reaches from the launcher's own formula (the
helpers cite the lines) and asserts it before comparing; the data-dependent counts (survivors, long columns, active columns) are
read back from the returned `bwd_index` / `ind`, not assumed.

  variant                                              selected at                      case id(s)
  ---------------------------------------------------  -------------------------------  ------------------------------------------
  ipsr_backward_kernel<8, staged>   N <= 2108          backward.hip:226-236             bw_r8_staged_top (N 2108)
  ipsr_backward_kernel<4, staged>   2109 .. 4220       backward.hip:226-236             bw_r4_staged_bottom (2109), bw_r4_staged_top (4220)
  ipsr_backward_kernel<2, staged>   4221 .. 7678       backward.hip:226-236             bw_r2_staged_bottom (4221), bw_r2_staged_top (7678)
  ipsr_backward_kernel<2, unstaged> 7679 .. 8444       backward.hip:226-236             bw_r2_unstaged_bottom (7679), bw_r2_unstaged_top (8444)
  ipsr_backward_kernel<1, staged>   8445 .. 9598       backward.hip:226-236             bw_r1_staged_bottom (8445), bw_r1_staged_top (9598)
  ipsr_backward_kernel<1, unstaged> 9599 ..            backward.hip:226-236             bw_r1_unstaged_bottom (9599), limit_n9600_m6388
  staged, survivors > bcap (read from L2)              backward.hip:236, :211-216       bw_r8_staged_survivors_beyond_bcap
  more than BW_MAXLONG = 512 long columns (inline)     backward.hip:40-46               bw_r2_staged_over_maxlong_long_columns
  attention_stage_kernel ring > 48 KiB dynamic LDS     attention.hip:796-801, :822-829  stage_ring_above_48k_compress_loops
  attention_stage_kernel<3, FULL> (Cp 1536)            attention.hip:834                stage_nch3_full
  attention_stage_kernel<3, partial> (Cp 1176)         attention.hip:834-835            stage_nch3_partial
  attention_stage_kernel<4, FULL> (Cp 2048)            attention.hip:834                stage_nch4_full
  attention_stage_kernel<8>  (Cp 2049 .. 4096)         attention.hip:843                stage_wide8
  attention_stage_kernel<12> (Cp 4097 .. 6144)         attention.hip:844                stage_wide12
  attention_stage_kernel<16> (Cp 6145 .. 8192)         attention.hip:845                stage_wide16, stage_wide16_cp8192 (C 2048, p 2)
  attn_compress_kernel, > AC_MAXT = 1024 columns       attention.hip:613, :859          stage_ring_above_48k_compress_loops, limit_n9600_m6388
  attn_compress_kernel, LDS > 48 KiB                   attention.hip:802, :854-858      stage_ring_above_48k_compress_loops, limit_n9600_m6388
  N = 9600, M = 6388: stage LDS exactly 150 KiB        attention.hip:796-807            limit_n9600_m6388
  patch_normalize_reg_kernel<64|32|16|8|4>             normalize.hip:183-196            norm_reg_L64 .. norm_reg_L4
  patch_normalize_kernel (generic)                     normalize.hip:185, :201          norm_generic_L3, norm_generic_L65
  refusal N = 9604 (stage LDS)                         attention.hip:807, api.hip:283   refuse_n9604
  refusal M = 6389 at N = 9600 (stage LDS)             attention.hip:807, api.hip:283   refuse_m6389
  refusal C*p*p = 8196 > 8192                          attention.hip:808, api.hip:283   refuse_cp8196

A refusal is checked twice: through `ops.forward` it raises NotImplementedError, and at the C ABI it returns IPSR_ERR_UNSUPPORTED
with every output buffer (out, ind, vmax, attn_rows, bwd_index), pre-filled with a NaN bit pattern, bitwise unchanged after a device
synchronisation: the limits are checked before the first launch (api.hip:283), not by the attention launcher after the correlation
has already written `ind` / `vmax`.
"""
import ctypes

import numpy as np
import pytest
import torch

from oracle import ipsr_oracle as orc
from test_gpu_parity import assert_index_equal

pytestmark = pytest.mark.gpu

IPSR_ERR_UNSUPPORTED = -2
KIB = 1024


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    from deepinpainting_amd import ops as _ops
    return _ops


def dev(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a))
    return (t.to(dtype) if dtype is not None else t).cuda()


def cdiv(a, b):
    return -(-a // b)


# ---- the launchers' formulas ------------------------------------------------------------------------------------------------------
def bw_variant(N, M, surv):
    """(R, staged, survivors in LDS) of ipsr_backward_kernel: launch_backward, backward.hip:226-236."""
    R = 8                                                           # BW_ROWS
    while R > 1 and R * (N + 4) * 4 > 66 * KIB:                     # BW_PAD, BW_LDS_BYTES (:227)
        R >>= 1
    rows = R * (N + 4) * 4
    assert rows <= 150 * KIB                                        # (:229)
    idx = (3 * N + 2) * 4
    staged = rows + idx <= 150 * KIB                                # BW_LDS_LIMIT (:233)
    bcap = min(2048, M * (M + 1) // 2, (150 * KIB - rows - idx) // 8) if staged else 0     # BW_BCAP (:235-236)
    return R, staged, staged and surv <= bcap


def stage_lds(N, M):
    """attention.hip:796-801 (stage_lds_bytes): (recurrence step lists, prepare role's 4N ints)."""
    rec = 6 * (((M + 3) & ~3) + 3 * 4) * 4 if M > 0 else 0         # RING = 4
    return rec, 4 * N * 4


def stage_variant(Cp):
    """attention.hip:831-846: the attention_stage_kernel<NCH, FULL> instantiation."""
    nch = cdiv(Cp, 512)
    if nch <= 4:
        return "<%d,%s>" % (nch, "full" if Cp == 512 * nch else "partial")
    for top in (8, 12, 16):
        if nch <= top:
            return "<%d>" % top
    return "refused"


def compress_lds(M):
    """attention.hip:802 (compress_lds_bytes), Mc = roundup(M, 32) (api.hip plan_forward)."""
    Mc = (M + 31) & ~31
    return (4 * M + Mc + 1 + M) * 4


def norm_variant(C):
    """normalize.hip:183-196: patch_normalize_reg_kernel<L> when L = ceil(C/8) is 4..64 and a multiple of 4, else the generic kernel."""
    L = cdiv(C, 8)
    Cp = (C + 7) & ~7
    return "reg<%d>" % L if (L <= 64 and L % 4 == 0 and 8 * L >= Cp) else "generic"


def index_counts(bwd_index, N):
    """Per sample: (survivor entries offB[N], long columns = more than BW_INLINE = 8 entries in all)."""
    bi = bwd_index if isinstance(bwd_index, np.ndarray) else bwd_index.cpu().numpy()
    out = []
    for row in bi:
        offA, offB = row[:N + 1].astype(np.int64), row[2 * N + 1:3 * N + 2].astype(np.int64)
        lens = (offA[1:] - offA[:-1]) + (offB[1:] - offB[:-1])
        out.append((int(offB[N]), int((lens > 8).sum())))
    return out


def active_columns(ind, mpi):
    """mprime: distinct arg-max columns of the masked positions (the columns attn_compress_kernel replays)."""
    ind = ind if isinstance(ind, np.ndarray) else ind.cpu().numpy()
    return [len(np.unique(r[np.asarray(mpi, np.int64)])) for r in ind]


# ---- inputs -----------------------------------------------------------------------------------------------------------------------
def inputs(kind, B, C, h, w, seed, frac=0.1, M=None):
    """abs: non-negative features, few survivors; signed: survivors everywhere."""
    rs = np.random.RandomState(seed)
    N = h * w
    if kind == "abs":
        x = np.abs(rs.standard_normal((B, C, h, w))).astype(np.float32)
        ref = rs.rand(B, C, h, w).astype(np.float32)
    else:
        x = rs.standard_normal((B, C, h, w)).astype(np.float32)
        ref = rs.standard_normal((B, C, h, w)).astype(np.float32)
    if M is None:
        mpi = np.sort(rs.choice(N, max(1, int(N * frac)), replace=False)).astype(np.int32)
    else:
        mpi = np.sort(rs.choice(N, M, replace=False)).astype(np.int32)
    g = rs.standard_normal((B, C, h, w)).astype(np.float32)
    return x, ref, mpi, g


def proto_inputs(C, h, w, own, mpi, seed):
    """x = unit-norm random columns; ref[:, q] = x[:, own[q]].  The arg-max of ref column q over the normalised x columns
    (ipsr_corr_argmax_cpu) is then exactly own[q]: correlation 1 there, < 1 with every other (distinct) column."""
    rs = np.random.RandomState(seed)
    N = h * w
    x = rs.standard_normal((1, C, N)).astype(np.float32)
    x /= np.linalg.norm(x, axis=1, keepdims=True)
    ref = np.ascontiguousarray(x[:, :, own])
    g = rs.standard_normal((1, C, h, w)).astype(np.float32)
    return x.reshape(1, C, h, w), ref.reshape(1, C, h, w), np.asarray(mpi, np.int32), g


def run_and_compare(ops, x, ref, mpi, g, tw, patch=1):
    """HIP vs oracle, everything bit for bit (as test_layer_random_shapes_vs_oracle): ind, vmax, attn_rows, the used part of
    bwd_index, out, gin.  Returns the HIP forward."""
    B, C, h, w = x.shape
    Np = (h - patch + 1) * (w - patch + 1)
    M = len(mpi)
    fo = orc.forward(x, ref, mpi, patch=patch)
    gin_o = orc.backward(g, mpi, fo.attn_rows, fo.bwd_index, tw) if patch == 1 else orc.backward_patch(g, M, fo.bwd_index, tw, patch)
    f = ops.forward(dev(x), dev(ref), dev(mpi, torch.int32), patch=patch, want_attn=True)
    gin = ops.backward(dev(g), f.bwd_index, tw, M, patch=patch)
    torch.cuda.synchronize()
    np.testing.assert_array_equal(f.ind.cpu().numpy(), fo.ind)
    np.testing.assert_array_equal(f.vmax.cpu().numpy(), fo.vmax)
    np.testing.assert_array_equal(f.attn_rows.cpu().numpy(), fo.attn_rows)
    assert_index_equal(f.bwd_index, fo.bwd_index, Np, M)
    np.testing.assert_array_equal(f.out.cpu().numpy(), fo.out)
    np.testing.assert_array_equal(gin.cpu().numpy(), gin_o)
    return f


# ---- A. the backward's (R, staged) instantiations, one case each side of every boundary ------------------------------------------------
BW_CASES = [
    # id,                      C,  h,    w,   (R, staged)
    ("bw_r8_staged_top",       12, 31,   68,  (8, True)),     # N 2108: last N with 8 LDS rows; C 12: a half-full last row block
    ("bw_r4_staged_bottom",    12, 37,   57,  (4, True)),     # N 2109
    ("bw_r4_staged_top",       10, 20,   211, (4, True)),     # N 4220
    ("bw_r2_staged_bottom",    9,  63,   67,  (2, True)),     # N 4221
    ("bw_r2_staged_top",       9,  22,   349, (2, True)),     # N 7678: last N whose CSR offsets fit beside 2 rows
    ("bw_r2_unstaged_bottom",  9,  7,    1097, (2, False)),   # N 7679
    ("bw_r2_unstaged_top",     9,  4,    2111, (2, False)),   # N 8444
    ("bw_r1_staged_bottom",    8,  15,   563, (1, True)),     # N 8445
    ("bw_r1_staged_top",       8,  2,    4799, (1, True)),    # N 9598
    ("bw_r1_unstaged_bottom",  8,  29,   331, (1, False)),    # N 9599
]


@pytest.mark.parametrize("C,h,w,want", [c[1:] for c in BW_CASES], ids=[c[0] for c in BW_CASES])
def test_backward_instantiations_at_their_boundaries(ops, C, h, w, want):
    N = h * w
    x, ref, mpi, g = inputs("abs", 1, C, h, w, seed=N, frac=0.08)
    f = run_and_compare(ops, x, ref, mpi, g, 0.75)
    (surv, nlong), = index_counts(f.bwd_index, N)
    R, staged, _ = bw_variant(N, len(mpi), surv)
    assert (R, staged) == want, (N, R, staged)
    assert nlong > 0, "the cooperative long-column phase should run too"


def test_backward_survivors_beyond_bcap(ops):
    """bw_r8_staged_survivors_beyond_bcap: signed features, more survivor entries than BW_BCAP = 2048 -> the staged kernel reads them
    from L2 (backward.hip:211-216) while the offsets and one-hot entries stay in LDS."""
    x, ref, mpi, g = inputs("signed", 2, 16, 32, 64, seed=7, M=1024)
    N = 32 * 64
    f = run_and_compare(ops, x, ref, mpi, g, 1.0)
    for surv, _ in index_counts(f.bwd_index, N):
        assert surv > 2048, surv
        assert bw_variant(N, len(mpi), surv) == (8, True, False)


def test_backward_more_long_columns_than_maxlong(ops):
    """bw_r2_staged_over_maxlong_long_columns: 600 columns with 9-11 one-hot entries each (> BW_INLINE = 8): more than BW_MAXLONG = 512
    deferred columns, so the rest fall through to the inline walk (backward.hip:40-46)."""
    h, w, P = 48, 128, 600
    N = h * w
    rs = np.random.RandomState(5)
    protos = rs.choice(N, P, replace=False)
    own = protos[np.arange(N) % P]
    x, ref, mpi, g = proto_inputs(16, h, w, own, np.arange(512), seed=6)
    f = run_and_compare(ops, x, ref, mpi, g, 0.5)
    (surv, nlong), = index_counts(f.bwd_index, N)
    assert nlong > 512, nlong
    assert bw_variant(N, len(mpi), surv)[:2] == (2, True)


# ---- A. the stage kernel: recurrence ring above 48 KiB, FULL nch 3 / 4, the wide buckets; the compress kernel --------------------------
def test_stage_ring_above_48k_compress_loops(ops):
    """stage_ring_above_48k_compress_loops: M = 2100 masked positions of a 48x48 map, each its own arg-max column: the recurrence's
    step lists need 50688 B of dynamic LDS (more than the prepare role's 36864 B and than 48 KiB), attn_compress_kernel 50452 B and
    2100 active columns (> AC_MAXT = 1024: the looping path)."""
    h = w = 48
    N, M = h * w, 2100
    x, ref, mpi, g = proto_inputs(16, h, w, np.arange(N), np.arange(M), seed=11)
    rec, prep = stage_lds(N, M)
    assert rec > 48 * KIB and rec > prep and compress_lds(M) > 48 * KIB
    f = run_and_compare(ops, x, ref, mpi, g, 0.5)
    assert active_columns(f.ind, mpi) == [M]


STAGE_CASES = [
    # id,                  B, C,    h,  w,  p, variant
    ("stage_nch3_full",    1, 384,  7,  9,  2, "<3,full>"),       # Cp 1536
    ("stage_nch3_partial", 2, 130,  8,  8,  3, "<3,partial>"),    # Cp 1176
    ("stage_nch4_full",    1, 512,  8,  7,  2, "<4,full>"),       # Cp 2048 (C 512, p 2)
    ("stage_wide8",        1, 256,  8,  9,  3, "<8>"),            # Cp 2304
    ("stage_wide12",       1, 512,  7,  8,  3, "<12>"),           # Cp 4608
    ("stage_wide16",       1, 768,  8,  8,  3, "<16>"),           # Cp 6912
    ("stage_wide16_cp8192", 1, 2048, 5, 6,  2, "<16>"),           # Cp 8192 exactly: the largest patch admitted
]


@pytest.mark.parametrize("B,C,h,w,p,want", [c[1:] for c in STAGE_CASES], ids=[c[0] for c in STAGE_CASES])
def test_stage_kernel_instantiations(ops, B, C, h, w, p, want):
    K = C * p * p
    assert stage_variant((K + 7) & ~7) == want
    rs = np.random.RandomState(K + h)
    x = np.abs(rs.standard_normal((B, C, h, w))).astype(np.float32)
    ref = rs.rand(B, C, h, w).astype(np.float32)
    Np = (h - p + 1) * (w - p + 1)
    mpi = np.sort(rs.choice(Np, max(2, Np // 4), replace=False)).astype(np.int32)
    g = rs.standard_normal((B, C, h, w)).astype(np.float32)
    run_and_compare(ops, x, ref, mpi, g, 0.75, patch=p)


def test_limit_n9600_m6388(ops):
    """limit_n9600_m6388: the largest layer the stage kernel admits: N = 9600 (a 96x100 map, the prepare role's 4N ints = 150 KiB) with
    M = 6388 (the recurrence's step lists = 150 KiB too); every masked position has its own arg-max column, so attn_compress_kernel
    replays 6388 columns (> 1024: looping) from 153364 B of LDS; the backward runs <1, unstaged>."""
    h, w = 96, 100
    N, M = h * w, 6388
    rs = np.random.RandomState(3)
    mpi = np.sort(rs.choice(N, M, replace=False))
    x, ref, mpi, g = proto_inputs(8, h, w, np.arange(N), mpi, seed=4)
    assert stage_lds(N, M) == (150 * KIB, 150 * KIB) and 48 * KIB < compress_lds(M) <= 150 * KIB
    f = run_and_compare(ops, x, ref, mpi, g, 0.25)
    assert active_columns(f.ind, mpi) == [M]
    (surv, _), = index_counts(f.bwd_index, N)
    assert bw_variant(N, M, surv)[:2] == (1, False)


# ---- A. patch normalisation: the register kernel per L and the generic fallback ------------------------------------------------------
NORM_CASES = [("norm_reg_L64", 512, "reg<64>"), ("norm_reg_L32", 256, "reg<32>"), ("norm_reg_L16", 128, "reg<16>"),
              ("norm_reg_L8", 64, "reg<8>"), ("norm_reg_L4", 32, "reg<4>"), ("norm_generic_L3", 20, "generic"),
              ("norm_generic_L65", 520, "generic")]


@pytest.mark.parametrize("C,want", [c[1:] for c in NORM_CASES], ids=[c[0] for c in NORM_CASES])
def test_patch_normalize_variants(ops, C, want):
    assert norm_variant(C) == want
    x, ref, mpi, g = inputs("abs", 2, C, 9, 12, seed=C, frac=0.25)
    run_and_compare(ops, x, ref, mpi, g, 0.5)


# ---- A. refusals, one step past each limit -----------------------------------------------------------------------------------------
REFUSALS = [
    # id,              C,    h,  w,   p, M
    ("refuse_n9604",   8,    98, 98,  1, 16),       # prepare role: 4 * 9604 ints > 150 KiB
    ("refuse_m6389",   8,    96, 100, 1, 6389),     # recurrence step lists > 150 KiB
    ("refuse_cp8196",  2049, 6,  6,   2, 4),        # C*p*p = 8196 > 8192
]


def _nan_fill(t):
    """Fill with a NaN bit pattern (int32 buffers get the same 32-bit word)."""
    t.view(torch.int32).fill_(0x7FC00DAD)
    return t


@pytest.mark.parametrize("C,h,w,p,M", [c[1:] for c in REFUSALS], ids=[c[0] for c in REFUSALS])
def test_refusals_write_nothing(ops, C, h, w, p, M):
    from deepinpainting_amd import _lib
    L = _lib.lib()
    Np = (h - p + 1) * (w - p + 1)
    rs = np.random.RandomState(M)
    x = torch.rand(1, C, h, w, device="cuda")
    ref = torch.rand(1, C, h, w, device="cuda")
    mpi = dev(np.sort(rs.choice(Np, M, replace=False)), torch.int32)
    if p == 1:
        assert max(stage_lds(Np, M)) > 150 * KIB
    else:
        assert stage_variant((C * p * p + 7) & ~7) == "refused"
    with pytest.raises(NotImplementedError):
        ops.forward(x, ref, mpi, patch=p, want_attn=True)
    out = _nan_fill(torch.empty(1, C, h, w, device="cuda"))
    ind = _nan_fill(torch.empty(1, Np, dtype=torch.int32, device="cuda"))
    vmax = _nan_fill(torch.empty(1, Np, device="cuda"))
    attn = _nan_fill(torch.empty(1, M, Np, device="cuda"))
    bidx = _nan_fill(torch.empty(1, L.ipsr_bwd_index_ints(Np, M), dtype=torch.int32, device="cuda"))
    keep = [t.clone() for t in (out, ind, vmax, attn, bidx)]
    nbytes = L.ipsr_forward_workspace_bytes(1, C, h, w, M, p, 1)
    ws = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    rc = L.ipsr_forward(x.data_ptr(), ref.data_ptr(), mpi.data_ptr(), M, 1, C, h, w, p, 1, out.data_ptr(), ind.data_ptr(), vmax.data_ptr(),
                        attn.data_ptr(), bidx.data_ptr(), ws.data_ptr(), ctypes.c_size_t(nbytes), ops._stream())
    torch.cuda.synchronize()
    assert rc == IPSR_ERR_UNSUPPORTED, (rc, L.ipsr_last_error())
    for name, a, b in zip(("out", "ind", "vmax", "attn_rows", "bwd_index"), (out, ind, vmax, attn, bidx), keep):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32)), "%s was written by a refused call" % name

