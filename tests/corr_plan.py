"""The launchers of csrc/corr_argmax.hip (and its two small neighbours, csrc/innercos.hip and the index kernel of csrc/mask_ops.hip)
restated in Python: which kernel instantiation, k-split plan and grid a shape reaches.

A plain module (like thin_conv_plan.py).  tests/test_corr_plan.py ties it to the built library through the workspace queries and
proves that the case tables below reach every row of the variant table; tests/test_gpu_corr_variants.py runs the tables.  Each
function names the function or kernel it mirrors; integer arithmetic is C's (all operands non-negative, so `//` is the same division).

What reading the launchers shows, and the sweep of tests/test_corr_plan.py confirms through the byte counts:
  * `window_plan` never launches an empty k-slice.  Its doubling loop may ask for more slices than `kper`-long pieces fit into N'
    (N' = 1985 .. 2016 at B = 1: 64 asked, kper 32), but the count it returns is recomputed as ceil(N' / kper): 63 slices, the
    last one 16 windows long.  The case `win_empty_last_slice` keeps its shape (N' = 2000): it is the trimmed plan, not an empty
    slice, and `(-inf, k_lo)` with k_lo >= N' is never written.
  * every instantiation of the file can be selected by a call: UNREACHABLE is empty.
"""

BM = BN = 128                                             # corr_argmax.hip: BM, BN
FBK = 16                                                  # FBK
PF = 4                                                    # PF
IC_MAX_BLOCKS, IC_FUSED_BLOCKS = 4096, 512                # innercos.hip: IC_MAX_BLOCKS, IC_FUSED_BLOCKS
IC_BWD_BLOCKS, IC_BWD_THREADS = 2048, 256                 # launch_innercos_backward


def align_up(x, a):
    return (x + a - 1) // a * a


def cdiv(a, b):
    return (a + b - 1) // b


# ---- the correlation ----------------------------------------------------------------------------------------------------------------
def corr_plan(B, N):
    """corr_argmax.hip `corr_plan` -> (qtiles, ktiles, ksplit, kt_per_wg, k-tiles of the last split).  A workgroup walks
    `kt_per_wg` k-tiles of 128 patches; the last split's `kt_hi = min(ktiles, ...)` (each kernel's decode) cuts it short when uneven."""
    qtiles, ktiles = cdiv(N, BN), cdiv(N, BM)
    base = B * qtiles
    best_cost, best = -1, ktiles
    for kpw in range(ktiles, 0, -1):
        ks = cdiv(ktiles, kpw)
        cost = cdiv(base * ks, 512) * (4 * kpw + 1)
        if best_cost < 0 or cost < best_cost:
            best_cost, best = cost, kpw
    ksplit = cdiv(ktiles, best)
    return qtiles, ktiles, ksplit, best, ktiles - (ksplit - 1) * best


def corr_ws(B, C, N):
    """`corr_argmax_ws_bytes` (`WsLayout::total` of `corr_plan`): the [B][ksplit][N] partial values and indices."""
    return 2 * align_up(B * corr_plan(B, N)[2] * N * 4, 256) + 256


def corr_bf16_ws(B, C, N, ld=0):
    """`bf16_plan`: the partials, then the two packed [C/8][ld][8] bf16 operands.  ld = N: `corr_argmax_bf16_ws_bytes` (the arg-max
    entry); ld = N rounded up to 128: `corr_R_bf16_ws_bytes` (the window path's R entry)."""
    if ld <= 0:
        ld = N
    return corr_ws(B, C, N) + 2 * align_up(B * ((C + 7) // 8) * ld * 16, 256)


def corr_bf16_supported(C, ld):
    """`corr_bf16_supported` with ld = N (the arg-max entry); with ld = N rounded up to 128 it is `corr_R_bf16_supported`, C alone."""
    return C % (16 * PF) == 0 and ld % BM == 0


def corr_variant(C, N, want_S):
    """`launch_corr_argmax`.  The alignment term is always true behind the entry points' own 16-byte check (`ipsr_corr_argmax`,
    `forward_impl`)."""
    fast = N % BM == 0 and C % FBK == 0
    return ("fast" if fast else "generic"), bool(want_S)


def corr_kernel_name(C, N, want_S):
    kind, S = corr_variant(C, N, want_S)
    s = "true" if S else "false"
    return "corr_argmax_fast_kernel<%s>" % s if kind == "fast" else "corr_argmax_kernel<%s>" % s


def fast_stages(C):
    """LDS stages of the fast kernel (`nstage`); its ring has 4 slots, 3 stages in flight (FNBUF, AHEAD)."""
    return C // FBK


# ---- the window arg-max of shift_sz > 1 ------------------------------------------------------------------------------------------
def window_split_sought(B, Np):
    """The doubling loop of `window_plan` alone: the power of two it stops at."""
    qblocks = cdiv(Np, 256) * B
    ks = 1
    while qblocks * ks < 1024 and ks < 64 and cdiv(Np, ks * 2) >= 32:
        ks *= 2
    return ks


def window_plan(B, Np):
    """`window_plan` -> (slices launched, kper, non-empty slices, length of the last non-empty one).  A slice s covers windows
    [s kper, min(N', (s + 1) kper)) (`window_corr_argmax_kernel`) and is empty when s kper >= N'."""
    kper = cdiv(Np, window_split_sought(B, Np))
    launched = cdiv(Np, kper)
    non_empty = sum(1 for s in range(launched) if s * kper < Np)
    return launched, kper, non_empty, Np - (non_empty - 1) * kper


def window_ws(B, Np):
    """`window_corr_ws_bytes` (`WsLayout::total` of `window_plan`): the partials of every launched slice, then the merged values and
    indices."""
    ks = window_plan(B, Np)[0]
    return 2 * align_up(B * ks * Np * 4, 256) + 2 * align_up(B * Np * 4, 256) + 256


def forward_ws(B, C, h, w, M, patch, corr_bf16):
    """api.hip `plan_forward`: the total of the layer's fifteen workspace slices.  `window_plan` is visible from the host
    only through the WS_RU slice of this sum."""
    K = C * patch * patch
    N = (h - patch + 1) * (w - patch + 1)
    hw = h * w
    win_bf16 = patch > 1 and corr_bf16
    Cp = (K + 7) & ~7
    Mc = (M + 31) & ~31 if M > 0 else 32
    Mx = M if M > 0 else 1
    if win_bf16:
        corr = corr_bf16_ws(B, C, hw, cdiv(hw, BM) * BM)                                  # corr_R_bf16_ws_bytes
    elif patch > 1:
        corr = corr_ws(B, C, hw)
    else:
        corr = corr_bf16_ws(B, K, N) if corr_bf16 else corr_ws(B, K, N)
    sz = [B * hw * hw * 4 if patch > 1 else B * K * N * 4,                                # WS_XN
          B * N * Cp * 4,                                                                 # WS_XT
          B * N * 4,                                                                      # WS_INV
          corr,                                                                           # WS_CORR
          B * Mx * 4, B * Mx * 4, B * Mx * 4, B * Mx * 4,                                 # WS_WN, WS_WO, WS_KQ, WS_JQ
          B * Mc * 4,                                                                     # WS_DLIST
          B * 4,                                                                          # WS_MPRIME
          B * N * 4,                                                                      # WS_RANKFLAG
          B * Mx * Mc * 4,                                                                # WS_AC
          B * hw * 4 if patch > 1 else 0,                                                 # WS_XU
          window_ws(B, N) if patch > 1 else 0,                                            # WS_RU
          B * K * N * 4 if patch > 1 else 0]                                              # WS_OU
    return 256 + sum(align_up(s, 256) for s in sz)


# ---- InnerCos and the index kernel ------------------------------------------------------------------------------------------------
def innercos_plan(B, Cuse, N, fused):
    """launch_innercos_loss without (two launches) / with a ticket (one launch) and the `(N & 3) == 0` of innercos_fused_kernel -> (vector,
    rows per block, blocks, rows of the last block)."""
    rows = B * Cuse
    rpb = cdiv(rows, IC_FUSED_BLOCKS if fused else IC_MAX_BLOCKS)
    blocks = cdiv(rows, rpb)
    return N % 4 == 0, rpb, blocks, rows - (blocks - 1) * rpb


def innercos_bwd_blocks(B, Cx, N):
    """launch_innercos_backward: the grid."""
    return min(IC_BWD_BLOCKS, cdiv(B * Cx * N, IC_BWD_THREADS))


def index_prep_chunks(h, w, patch, stride):
    """mask_ops.hip:84, :118: one workgroup walks the positions in chunks of 1024."""
    return cdiv(((h - patch) // stride + 1) * ((w - patch) // stride + 1), 1024)


# ---- the GPU cases and what they must reach ------------------------------------------------------------------------------------
# fp32 correlation through ops.patch_normalize -> ops.corr_argmax.  id: ((B, C, N), want_S, negative ref, order-rule data too,
# kernel, (ksplit, kt_per_wg, k-tiles of the last split))
CORR_CASES = {
    "fast_one_tile": ((1, 16, 128), True, False, False, "fast", (1, 1, 1)),                # one LDS stage: fewer than the 3 in flight
    "fast_two_stages": ((2, 32, 256), True, False, False, "fast", (2, 1, 1)),
    "fast_ring_exact": ((1, 48, 128), False, False, False, "fast", (1, 1, 1)),             # 3 stages: the prologue fills exactly
    "fast_ring_wraps": ((1, 80, 128), False, False, False, "fast", (1, 1, 1)),             # 5 stages: past the 4-slot ring
    "fast_kpw2_even": ((33, 16, 512), True, False, True, "fast", (2, 2, 2)),
    "fast_kpw2_uneven": ((57, 16, 384), False, False, False, "fast", (2, 2, 1)),
    "fast_kpw3_uneven": ((41, 16, 640), False, False, True, "fast", (2, 3, 2)),
    "fast_kpw4_four_splits": ((8, 16, 1792), False, False, False, "fast", (4, 4, 2)),
    "generic_single": ((1, 1, 1), True, False, False, "generic", (1, 1, 1)),
    "generic_tiny": ((2, 3, 5), True, False, False, "generic", (1, 1, 1)),
    "generic_c_ragged_full_tiles": ((1, 20, 256), True, False, False, "generic", (2, 1, 1)),
    "generic_n_ragged_negative": ((3, 16, 100), False, True, False, "generic", (1, 1, 1)),
    "generic_kpw2_even": ((33, 16, 484), True, False, True, "generic", (2, 2, 2)),
    "generic_kpw2_uneven": ((57, 20, 356), False, True, False, "generic", (2, 2, 1)),
    "generic_kpw3_uneven": ((41, 16, 612), False, False, True, "generic", (2, 3, 2)),
    "generic_kpw4": ((32, 16, 868), False, False, False, "generic", (2, 4, 3)),
}
FAST_STAGES = {"fast_one_tile": 1, "fast_two_stages": 2, "fast_ring_exact": 3, "fast_ring_wraps": 5}

# bf16 correlation through ops.corr_argmax(corr="bf16"), on small integers (exact on either matrix core).  Added to the issue's
# tables so that every reachable instantiation of the file has a case.  id: ((B, C, N), (ksplit, kt_per_wg, last))
BF16_CASES = {
    "bf16_one_tile": ((1, 64, 128), (1, 1, 1)),
    "bf16_kpw2_uneven": ((57, 64, 384), (2, 2, 1)),
}

# the whole layer, patch 1: the stage kernel folds the partials itself (merged_argmax).  id: ((B, C, h, w), kernel, (ks, kpw, last))
LAYER_CASES = {"layer_kpw2_in_consumer_merge": ((33, 16, 16, 32), "fast", (2, 2, 2))}

# ops.forward(patch = p).  id: ((B, C, h, w, p), N', window plan (launched, kper, non-empty, last length), bf16 correlation)
WINDOW_CASES = {
    "win_one_slice": ((1, 8, 8, 8, 3), 36, (1, 36, 1, 36), False),
    "win_two_slices_short_last": ((1, 8, 9, 11, 3), 63, (2, 32, 2, 31), False),
    "win_p2": ((1, 16, 8, 16, 2), 105, (2, 53, 2, 52), False),                             # h w = 128, C 16: fast WRITE_S under the stencil
    "win_16_slices": ((1, 8, 32, 32, 3), 900, (16, 57, 16, 45), False),                    # generic WRITE_S at 8 splits
    "win_batch_limited": ((32, 8, 32, 32, 3), 900, (8, 113, 8, 109), False),
    # the issue expected 64 launched / 63 non-empty here; the launcher trims the count itself (see the module docstring)
    "win_empty_last_slice": ((1, 8, 42, 52, 3), 2000, (63, 32, 63, 16), False),           # generic WRITE_S at 18 splits
    # bf16 1x1 correlation under the fp32 stencil, on small integers: h w a multiple of 128 or not
    "win_bf16_full_tiles": ((1, 64, 8, 16, 2), 105, (2, 53, 2, 52), True),
    "win_bf16_ragged": ((1, 64, 9, 11, 3), 63, (2, 32, 2, 31), True),
}
WINDOW_CORR_SPLITS = {"win_16_slices": 8, "win_empty_last_slice": 18}

# ops.innercos_loss / innercos_loss_backward.  id: ((B, Cx, Cuse, h, w), what it reaches)
IC_CASES = {
    "ic_scalar_small": ((2, 5, 5, 1, 3), dict(vector=False, rpb=1, blocks=10, last=1, fused_rpb=1, bwd_blocks=1)),
    "ic_vector_cx_wider": ((2, 12, 7, 2, 4), dict(vector=True, rpb=1, fused_rpb=1, bwd_blocks=1)),
    "ic_rpb2_ragged_scalar": ((17, 250, 241, 1, 5), dict(vector=False, rpb=2, blocks=2049, last=1, fused_rpb=9)),
    "ic_rpb2_ragged_vector": ((17, 241, 241, 2, 4), dict(vector=True, rpb=2, blocks=2049, last=1, fused_rpb=9)),
    # (the issue calls this one scalar; N = 460 = 4 x 115 takes the vector path)
    "ic_bwd_grid_stride": ((2, 600, 512, 20, 23), dict(vector=True, rpb=1, bwd_blocks=2048, bwd_strides=True)),
}

# ops.index_prep.  id: ((h, w), (patch, stride, mask_thred), 1024-chunks)
INDEX_PREP_CASES = {
    "ip_p1_s1_t1": ((13, 17), (1, 1, 1), 1),
    "ip_p2_s1_t2": ((13, 17), (2, 1, 2), 1),
    "ip_p3_s2_t1": ((13, 17), (3, 2, 1), 1),
    "ip_p3_s1_t9": ((13, 17), (3, 1, 9), 1),
    "ip_p4_s2_t16": ((13, 17), (4, 2, 16), 1),
    "ip_p2_s2_t4": ((13, 17), (2, 2, 4), 1),
    "ip_40x40_p3_s1_t5": ((40, 40), (3, 1, 5), 2),
}

ALL_TABLES = (CORR_CASES, BF16_CASES, LAYER_CASES, WINDOW_CASES, IC_CASES, INDEX_PREP_CASES)
ALL_CASE_IDS = tuple(cid for t in ALL_TABLES for cid in t)


def case_plan(cid):
    """What the restatement says a case reaches: a dict with `kernels` (the instantiations of corr_argmax.hip it launches) and the
    plan fields of its table."""
    if cid in CORR_CASES:
        (B, C, N), want_S = CORR_CASES[cid][:2]
        _, _, ks, kpw, last = corr_plan(B, N)
        return dict(kind=corr_variant(C, N, want_S)[0], want_S=want_S, split=(ks, kpw, last), stages=fast_stages(C),
                    kernels={corr_kernel_name(C, N, want_S), "argmax_merge_kernel"}, ws=corr_ws(B, C, N))
    if cid in BF16_CASES:
        B, C, N = BF16_CASES[cid][0]
        assert corr_bf16_supported(C, N)
        _, _, ks, kpw, last = corr_plan(B, N)
        return dict(kind="bf16", split=(ks, kpw, last), ws=corr_bf16_ws(B, C, N),
                    kernels={"pack_bf16_k8_kernel", "corr_argmax_bf16_kernel<false,false>", "argmax_merge_kernel"})
    if cid in LAYER_CASES:
        B, C, h, w = LAYER_CASES[cid][0]
        _, _, ks, kpw, last = corr_plan(B, h * w)
        return dict(kind=corr_variant(C, h * w, False)[0], split=(ks, kpw, last), stages=fast_stages(C), in_consumer_merge=True,
                    kernels={corr_kernel_name(C, h * w, False)})
    if cid in WINDOW_CASES:
        (B, C, h, w, p), _, _, bf16 = WINDOW_CASES[cid]
        Np = (h - p + 1) * (w - p + 1)
        hw = h * w
        if bf16:
            assert corr_bf16_supported(C, cdiv(hw, BM) * BM)
            under = {"pack_bf16_k8_kernel", "corr_argmax_bf16_kernel<%s,true>" % ("false" if hw % BM == 0 else "true")}
        else:
            under = {corr_kernel_name(C, hw, True)}
        launched, kper, non_empty, last = window_plan(B, Np)
        return dict(kind="window", Np=Np, window=(launched, kper, non_empty, last), sought=window_split_sought(B, Np),
                    corr_kind="bf16" if bf16 else corr_variant(C, hw, True)[0], corr_splits=corr_plan(B, hw)[2],
                    kernels=under | {"window_corr_argmax_kernel", "argmax_merge_kernel"})
    if cid in IC_CASES:
        B, Cx, Cuse, h, w = IC_CASES[cid][0]
        vec, rpb, blocks, last = innercos_plan(B, Cuse, h * w, False)
        nb = innercos_bwd_blocks(B, Cx, h * w)
        return dict(kind="innercos", vector=vec, rpb=rpb, blocks=blocks, last=last, fused_rpb=innercos_plan(B, Cuse, h * w, True)[1],
                    cx_wider=Cx > Cuse, bwd_blocks=nb, bwd_strides=B * Cx * h * w > nb * IC_BWD_THREADS, kernels=set())
    (h, w), (p, s, _), _ = INDEX_PREP_CASES[cid]
    return dict(kind="index_prep", chunks=index_prep_chunks(h, w, p, s), args=INDEX_PREP_CASES[cid][1], kernels=set())


def check_case(cid):
    """Assert that a case reaches the variant and plan written beside it -> its plan."""
    got = case_plan(cid)
    if cid in CORR_CASES:
        _, want_S, _, _, kind, split = CORR_CASES[cid]
        assert (got["kind"], got["want_S"], got["split"]) == (kind, want_S, split), (cid, got)
        assert got["stages"] == FAST_STAGES.get(cid, got["stages"]), (cid, got)
    elif cid in BF16_CASES:
        assert got["split"] == BF16_CASES[cid][1], (cid, got)
    elif cid in LAYER_CASES:
        assert (got["kind"], got["split"]) == LAYER_CASES[cid][1:], (cid, got)
    elif cid in WINDOW_CASES:
        _, Np, window, _ = WINDOW_CASES[cid]
        assert (got["Np"], got["window"]) == (Np, window), (cid, got)
        assert got["corr_splits"] == WINDOW_CORR_SPLITS.get(cid, got["corr_splits"]), (cid, got)
    elif cid in IC_CASES:
        want = IC_CASES[cid][1]
        miss = {k: (got[k], v) for k, v in want.items() if got[k] != v}
        assert not miss, "%s reaches another variant: (got, wanted) %s" % (cid, miss)
    else:
        assert got["chunks"] == INDEX_PREP_CASES[cid][2], (cid, got)
    return got


# ---- the instantiations of corr_argmax.hip ----------------------------------------------------------------------------------------
# (instantiation, selected at, case ids).  `case_plan(cid)["kernels"]` must hold the instantiation for each of its case ids.
REACHABLE = (
    ("corr_argmax_fast_kernel<false>", "launch_corr_argmax",
     ("fast_ring_exact", "fast_ring_wraps", "fast_kpw2_uneven", "fast_kpw3_uneven", "fast_kpw4_four_splits", "layer_kpw2_in_consumer_merge")),
    ("corr_argmax_fast_kernel<true>", "launch_corr_argmax", ("fast_one_tile", "fast_two_stages", "fast_kpw2_even", "win_p2")),
    ("corr_argmax_kernel<false>", "launch_corr_argmax",
     ("generic_n_ragged_negative", "generic_kpw2_uneven", "generic_kpw3_uneven", "generic_kpw4")),
    ("corr_argmax_kernel<true>", "launch_corr_argmax",
     ("generic_single", "generic_tiny", "generic_c_ragged_full_tiles", "generic_kpw2_even", "win_one_slice", "win_two_slices_short_last",
      "win_16_slices", "win_batch_limited", "win_empty_last_slice")),
    ("pack_bf16_k8_kernel", "launch_bf16", ("bf16_one_tile", "bf16_kpw2_uneven", "win_bf16_full_tiles", "win_bf16_ragged")),
    ("corr_argmax_bf16_kernel<false,false>", "launch_bf16 (launch_corr_argmax_bf16)", ("bf16_one_tile", "bf16_kpw2_uneven")),
    ("corr_argmax_bf16_kernel<false,true>", "launch_bf16 (launch_corr_R_bf16)", ("win_bf16_full_tiles",)),
    ("corr_argmax_bf16_kernel<true,true>", "launch_bf16 (launch_corr_R_bf16)", ("win_bf16_ragged",)),
    ("window_corr_argmax_kernel", "launch_window_corr_argmax", tuple(WINDOW_CASES)),
    ("argmax_merge_kernel", "finish_argmax", ("fast_kpw4_four_splits", "generic_kpw2_even", "bf16_kpw2_uneven", "win_16_slices")),
)
# (instantiation, why no call selects it): none.  The row stride that selected the RAGGED fast kernels and the RAGGED bf16 kernel
# without WRITE_S is gone from the launchers, and those instantiations with it.
UNREACHABLE = ()


# ---- plan-level rows of the variant table: (variant, selected at, predicate on a plan, case ids) -----------------------------------
def _split(kind, pred):
    return lambda p: p["kind"] == kind and "split" in p and pred(*p["split"])


def _ic(**want):
    return lambda p: p["kind"] == "innercos" and all(p[k] == v for k, v in want.items())


EDGES = (
    ("fast kernel: 1 / 2 LDS stages (fewer than the 3 in flight)", "corr_argmax_fast_kernel: prologue", lambda p: p["kind"] == "fast" and p["stages"] in (1, 2) and "want_S" in p,
     ("fast_one_tile", "fast_two_stages")),
    ("fast kernel: 3 and 5 stages (at and past the 4-slot ring)", "corr_argmax_fast_kernel: stage loop", lambda p: p["kind"] == "fast" and p["stages"] in (3, 5),
     ("fast_ring_exact", "fast_ring_wraps")),
    ("fast kernel: kt_per_wg == 1", "corr_plan", _split("fast", lambda ks, kpw, last: kpw == 1),
     ("fast_one_tile", "fast_two_stages", "fast_ring_exact", "fast_ring_wraps")),
    ("fast kernel: kt_per_wg >= 2, even last split", "corr_argmax_fast_kernel: kt_hi, k-tile loop", _split("fast", lambda ks, kpw, last: kpw >= 2 and last == kpw),
     ("fast_kpw2_even", "layer_kpw2_in_consumer_merge")),
    ("fast kernel: kt_per_wg >= 2, uneven last split", "corr_argmax_fast_kernel: kt_hi", _split("fast", lambda ks, kpw, last: kpw >= 2 and last < kpw),
     ("fast_kpw2_uneven", "fast_kpw3_uneven", "fast_kpw4_four_splits")),
    ("generic kernel: kt_per_wg == 1", "corr_plan", _split("generic", lambda ks, kpw, last: kpw == 1),
     ("generic_single", "generic_tiny", "generic_c_ragged_full_tiles", "generic_n_ragged_negative")),
    ("generic kernel: kt_per_wg >= 2, even last split", "corr_argmax_kernel: kt_hi, k-tile loop", _split("generic", lambda ks, kpw, last: kpw >= 2 and last == kpw),
     ("generic_kpw2_even",)),
    ("generic kernel: kt_per_wg >= 2, uneven last split", "corr_argmax_kernel: kt_hi", _split("generic", lambda ks, kpw, last: kpw >= 2 and last < kpw),
     ("generic_kpw2_uneven", "generic_kpw3_uneven", "generic_kpw4")),
    ("bf16 kernel: kt_per_wg >= 2, uneven last split", "corr_argmax_bf16_kernel: kt_hi, k-tile loop", _split("bf16", lambda ks, kpw, last: kpw >= 2 and last < kpw),
     ("bf16_kpw2_uneven",)),
    ("in-consumer merge of the partials (merged_argmax)", "merged_argmax, forward_impl", lambda p: p.get("in_consumer_merge", False),
     ("layer_kpw2_in_consumer_merge",)),
    ("window plan: one slice", "window_plan", lambda p: p["kind"] == "window" and p["window"][0] == 1, ("win_one_slice",)),
    ("window plan: every slice sought is launched, short last one", "window_plan", lambda p: p["kind"] == "window" and 1 < p["window"][0] == p["sought"] and p["window"][3] < p["window"][1],
     ("win_two_slices_short_last", "win_p2", "win_16_slices", "win_batch_limited", "win_bf16_full_tiles", "win_bf16_ragged")),
    ("window plan: split limited by the batch (8 < 16 slices)", "window_plan", lambda p: p["kind"] == "window" and p["Np"] == 900 and p["window"][0] == 8,
     ("win_batch_limited",)),
    ("window plan: 64 slices sought, 63 launched (none empty)", "window_plan", lambda p: p["kind"] == "window" and p["window"][0] < p["sought"] and p["window"][2] == p["window"][0],
     ("win_empty_last_slice",)),
    ("innercos_fused_kernel: scalar path (N % 4 != 0)", "innercos_fused_kernel: `(N & 3) == 0` else", _ic(vector=False), ("ic_scalar_small", "ic_rpb2_ragged_scalar")),
    ("innercos_fused_kernel: vector path", "innercos_fused_kernel: `(N & 3) == 0`", _ic(vector=True), ("ic_vector_cx_wider", "ic_rpb2_ragged_vector", "ic_bwd_grid_stride")),
    ("innercos_fused_kernel: two launches, 2 rows per block, last block 1 row", "launch_innercos_loss: rows per block", _ic(rpb=2, last=1),
     ("ic_rpb2_ragged_scalar", "ic_rpb2_ragged_vector")),
    ("innercos_fused_kernel: one launch, 9 rows per block", "launch_innercos_loss: with a ticket", _ic(fused_rpb=9), ("ic_rpb2_ragged_scalar", "ic_rpb2_ragged_vector")),
    ("innercos_backward_kernel: Cx > Cuse (zero-filled channels)", "innercos_backward_kernel: `c < Cuse`", _ic(cx_wider=True), ("ic_vector_cx_wider", "ic_rpb2_ragged_scalar", "ic_bwd_grid_stride")),
    ("innercos_backward_kernel: grid-stride loop (> 2048 x 256 elements)", "innercos_backward_kernel: stride loop", _ic(bwd_blocks=2048, bwd_strides=True), ("ic_bwd_grid_stride",)),
    ("index_prep_kernel: patch > 1, stride 2, threshold > 1", "mask_ops.hip:88-92, :118", lambda p: p["kind"] == "index_prep" and p["args"] != (1, 1, 1),
     ("ip_p2_s1_t2", "ip_p3_s2_t1", "ip_p3_s1_t9", "ip_p4_s2_t16", "ip_p2_s2_t4", "ip_40x40_p3_s1_t5")),
    ("index_prep_kernel: two 1024-chunks", "mask_ops.hip:84", lambda p: p["kind"] == "index_prep" and p["chunks"] == 2, ("ip_40x40_p3_s1_t5",)),
)


def variant_table():
    """The table of tests/test_gpu_corr_variants.py's docstring, generated (tests/test_corr_plan.py checks it is all there)."""
    rows = [(v, at, ", ".join(c)) for v, at, c in REACHABLE] + [(v, at, ", ".join(c)) for v, at, _, c in EDGES]
    w0, w1 = max(len(r[0]) for r in rows), max(len(r[1]) for r in rows)
    out = ["  %-*s  %-*s  case ids" % (w0, "variant", w1, "selected at"), "  %s  %s  %s" % ("-" * w0, "-" * w1, "-" * 40)]
    for v, at, cases in rows:
        ids = cases.split(", ")
        lines = [", ".join(ids[i:i + 3]) for i in range(0, len(ids), 3)]
        out.append("  %-*s  %-*s  %s" % (w0, v, w1, at, lines[0]))
        out.extend("  %-*s  %-*s  %s" % (w0, "", w1, "", ln) for ln in lines[1:])
    for v, why in UNREACHABLE:
        out.append("  unreachable: %s" % v)
        out.append("      %s" % why)
    return "\n".join(out)
