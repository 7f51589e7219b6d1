"""The two fp32 matrix-core launchers restated in Python: `sm_plan` of csrc/smallmap.hip (ipsr_conv_smallmap) and `make_plan` /
`choose_split` / `launch_conv_gemm` of csrc/conv_gemm.hip (ipsr_conv2d) — which kernel instantiation, grid, slab or split a shape reaches.

A plain module (like thin_conv_plan.py, bf16_conv_plan.py, guarded.py).  tests/test_fp32_conv_plan.py ties it to the built library
through the two workspace queries and proves that the case tables below reach every row of VARIANTS; tests/test_gpu_fp32_conv_variants.py
runs the tables.  Each function names the lines it mirrors; integer arithmetic is C's: every operand that is divided is non-negative, so `//` is the same
division, except in the output extent of a Conv2d, which `c_div` truncates as C does (see `conv_out_dim`).

A plan is a dict, `None` = the entry point refuses the shape (workspace query 0).  Pointer alignment and the limits of a grid axis are
not restated: no case comes near them.
"""

SM_DATA, SM_WRW, SM_FWD = 0, 1, 2                         # ops.py:1036
CONV_FWD, CONV_BWD_DATA, CONVT_FWD, CONVT_BWD_DATA = 0, 1, 2, 3
CG_BM, CG_BN, CG_NBUF = 128, 128, 4                       # conv_gemm.hip:36


def align_up(x, a):
    return (x + a - 1) // a * a


def cdiv(a, b):
    return (a + b - 1) // b


def c_div(a, b):
    """C's integer division (b > 0): towards zero."""
    return a // b if a >= 0 else -(-a // b)


def conv_out_dim(op, n, k, stride, pad, dil):
    """conv_gemm.hip:478-482 (`conv_out_dim`) and the grid check of `sm_plan` (smallmap.hip).  Where the window overhangs the padded input by less than the
    stride (span in -stride + 1 .. -1, e.g. k4 s2 p1 on a 1 x 1 map) C's division answers 1 where floor answers 0: both entry points
    serve that shape as one output position whose window is cut by the (bounds-checked) taps.  torch refuses such a module call, so the
    nets never get there; the mirror restates the library as it is."""
    if op in (CONV_FWD, CONV_BWD_DATA):
        return c_div(n + 2 * pad - dil * (k - 1) - 1, stride) + 1
    return (n - 1) * stride - 2 * pad + dil * (k - 1) + 1


# ---- ipsr_conv_smallmap ----------------------------------------------------------------------------------------------------------------
def _waves(total, per, nslab):
    """The reduction ranges [a, b) of the 4 * nslab waves (smallmap.hip: `ra` / `rb` of sm_data_kernel, `qa` / `qb` of sm_fwd_kernel): wave w of slab s starts at min(total, (4 s + w) per)."""
    out = []
    for i in range(4 * nslab):
        a = min(total, i * per)
        out.append((a, min(total, a + per)))
    return out


def _wave_facts(waves, per, group):
    """Short waves (range cut by the end of the reduction), idle ones (`ra == rb`), and whether some live wave's range is no multiple of
    the unroll group, i.e. the `ok` guard of a partly filled group fires (smallmap.hip: sm_data_kernel, sm_fwd_kernel, sm_wrw_kernel)."""
    lens = [b - a for a, b in waves]
    return dict(short_waves=sum(1 for n in lens if 0 < n < per), idle_waves=sum(1 for n in lens if n == 0),
                partial_group=any(n % group for n in lens if n), full_groups=any(n >= group for n in lens), group=group)


def sm_plan(op, B, R, Cq, Ho, Wo, Hf, Wf, k, st, pad, dil):
    """smallmap.hip: the argument check of ipsr_conv_smallmap_workspace_bytes and `sm_plan`; the kernel and grid of `launch_smallmap`."""
    if min(B, R, Cq, Ho, Wo, Hf, Wf) < 1 or op not in (SM_DATA, SM_WRW, SM_FWD):
        return None
    if k < 1 or k > 4 or st < 1 or st > 2 or dil < 1 or pad < 0:                          # sm_plan: k, stride, dilation, pad
        return None
    if Ho != conv_out_dim(CONV_FWD, Hf, k, st, pad, dil) or Wo != conv_out_dim(CONV_FWD, Wf, k, st, pad, dil):      # sm_plan: the output grid
        return None
    P, Q = B * Ho * Wo, Cq * k * k
    if Q % 128 != 0 or R % 32 != 0 or P > 1024:                                           # sm_plan: Q, R, P
        return None
    blocks = cdiv(P, 32)
    nb = 4 if blocks >= 3 else blocks                                                     # sm_plan: nb
    if op == SM_DATA and nb == 4:                                                         # sm_plan: nb of op 0
        nb = 2
    ngroups = cdiv(blocks, nb)
    Tp, Pp = ngroups * nb * 32, (P + 1) & ~1
    a_floats = b_floats = m_floats = 0
    nslab, per_slab = 1, 0
    w_bytes = R * Q * 4
    if op == SM_DATA:                                                                     # sm_plan: op 0
        qb = Q // 128
        cap = max(1, w_bytes // (Q * Tp * 4))
        ns = max(1, min(R // 64, cap, (256 + qb * ngroups - 1) // (qb * ngroups)))
        per_slab = (cdiv(R, 4 * ns) + 1) & ~1
        nslab = cdiv(R, 4 * per_slab)
        b_floats, m_floats = R * Tp, nslab * Q * Tp
        kernel, grid = "sm_data_kernel<%d>" % nb, (Q // 128, nslab, ngroups)
        waves = _waves(R, per_slab, nslab)
        facts = _wave_facts(waves, per_slab, 2 * {1: 8, 2: 4, 4: 2}[nb])                 # U of sm_data_kernel
    elif op == SM_FWD:                                                                    # sm_plan: op 2
        rb = R // 32
        cap = max(1, w_bytes // (R * Tp * 4))
        ns = max(1, min(Q // 256, cap, (256 + rb * ngroups - 1) // (rb * ngroups)))
        per_slab = (cdiv(Q, 4 * ns) + 7) & ~7
        nslab = cdiv(Q, 4 * per_slab)
        b_floats, m_floats = Q * Tp, nslab * R * Tp
        kernel, grid = "sm_fwd_kernel<%d>" % nb, (R // 32, nslab, ngroups)
        waves = _waves(Q, per_slab, nslab)
        facts = _wave_facts(waves, per_slab, 32)                                          # U of sm_fwd_kernel
    else:                                                                                 # sm_plan: op 1
        a_floats, b_floats = Pp * R, Pp * Q
        kernel, grid = "sm_wrw_kernel", (Q // 128, R // 32, 1)
        waves = [(0, Pp)]
        facts = _wave_facts(waves, Pp, 8)                                                 # sm_wrw_kernel
    ws = align_up(a_floats * 4, 256) + align_up(b_floats * 4, 256) + align_up(m_floats * 4, 256) + 256
    return dict(op=op, kernel=kernel, grid=grid, P=P, Q=Q, R=R, blocks=blocks, nb=nb, ngroups=ngroups, Tp=Tp, Pp=Pp, nslab=nslab, per_slab=per_slab,
                waves=waves, zero_blocks=Tp // 32 - blocks, padded_columns=Tp - P, zero_row=Pp - P, ws=ws, **facts)


def sm_ws(*a):
    p = sm_plan(*a)
    return 0 if p is None else p["ws"]


def sm_geometry(case):
    """(B, R, Cq, Ho, Wo, Hf, Wf, k, st, pad, dil) of ipsr_conv_smallmap for a module (kind, Ci, Co, H, W, k, s, p, d, B), as
    tests/test_gpu_conv.py:244-250 maps it: R and (Ho, Wo) are the weight's first channel dimension and the grid on its side."""
    kind, Ci, Co, H, W, k, st, pad, dil, B = case
    if kind == "convT":
        return (B, Ci, Co, H, W, conv_out_dim(CONVT_FWD, H, k, st, pad, dil), conv_out_dim(CONVT_FWD, W, k, st, pad, dil), k, st, pad, dil)
    return (B, Co, Ci, conv_out_dim(CONV_FWD, H, k, st, pad, dil), conv_out_dim(CONV_FWD, W, k, st, pad, dil), H, W, k, st, pad, dil)


# ---- ipsr_conv2d -------------------------------------------------------------------------------------------------------------------------
def axis_taps(k, stride, pad, dil, par):
    """conv_gemm.hip:320-328: the taps r of one axis that reach output parity `par` in the transposed form -> ([r], [offset])."""
    rr, off = [], []
    for r in range(k):
        v = par + pad - r * dil
        if v % stride == 0:                               # Python's % is the ((v % s) + s) % s of :325
            rr.append(r)
            off.append(v // stride)
    return rr, off


def choose_split(tiles, nstage):
    """conv_gemm.hip:330-337 -> (ksplit, stages_per_split)."""
    ks = 1
    while tiles * ks < 512 and nstage // (ks * 2) >= 8 and ks < 64:
        ks *= 2
    sps = cdiv(nstage, ks)
    return cdiv(nstage, sps), sps


def _progression(v):
    return all(v[a] - v[a - 1] == v[1] - v[0] for a in range(2, len(v)))


def conv_gemm_plan(transposed, B, Cred, M, Hin, Win, Hout, Wout, k, stride, pad, dil):
    """conv_gemm.hip:342-389 (`make_plan`) and the refusals and per-class launch of :413-468 (`launch_conv_gemm`)."""
    if B * Cred * Hin * Win * 4 + (k * dil + pad + 1) * (Win + 1) * 8 >= 1 << 31:        # :347
        return None
    Mp = align_up(M, CG_BM)
    m_tiles = Mp // CG_BM
    need_zero = False
    if not transposed or stride == 1:                                                     # :353-356
        classes = [dict(NT=k * k, Ho=Hout, Wo=Wout, py=0, px=0)]
    else:
        if stride != 2:                                                                   # :358
            return None
        classes = []
        for c in range(4):
            py, px = c >> 1, c & 1
            c = dict(NT=len(axis_taps(k, stride, pad, dil, py)[0]) * len(axis_taps(k, stride, pad, dil, px)[0]), py=py, px=px,
                     Ho=(Hout - py + 1) // 2, Wo=(Wout - px + 1) // 2)
            if c["NT"] == 0 and c["Ho"] > 0 and c["Wo"] > 0:                              # :367
                need_zero = True
            classes.append(c)
    off = part_floats = 0
    for c in classes:
        c.update(BK=0, nstage=0, ksplit=1, stages_per_split=0, live=False)
        if c["NT"] == 0 or c["Ho"] <= 0 or c["Wo"] <= 0:                                  # :372
            continue
        if c["NT"] not in (4, 9, 16):                                                     # :317, :373
            return None
        BK = 18 if c["NT"] == 9 else 16
        cps = BK // c["NT"]
        if Cred % cps != 0:                                                               # :376
            return None
        nstage = cdiv(Cred, cps)
        off += align_up(nstage * BK * Mp * 4, 256) // 4
        ntot = B * c["Ho"] * c["Wo"]
        n_tiles = cdiv(ntot, CG_BN)
        ksplit, sps = choose_split(n_tiles * m_tiles, nstage)                             # :380-381
        if ksplit > 1:
            part_floats = max(part_floats, ksplit * M * ntot)
        c.update(BK=BK, nstage=nstage, ksplit=ksplit, stages_per_split=sps, last_split_stages=nstage - (ksplit - 1) * sps, live=True, ntot=ntot,
                 n_tiles=n_tiles, last_n_pixels=ntot - (n_tiles - 1) * CG_BN, workgroups=m_tiles * n_tiles * ksplit)
        # the tap table of the launch, :418-439
        if not transposed:
            c.update(dy0=-pad, dys=dil, in_mul=stride)
        elif stride == 1:
            c.update(dy0=pad, dys=-dil, in_mul=1)
        else:
            (rr, ro), (sr, so) = axis_taps(k, stride, pad, dil, c["py"]), axis_taps(k, stride, pad, dil, c["px"])
            if not (_progression(rr) and _progression(ro) and _progression(sr) and _progression(so)):       # :430-433 "irregular tap set"
                return None
            if len(rr) != len(sr):                                                        # :434
                return None
            c.update(dy0=ro[0], dys=ro[1] - ro[0] if len(ro) > 1 else 0, dx0=so[0], dxs=so[1] - so[0] if len(so) > 1 else 0, in_mul=1)
    live = [c for c in classes if c["live"]]
    return dict(classes=classes, live=live, Mp=Mp, m_tiles=m_tiles, last_m_rows=M - (m_tiles - 1) * CG_BM, need_zero=need_zero,
                ws=off * 4 + align_up(part_floats * 4, 256) + 256,                        # :387
                # the summary a case requirement is written in: one entry per launched class, in launch order
                NT=tuple(c["NT"] for c in live), nstage=tuple(c["nstage"] for c in live), ksplit=tuple(c["ksplit"] for c in live),
                stages_per_split=tuple(c["stages_per_split"] for c in live), last_split_stages=tuple(c["last_split_stages"] for c in live),
                grids=tuple((c["Ho"], c["Wo"]) for c in live), n_tiles=tuple(c["n_tiles"] for c in live),
                last_n_pixels=tuple(c["last_n_pixels"] for c in live), workgroups=tuple(c["workgroups"] for c in live),
                empty_classes=sum(1 for c in classes if c["NT"] == 0))


def conv2d_plan(op, B, Cin, H, W, Cout, k, stride, pad, dil):
    """conv_gemm.hip:484-504 (`conv_args_ok`, `ipsr_conv2d_workspace_bytes`): the four ops in the terms of `make_plan`."""
    if op not in (0, 1, 2, 3) or min(B, Cin, Cout, H, W, k, stride, dil) < 1 or k > 4 or pad < 0:
        return None
    Ho, Wo = conv_out_dim(op, H, k, stride, pad, dil), conv_out_dim(op, W, k, stride, pad, dil)
    if Ho < 1 or Wo < 1:
        return None
    if op == CONV_FWD:
        return conv_gemm_plan(False, B, Cin, Cout, H, W, Ho, Wo, k, stride, pad, dil)
    if op == CONV_BWD_DATA:
        return conv_gemm_plan(True, B, Cout, Cin, Ho, Wo, H, W, k, stride, pad, dil)
    if op == CONVT_FWD:
        return conv_gemm_plan(True, B, Cin, Cout, H, W, Ho, Wo, k, stride, pad, dil)
    return conv_gemm_plan(False, B, Cout, Cin, Ho, Wo, H, W, k, stride, pad, dil)


def conv2d_ws(*a):
    p = conv2d_plan(*a)
    return 0 if p is None else p["ws"]


# ---- the GPU cases and the paths they must reach ------------------------------------------------------------------------------------
# A requirement is a dict of plan fields that must match exactly.
#
# ops.conv_smallmap.  id: ((kind, Ci, Co, H, W, k, s, p, d, B) of the module, {op: requirement}); all three ops run per case.
D, WG, FW = SM_DATA, SM_WRW, SM_FWD
SM_CASES = {
    "conv8_32_12x12_k4s2_b2": (("conv", 8, 32, 12, 12, 4, 2, 1, 1, 2), {
        D: dict(P=72, blocks=3, nb=2, ngroups=2, zero_blocks=1), FW: dict(nb=4, ngroups=1, zero_blocks=1, padded_columns=56), WG: dict(Pp=72)}),
    "conv8_32_18x14_k4s2_b2": (("conv", 8, 32, 18, 14, 4, 2, 1, 1, 2), {
        D: dict(P=126, nb=2, ngroups=2, zero_blocks=0), FW: dict(kernel="sm_fwd_kernel<4>", ngroups=1, padded_columns=2), WG: dict(Pp=126)}),
    "conv8_32_20x20_k4s2_b2": (("conv", 8, 32, 20, 20, 4, 2, 1, 1, 2), {
        D: dict(P=200, ngroups=4), FW: dict(nb=4, ngroups=2, zero_blocks=1), WG: dict(Pp=200)}),
    "conv8_64_32x32_k4s2_b4": (("conv", 8, 64, 32, 32, 4, 2, 1, 1, 4), {
        D: dict(P=1024, ngroups=16, padded_columns=0), FW: dict(nb=4, ngroups=8, padded_columns=0), WG: dict(Pp=1024, partial_group=False)}),
    "conv8_224_6x6_k4s2_b1": (("conv", 8, 224, 6, 6, 4, 2, 1, 1, 1), {
        D: dict(P=9, nb=1, nslab=3, per_slab=20, short_waves=1, idle_waves=0, partial_group=True), FW: dict(nb=1, nslab=1, per_slab=32),
        WG: dict(Pp=10, zero_row=1, partial_group=True)}),
    "convT224_8_3x3_k4s2_b1": (("convT", 224, 8, 3, 3, 4, 2, 1, 1, 1), {
        D: dict(P=9, nb=1, nslab=3, per_slab=20, short_waves=1, partial_group=True), FW: dict(nb=1, nslab=1, per_slab=32),
        WG: dict(Pp=10, zero_row=1)}),
    "conv128_96_3x3_k3s1_b1": (("conv", 128, 96, 3, 3, 3, 1, 1, 1, 1), {
        D: dict(P=9, Q=1152, nb=1, per_slab=24, nslab=1, partial_group=True, full_groups=True), FW: dict(per_slab=72, nslab=4, partial_group=True, short_waves=0),
        WG: dict(Pp=10, zero_row=1)}),
    "conv32_160_5x5_k4s1_b3": (("conv", 32, 160, 5, 5, 4, 1, 1, 1, 3), {
        D: dict(P=48, nb=2, per_slab=20, nslab=2, partial_group=True), FW: dict(nb=2, partial_group=False), WG: dict(Pp=48, partial_group=False)}),
    "conv24_32_8x8_k4s2_b1": (("conv", 24, 32, 8, 8, 4, 2, 1, 1, 1), {
        D: dict(P=16, nb=1, per_slab=8, nslab=1, partial_group=True, full_groups=False), FW: dict(per_slab=96, nslab=1, partial_group=False), WG: dict(Pp=16)}),
    # added to the issue's list: a short wave (48 of 72 columns: one full unroll group and a partly filled one) and an idle wave in FWD
    "conv120_32_8x8_k4s2_b1": (("conv", 120, 32, 8, 8, 4, 2, 1, 1, 1), {
        D: dict(P=16, Q=1920, per_slab=8), FW: dict(per_slab=72, nslab=7, short_waves=1, idle_waves=1, partial_group=True), WG: dict(Pp=16)}),
}
# refused by all three ops: P = 4 * 16 * 17 = 1088 > 1024
SM_REFUSED = {"conv8_32_32x34_k4s2_b4": ("conv", 8, 32, 32, 34, 4, 2, 1, 1, 4)}
# the most ragged case of each op, run once more inside guard bands
SM_GUARDED = {D: "conv8_224_6x6_k4s2_b1", FW: "conv120_32_8x8_k4s2_b1", WG: "conv8_224_6x6_k4s2_b1"}
SM_OP_NAME = {D: "data", WG: "wrw", FW: "fwd"}

# ops.conv2d.  id: ((kind, Cin, H, W, Cout, k, s, p, d, B) of the module, in the order of GEOMS of tests/test_gpu_conv.py plus B,
# {"fwd" | "bwd": requirement}).  "fwd" is op 0 (Conv2d) / op 2 (ConvTranspose2d), "bwd" op 1 / op 3; the passes named in the
# requirement dict run (the other pass of a header cross-check is the transposed form, which CG_REFUSED covers where it is refused).
CG_CASES = {
    # stage counts 1, 2, 3, 5 (the first wrap of the 4-slot ring) and 15 without split-K: NT = 9 (two channels per stage)
    "conv2_9x7_c5_k3_b1": (("conv", 2, 9, 7, 5, 3, 1, 1, 1, 1), dict(fwd=dict(NT=(9,), nstage=(1,), ksplit=(1,), n_tiles=(1,), last_n_pixels=(63,), last_m_rows=5))),
    "conv4_9x7_c6_k3_b2": (("conv", 4, 9, 7, 6, 3, 1, 1, 1, 2), dict(fwd=dict(NT=(9,), nstage=(2,), ksplit=(1,), last_n_pixels=(126,)), bwd=dict(NT=(9,), nstage=(3,)))),
    "conv6_11x13_c10_k3_b3": (("conv", 6, 11, 13, 10, 3, 1, 1, 1, 3), dict(fwd=dict(NT=(9,), nstage=(3,), n_tiles=(4,), last_n_pixels=(45,), workgroups=(4,)),
                                                                         bwd=dict(NT=(9,), nstage=(5,)))),
    "conv10_5x6_c30_k3_b1": (("conv", 10, 5, 6, 30, 3, 1, 1, 1, 1), dict(fwd=dict(nstage=(5,), ksplit=(1,)), bwd=dict(nstage=(15,), ksplit=(1,)))),
    "convT30_5x6_c2_k3_b2": (("convT", 30, 5, 6, 2, 3, 1, 1, 1, 2), dict(fwd=dict(NT=(9,), nstage=(15,), ksplit=(1,)), bwd=dict(NT=(9,), nstage=(1,)))),
    # NT = 16 (one channel per stage), k4 stride 2 direct; the input gradients are the 2 x 2 parity classes (NT = 4, four channels per stage)
    "conv1_12x10_c4_k4s2_b2": (("conv", 1, 12, 10, 4, 4, 2, 1, 1, 2), dict(fwd=dict(NT=(16,), nstage=(1,)), bwd=dict(NT=(4, 4, 4, 4), nstage=(1, 1, 1, 1)))),
    "conv2_12x10_c8_k4s2_b1": (("conv", 2, 12, 10, 8, 4, 2, 1, 1, 1), dict(fwd=dict(NT=(16,), nstage=(2,)), bwd=dict(NT=(4, 4, 4, 4), nstage=(2, 2, 2, 2)))),
    "conv3_9x11_c12_k4s2_b3": (("conv", 3, 9, 11, 12, 4, 2, 1, 1, 3), dict(fwd=dict(NT=(16,), nstage=(3,)),
                                                                         bwd=dict(nstage=(3, 3, 3, 3), grids=((5, 6), (5, 5), (4, 6), (4, 5))))),
    "conv5_8x8_c20_k4s2_b1": (("conv", 5, 8, 8, 20, 4, 2, 1, 1, 1), dict(fwd=dict(NT=(16,), nstage=(5,)), bwd=dict(nstage=(5, 5, 5, 5)))),
    "conv15_6x6_c60_k4s2_b1": (("conv", 15, 6, 6, 60, 4, 2, 1, 1, 1), dict(fwd=dict(NT=(16,), nstage=(15,), ksplit=(1,)), bwd=dict(nstage=(15,) * 4, ksplit=(1,) * 4))),
    # ConvTranspose2d k4 s2 p1: the forward is the parity form, on odd output extents four different grids
    "convT4_4x6_c3_k4s2_b1": (("convT", 4, 4, 6, 3, 4, 2, 1, 1, 1), dict(fwd=dict(NT=(4, 4, 4, 4), nstage=(1,) * 4), bwd=dict(NT=(16,), nstage=(3,)))),
    "convT8_5x3_c5_k4s2_b2": (("convT", 8, 5, 3, 5, 4, 2, 1, 1, 2), dict(fwd=dict(nstage=(2,) * 4), bwd=dict(NT=(16,), nstage=(5,)))),
    "convT12_3x5_c2_k4s2_b3": (("convT", 12, 3, 5, 2, 4, 2, 1, 1, 3), dict(fwd=dict(nstage=(3,) * 4), bwd=dict(NT=(16,), nstage=(2,)))),
    "convT20_6x4_c1_k4s2_b1": (("convT", 20, 6, 4, 1, 4, 2, 1, 1, 1), dict(fwd=dict(nstage=(5,) * 4, last_m_rows=1), bwd=dict(NT=(16,), nstage=(1,)))),
    "convT60_2x3_c4_k4s2_b2": (("convT", 60, 2, 3, 4, 4, 2, 1, 1, 2), dict(fwd=dict(nstage=(15,) * 4, ksplit=(1,) * 4), bwd=dict(NT=(16,), nstage=(4,)))),
    # split-K: two even splits; eight splits, the last of 2 stages (the existing shape of GEOMS); two m tiles, the second with 8 live rows
    "conv32_6x5_c136_k3_b2": (("conv", 32, 6, 5, 136, 3, 1, 1, 1, 2), dict(
        fwd=dict(nstage=(16,), ksplit=(2,), stages_per_split=(8,), last_split_stages=(8,), m_tiles=2, last_m_rows=8, workgroups=(4,)),
        bwd=dict(nstage=(68,), ksplit=(8,), stages_per_split=(9,), last_split_stages=(5,), m_tiles=1))),
    "conv130_9x13_c70_k3_b3": (("conv", 130, 9, 13, 70, 3, 1, 1, 1, 3), dict(
        fwd=dict(nstage=(65,), ksplit=(8,), stages_per_split=(9,), last_split_stages=(2,), n_tiles=(3,), last_n_pixels=(95,), workgroups=(24,)),
        bwd=dict(nstage=(35,), ksplit=(4,), stages_per_split=(9,), last_split_stages=(8,)))),
    "conv17_5x5_c136_k4s1_b1": (("conv", 17, 5, 5, 136, 4, 1, 1, 1, 1), dict(
        fwd=dict(NT=(16,), nstage=(17,), ksplit=(2,), stages_per_split=(9,), last_split_stages=(8,), m_tiles=2, last_m_rows=8),
        bwd=dict(NT=(16,), nstage=(136,), ksplit=(16,), stages_per_split=(9,), last_split_stages=(1,)))),
    # tiles: several pixel tiles with a ragged last one, a grid that is no multiple of 8 workgroups
    "conv4_24x23_c136_k3_b3": (("conv", 4, 24, 23, 136, 3, 1, 1, 1, 3), dict(
        fwd=dict(m_tiles=2, last_m_rows=8, n_tiles=(13,), last_n_pixels=(120,), workgroups=(26,), ksplit=(1,)), bwd=dict(nstage=(68,), workgroups=(104,)))),
    # parity classes: odd output extents (four grids), classes without taps (need_zero), down to the 2 x 2 map
    "conv4_21x19_c8_k4s2_b2": (("conv", 4, 21, 19, 8, 4, 2, 1, 1, 2), dict(fwd=dict(NT=(16,), grids=((10, 9),)),
                                                                         bwd=dict(NT=(4,) * 4, nstage=(2,) * 4, grids=((11, 10), (11, 9), (10, 10), (10, 9)), need_zero=False))),
    "conv3_12x10_c5_k4s2p3d2_b2": (("conv", 3, 12, 10, 5, 4, 2, 3, 2, 2), dict(fwd=dict(NT=(16,), nstage=(3,)),
                                                                             bwd=dict(NT=(16,), need_zero=True, empty_classes=3, grids=((6, 5),), nstage=(5,)))),
    "conv3_2x2_c5_k4s2p3d2_b3": (("conv", 3, 2, 2, 5, 4, 2, 3, 2, 3), dict(fwd=dict(NT=(16,), grids=((1, 1),)), bwd=dict(NT=(16,), need_zero=True, grids=((1, 1),)))),
    # the header's sentences: k = 2 and stride 3 on the direct forms, dilation 3 on the stride-2 transposed forms
    "conv4_9x8_c8_k2s1_b2": (("conv", 4, 9, 8, 8, 2, 1, 0, 1, 2), dict(fwd=dict(NT=(4,), nstage=(1,)), bwd=dict(NT=(4,), nstage=(2,), grids=((9, 8),)))),
    "conv8_9x8_c6_k2s2p1_b1": (("conv", 8, 9, 8, 6, 2, 2, 1, 1, 1), dict(fwd=dict(NT=(4,), nstage=(2,)))),
    "convT6_5x4_c12_k2s2_b2": (("convT", 6, 5, 4, 12, 2, 2, 0, 1, 2), dict(bwd=dict(NT=(4,), nstage=(3,)))),
    "conv4_13x11_c6_k3s3_b2": (("conv", 4, 13, 11, 6, 3, 3, 1, 1, 2), dict(fwd=dict(NT=(9,), nstage=(2,), grids=((5, 4),)))),
    "conv3_13x11_c6_k4s3p2_b1": (("conv", 3, 13, 11, 6, 4, 3, 2, 1, 1), dict(fwd=dict(NT=(16,), nstage=(3,), grids=((5, 4),)))),
    "convT6_4x5_c3_k4s3_b2": (("convT", 6, 4, 5, 3, 4, 3, 1, 1, 2), dict(bwd=dict(NT=(16,), nstage=(3,)))),
    "conv8_15x13_c4_k4s2p1d3_b2": (("conv", 8, 15, 13, 4, 4, 2, 1, 3, 2), dict(fwd=dict(NT=(16,), nstage=(8,)), bwd=dict(NT=(4,) * 4, nstage=(1,) * 4, need_zero=False))),
    # even dilation on the stride-2 transposed forms puts all k * k taps of k = 2, 3 into one parity class too (the rest of dx is zero)
    "conv6_9x8_c4_k3s2p2d2_b2": (("conv", 6, 9, 8, 4, 3, 2, 2, 2, 2), dict(fwd=dict(NT=(9,), nstage=(3,), grids=((5, 4),)),
                                                                         bwd=dict(NT=(9,), nstage=(2,), need_zero=True, empty_classes=3, grids=((5, 4),)))),
    "conv4_9x8_c8_k2s2p1d2_b1": (("conv", 4, 9, 8, 8, 2, 2, 1, 2, 1), dict(fwd=dict(NT=(4,), nstage=(1,), grids=((5, 4),)),
                                                                         bwd=dict(NT=(4,), nstage=(2,), need_zero=True, empty_classes=3, grids=((4, 4),)))),
    "convT8_4x3_c4_k4s2p1d3_b1": (("convT", 8, 4, 3, 4, 4, 2, 1, 3, 1), dict(fwd=dict(NT=(4,) * 4, nstage=(2,) * 4), bwd=dict(NT=(16,), nstage=(4,)))),
}
# refused: id -> ((kind, Cin, H, W, Cout, k, s, p, d, B), the refused passes, the refusing line)
CG_REFUSED = {
    "conv4_8x8_c4_k3s2_bwd": (("conv", 4, 8, 8, 4, 3, 2, 1, 1, 1), ("bwd",), "k3 s2 transposed: one or two taps in a parity class"),
    "convT4_4x4_c4_k3s2_fwd": (("convT", 4, 4, 4, 4, 3, 2, 1, 1, 1), ("fwd",), "k3 s2 transposed: one or two taps in a parity class"),
    "conv4_6x6_c4_k1": (("conv", 4, 6, 6, 4, 1, 1, 0, 1, 1), ("fwd", "bwd"), "k = 1: one tap"),
    "conv3_6x6_c4_k3_odd": (("conv", 3, 6, 6, 4, 3, 1, 1, 1, 1), ("fwd",), "k3: odd reduction channels"),
    "conv4_6x6_c3_k3_odd": (("conv", 4, 6, 6, 3, 3, 1, 1, 1, 1), ("bwd",), "k3: odd reduction channels"),
    "convT6_4x4_c4_k4s2_mod4": (("convT", 6, 4, 4, 4, 4, 2, 1, 1, 1), ("fwd",), "4-tap classes: reduction channels no multiple of 4"),
    "conv4_8x8_c6_k4s2_mod4": (("conv", 4, 8, 8, 6, 4, 2, 1, 1, 1), ("bwd",), "4-tap classes: reduction channels no multiple of 4"),
    "conv6_9x8_c6_k2_mod4": (("conv", 6, 9, 8, 6, 2, 1, 0, 1, 1), ("fwd",), "k2 direct: reduction channels no multiple of 4"),
    "conv4_13x11_c4_k4s3_bwd": (("conv", 4, 13, 11, 4, 4, 3, 1, 1, 1), ("bwd",), "stride 3 transposed"),
    "convT4_4x5_c4_k4s3_fwd": (("convT", 4, 4, 5, 4, 4, 3, 1, 1, 1), ("fwd",), "stride 3 transposed"),
}
# the most ragged case of each op, run once more inside guard bands
CG_GUARDED = {0: "conv6_11x13_c10_k3_b3", 1: "conv4_21x19_c8_k4s2_b2", 2: "convT8_5x3_c5_k4s2_b2", 3: "convT6_4x5_c3_k4s3_b2"}


def cg_ops(kind):
    """{"fwd": op, "bwd": op} of ipsr_conv2d for a module kind."""
    return dict(fwd=CONVT_FWD, bwd=CONVT_BWD_DATA) if kind == "convT" else dict(fwd=CONV_FWD, bwd=CONV_BWD_DATA)


def cg_args(case, which):
    """(op, B, Cin, H, W, Cout, k, stride, pad, dil) of ipsr_conv2d for a CG case and "fwd" | "bwd"."""
    kind, Cin, H, W, Cout, k, st, pad, dil, B = case
    return (cg_ops(kind)[which], B, Cin, H, W, Cout, k, st, pad, dil)


def case_plan(pid):
    """The plan of "case id:pass", pass = data | wrw | fwd for a small-map case and fwd | bwd for an implicit-GEMM one."""
    cid, which = pid.split(":")
    if cid in SM_CASES or cid in SM_REFUSED:
        case = SM_CASES[cid][0] if cid in SM_CASES else SM_REFUSED[cid]
        return sm_plan({v: k for k, v in SM_OP_NAME.items()}[which], *sm_geometry(case))
    case = CG_CASES[cid][0] if cid in CG_CASES else CG_REFUSED[cid][0]
    return conv2d_plan(*cg_args(case, which))


ALL_PLAN_IDS = tuple("%s:%s" % (cid, SM_OP_NAME[op]) for cid, (_, req) in SM_CASES.items() for op in req) + \
    tuple("%s:%s" % (cid, which) for cid, (_, req) in CG_CASES.items() for which in req)


def check_case(pid):
    """Assert that a case's pass reaches the path written beside it -> its plan."""
    cid, which = pid.split(":")
    if cid in SM_CASES:
        want = SM_CASES[cid][1][{v: k for k, v in SM_OP_NAME.items()}[which]]
    else:
        want = CG_CASES[cid][1][which]
    got = case_plan(pid)
    assert got is not None, "%s: refused" % pid
    miss = {k: (got.get(k), v) for k, v in want.items() if got.get(k) != v}
    assert not miss, "%s reaches another variant: (got, wanted) %s" % (pid, miss)
    return got


# ---- the variant table: (variant, selecting lines, predicate on a plan, "case id:pass" that reach it) -------------------------------------
def _sm(op, **kw):
    return lambda p: "classes" not in p and p["op"] == op and all(p[k] == v for k, v in kw.items())


def _cg(f):
    """A predicate over the launched classes of an implicit-GEMM plan: true when some class satisfies `f(class, plan)`."""
    return lambda p: "classes" in p and any(f(c, p) for c in p["live"])


def _stages(NT, n):
    """Workgroups of exactly `n` stages on the NT-tap kernel (no split-K: the prologue and ring see all n)."""
    return _cg(lambda c, p: c["NT"] == NT and c["ksplit"] == 1 and c["nstage"] == n)


_S, _G = "smallmap.hip", "conv_gemm.hip"
VARIANTS = (
    ("sm_data_kernel<1>", _S + ": sm_plan nb, launch_smallmap", _sm(D, nb=1), ("conv8_224_6x6_k4s2_b1:data", "conv24_32_8x8_k4s2_b1:data")),
    ("sm_data_kernel<2>, one group", _S + ": sm_plan nb (DATA), launch_smallmap", _sm(D, nb=2, ngroups=1), ("conv32_160_5x5_k4s1_b3:data",)),
    ("sm_data_kernel<2>: blockIdx.z > 0, the last group half zero blocks", _S + ": sm_plan ngroups, sm_data_kernel", lambda p: _sm(D, nb=2)(p) and p["ngroups"] >= 2 and p["zero_blocks"] == 1,
     ("conv8_32_12x12_k4s2_b2:data", "conv8_32_20x20_k4s2_b2:data")),
    ("sm_data_kernel<2>: blockIdx.z > 0, a ragged last block", _S + ": sm_plan ngroups, sm_data_kernel", lambda p: _sm(D, nb=2)(p) and p["ngroups"] >= 2 and p["P"] % 32 != 0,
     ("conv8_32_18x14_k4s2_b2:data", "conv8_32_12x12_k4s2_b2:data")),
    ("sm_data_kernel<2>: 16 groups at the limit of 1024 positions", _S + ": sm_plan, P > 1024", _sm(D, P=1024, ngroups=16), ("conv8_64_32x32_k4s2_b4:data",)),
    ("sm_data_kernel: three slabs, a short wave (4 of 20 rows)", _S + ": sm_plan slabs, sm_data_kernel", lambda p: _sm(D, nslab=3, per_slab=20, short_waves=1)(p),
     ("conv8_224_6x6_k4s2_b1:data", "convT224_8_3x3_k4s2_b1:data")),
    ("sm_data_kernel<1>: a full unroll group and a partly filled one", _S + ": sm_data_kernel unroll loop", lambda p: _sm(D, nb=1, partial_group=True, full_groups=True)(p),
     ("conv128_96_3x3_k3s1_b1:data", "conv8_224_6x6_k4s2_b1:data")),
    ("sm_data_kernel<1>: half an unroll group only", _S + ": sm_data_kernel unroll loop", _sm(D, nb=1, per_slab=8, full_groups=False), ("conv24_32_8x8_k4s2_b1:data", "conv120_32_8x8_k4s2_b1:data")),
    ("sm_data_kernel<2>: a partly filled unroll group", _S + ": sm_data_kernel unroll loop", _sm(D, nb=2, partial_group=True), ("conv32_160_5x5_k4s1_b3:data",)),
    ("sm_fwd_kernel<1>", _S + ": sm_plan nb, launch_smallmap", _sm(FW, nb=1), ("conv8_224_6x6_k4s2_b1:fwd", "conv24_32_8x8_k4s2_b1:fwd")),
    ("sm_fwd_kernel<2>", _S + ": sm_plan nb, launch_smallmap", _sm(FW, nb=2), ("conv32_160_5x5_k4s1_b3:fwd",)),
    ("sm_fwd_kernel<4> with one all-zero block (three position blocks)", _S + ": sm_plan nb, launch_smallmap", _sm(FW, nb=4, blocks=3, zero_blocks=1), ("conv8_32_12x12_k4s2_b2:fwd",)),
    ("sm_fwd_kernel<4> with a ragged last block", _S + ": sm_plan nb, launch_smallmap", _sm(FW, nb=4, blocks=4, padded_columns=2), ("conv8_32_18x14_k4s2_b2:fwd",)),
    ("sm_fwd_kernel<4>: blockIdx.z > 0", _S + ": sm_plan ngroups, sm_fwd_kernel", lambda p: _sm(FW, nb=4)(p) and p["ngroups"] >= 2, ("conv8_32_20x20_k4s2_b2:fwd", "conv8_64_32x32_k4s2_b4:fwd")),
    ("sm_fwd_kernel<4>: 8 groups at the limit of 1024 positions", _S + ": sm_plan, P > 1024", _sm(FW, P=1024, ngroups=8), ("conv8_64_32x32_k4s2_b4:fwd",)),
    ("sm_fwd_kernel: four slabs of 72 columns (two groups and one 8-column step over)", _S + ": sm_plan slabs, sm_fwd_kernel `ok`", _sm(FW, per_slab=72, nslab=4, partial_group=True),
     ("conv128_96_3x3_k3s1_b1:fwd",)),
    ("sm_fwd_kernel: a short wave and an idle wave (`qa == qb`)", _S + ": sm_plan slabs, sm_fwd_kernel", lambda p: _sm(FW)(p) and p["short_waves"] >= 1 and p["idle_waves"] >= 1,
     ("conv120_32_8x8_k4s2_b1:fwd",)),
    ("sm_wrw_kernel: odd P, the zero row of Pp is read", _S + ": sm_plan Pp, launch_smallmap", lambda p: _sm(WG)(p) and p["zero_row"] == 1,
     ("conv8_224_6x6_k4s2_b1:wrw", "convT224_8_3x3_k4s2_b1:wrw", "conv128_96_3x3_k3s1_b1:wrw")),
    ("sm_wrw_kernel: a partly filled unroll group (Pp % 8 != 0)", _S + ": sm_wrw_kernel unroll loop", _sm(WG, partial_group=True),
     ("conv8_224_6x6_k4s2_b1:wrw", "conv8_32_18x14_k4s2_b2:wrw")),
    ("sm_wrw_kernel: 1024 positions", _S + ": sm_plan, P > 1024", _sm(WG, Pp=1024), ("conv8_64_32x32_k4s2_b4:wrw",)),
    ("sm_wrw_kernel: more than one block on x and y", _S + ": launch_smallmap, op 1 grid", lambda p: _sm(WG)(p) and p["grid"][0] >= 2 and p["grid"][1] >= 2,
     ("conv128_96_3x3_k3s1_b1:wrw", "conv32_160_5x5_k4s1_b3:wrw")),
    ("conv_gemm_kernel<9>: 1 stage", _G + ":180-184", _stages(9, 1), ("conv2_9x7_c5_k3_b1:fwd", "convT30_5x6_c2_k3_b2:bwd")),
    ("conv_gemm_kernel<9>: 2 stages", _G + ":181", _stages(9, 2), ("conv4_9x7_c6_k3_b2:fwd", "conv4_13x11_c6_k3s3_b2:fwd")),
    ("conv_gemm_kernel<9>: 3 stages", _G + ":182", _stages(9, 3), ("conv6_11x13_c10_k3_b3:fwd", "conv4_9x7_c6_k3_b2:bwd")),
    ("conv_gemm_kernel<9>: 5 stages, the ring wraps", _G + ":156, :193", _stages(9, 5), ("conv10_5x6_c30_k3_b1:fwd", "conv6_11x13_c10_k3_b3:bwd")),
    ("conv_gemm_kernel<9>: 15 stages", _G + ":334", _stages(9, 15), ("conv10_5x6_c30_k3_b1:bwd", "convT30_5x6_c2_k3_b2:fwd")),
    ("conv_gemm_kernel<16>: 1 stage", _G + ":180-184", _stages(16, 1), ("conv1_12x10_c4_k4s2_b2:fwd", "convT20_6x4_c1_k4s2_b1:bwd")),
    ("conv_gemm_kernel<16>: 2 stages", _G + ":181", _stages(16, 2), ("conv2_12x10_c8_k4s2_b1:fwd", "convT12_3x5_c2_k4s2_b3:bwd")),
    ("conv_gemm_kernel<16>: 3 stages", _G + ":182", _stages(16, 3), ("conv3_9x11_c12_k4s2_b3:fwd", "convT4_4x6_c3_k4s2_b1:bwd")),
    ("conv_gemm_kernel<16>: 5 stages, the ring wraps", _G + ":156, :193", _stages(16, 5), ("conv5_8x8_c20_k4s2_b1:fwd", "convT8_5x3_c5_k4s2_b2:bwd")),
    ("conv_gemm_kernel<16>: 15 stages", _G + ":334", _stages(16, 15), ("conv15_6x6_c60_k4s2_b1:fwd",)),
    ("conv_gemm_kernel<4>: 1 stage", _G + ":180-184", _stages(4, 1), ("conv1_12x10_c4_k4s2_b2:bwd", "convT4_4x6_c3_k4s2_b1:fwd")),
    ("conv_gemm_kernel<4>: 2 stages", _G + ":181", _stages(4, 2), ("conv2_12x10_c8_k4s2_b1:bwd", "convT8_5x3_c5_k4s2_b2:fwd")),
    ("conv_gemm_kernel<4>: 3 stages", _G + ":182", _stages(4, 3), ("conv3_9x11_c12_k4s2_b3:bwd", "convT12_3x5_c2_k4s2_b3:fwd")),
    ("conv_gemm_kernel<4>: 5 stages, the ring wraps", _G + ":156, :193", _stages(4, 5), ("conv5_8x8_c20_k4s2_b1:bwd", "convT20_6x4_c1_k4s2_b1:fwd")),
    ("conv_gemm_kernel<4>: 15 stages", _G + ":334", _stages(4, 15), ("conv15_6x6_c60_k4s2_b1:bwd", "convT60_2x3_c4_k4s2_b2:fwd")),
    ("split-K: two even splits of 8 stages", _G + ":334-336, :231", _cg(lambda c, p: (c["ksplit"], c["stages_per_split"], c["last_split_stages"]) == (2, 8, 8)),
     ("conv32_6x5_c136_k3_b2:fwd",)),
    ("split-K: a short last split of 2 stages (`ns > 2` false)", _G + ":142, :182", _cg(lambda c, p: c["ksplit"] == 8 and c["last_split_stages"] == 2),
     ("conv130_9x13_c70_k3_b3:fwd",)),
    ("split-K: a short last split of 1 stage (`ns > 1` false), 16 splits", _G + ":142, :181", _cg(lambda c, p: c["ksplit"] == 16 and c["last_split_stages"] == 1),
     ("conv17_5x5_c136_k4s1_b1:bwd",)),
    ("split-K on the 16-tap kernel, last split one stage short", _G + ":335-336", _cg(lambda c, p: c["NT"] == 16 and c["ksplit"] == 2 and c["last_split_stages"] == 8 and c["stages_per_split"] == 9),
     ("conv17_5x5_c136_k4s1_b1:fwd",)),
    ("two m tiles, the second with 8 live rows", _G + ":349, :238, :250", lambda p: "classes" in p and p["m_tiles"] == 2 and p["last_m_rows"] == 8,
     ("conv32_6x5_c136_k3_b2:fwd", "conv17_5x5_c136_k4s1_b1:fwd", "conv4_24x23_c136_k3_b3:fwd")),
    ("two m tiles and split-K: partial tiles of the second m tile", _G + ":232-238", lambda p: "classes" in p and p["m_tiles"] == 2 and max(p["ksplit"]) > 1,
     ("conv32_6x5_c136_k3_b2:fwd", "conv17_5x5_c136_k4s1_b1:fwd")),
    ("one pixel tile partly filled", _G + ":127, :230", _cg(lambda c, p: c["n_tiles"] == 1 and c["last_n_pixels"] < 128), ("conv2_9x7_c5_k3_b1:fwd", "conv4_9x7_c6_k3_b2:fwd")),
    ("several pixel tiles, a ragged last one", _G + ":127, :230", _cg(lambda c, p: c["n_tiles"] >= 3 and c["last_n_pixels"] < 128),
     ("conv6_11x13_c10_k3_b3:fwd", "conv4_24x23_c136_k3_b3:fwd", "conv130_9x13_c70_k3_b3:fwd")),
    ("a grid that is no multiple of 8 workgroups, above 8 (xcd_remap)", "ipsr_common.h:46-52", _cg(lambda c, p: c["workgroups"] > 8 and c["workgroups"] % 8 != 0),
     ("conv4_24x23_c136_k3_b3:fwd",)),
    ("parity classes: odd output extents, four different grids", _G + ":366", lambda p: "classes" in p and len(p["grids"]) == 4 and len(set(p["grids"])) == 4,
     ("conv4_21x19_c8_k4s2_b2:bwd", "conv3_9x11_c12_k4s2_b3:bwd", "conv8_15x13_c4_k4s2p1d3_b2:bwd")),
    ("parity classes without taps: need_zero, one 16-tap class", _G + ":367, :411-412", lambda p: "classes" in p and p["need_zero"] and p["empty_classes"] == 3 and p["NT"] == (16,),
     ("conv3_12x10_c5_k4s2p3d2_b2:bwd", "conv3_2x2_c5_k4s2p3d2_b3:bwd")),
    ("the dilated input gradient on the 2 x 2 map", _G + ":366-367", lambda p: "classes" in p and p["need_zero"] and p["grids"] == ((1, 1),), ("conv3_2x2_c5_k4s2p3d2_b3:bwd",)),
    ("k = 2 on the direct forms: a 4-tap gather, stride 1 and 2, op 0 and op 3", _G + ":317, :355, :419",
     lambda p: "classes" in p and len(p["classes"]) == 1 and p["NT"] == (4,) and p["live"][0]["dys"] > 0,
     ("conv4_9x8_c8_k2s1_b2:fwd", "conv8_9x8_c6_k2s2p1_b1:fwd", "convT6_5x4_c12_k2s2_b2:bwd", "conv4_9x8_c8_k2s2p1d2_b1:fwd")),
    ("k = 2 on the stride-1 transposed form (op 1)", _G + ":353, :423", lambda p: "classes" in p and len(p["classes"]) == 1 and p["NT"] == (4,) and p["live"][0]["dys"] == -1,
     ("conv4_9x8_c8_k2s1_b2:bwd",)),
    ("k = 2, 3 with dilation 2 on the stride-2 transposed form: all taps in one parity class", _G + ":363-367",
     lambda p: "classes" in p and p["need_zero"] and p["empty_classes"] == 3 and p["NT"] in ((4,), (9,)), ("conv6_9x8_c4_k3s2p2d2_b2:bwd", "conv4_9x8_c8_k2s2p1d2_b1:bwd")),
    ("stride 3 on the direct forms, k3 and k4, op 0 and op 3", _G + ":421, :130", lambda p: "classes" in p and len(p["classes"]) == 1 and p["live"][0]["in_mul"] == 3,
     ("conv4_13x11_c6_k3s3_b2:fwd", "conv3_13x11_c6_k4s3p2_b1:fwd", "convT6_4x5_c3_k4s3_b2:bwd")),
    ("dilation 3 on the stride-2 transposed forms: two taps per parity, offsets a step of -3 apart", _G + ":325, :435-436",
     lambda p: "classes" in p and len(p["live"]) == 4 and all(c["dys"] == -3 and c["dxs"] == -3 for c in p["live"]),
     ("conv8_15x13_c4_k4s2p1d3_b2:bwd", "convT8_4x3_c4_k4s2p1d3_b1:fwd")),
)
