"""The launchers of csrc/thin_conv.hip restated in Python: which kernel instantiation and grid a shape reaches.

A plain module (like bf16_conv_plan.py, guarded.py).  tests/test_thin_conv_plan.py ties it to the built library through the three
workspace queries and `ipsr_conv_thin_f2m_mfma_supported`, and proves that the case tables below reach every variant;
tests/test_gpu_thin_variants.py runs the tables.  Each function names the plan function of thin_conv.hip it mirrors; integer arithmetic is
C's (all operands non-negative, so `//` is the same division).

A plan is a dict, `None` = the launcher refuses the shape (IPSR_ERR_UNSUPPORTED, workspace query 0).  Pointer alignment and the
65535 limits of a grid axis are not restated: no case comes near them.
"""

THIN_OC, THIN_CB, THIN_ROWS = 16, 2, 64                   # the constants of thin_conv.hip
ONE_CCH = 8
LDS_M2F = 48 * 1024                                       # thin_m2f_plan
LDS_ONE = 64 * 1024                                       # ONE_LDS_MAX (to_one_plan)


def align_up(x, a):
    return (x + a - 1) // a * a


def cdiv(a, b):
    return (a + b - 1) // b


def _row_groups(n, rows):
    """A kernel walks `n` rows in workgroups of `rows` (four waves, wave w takes rows w, w + 4, ...): the number of groups, the rows of
    the last one, and whether that one is ragged (shorter than the others: the `y < Ho` bound cuts a wave's walk, or leaves it idle)."""
    groups = cdiv(n, rows)
    last = n - (groups - 1) * rows
    return groups, last, last != rows


def thin_f2m_mfma_plan(B, Cs, O, Ho, Wo, k, stride):
    """`thin_f2m_mfma_plan`."""
    k3, k4 = k == 3 and stride == 1, k == 4 and stride == 2
    if B < 1 or O < 1 or Ho < 1 or Cs not in (3, 6) or not (k3 or k4) or Wo % 32 != 0 or O % 8 != 0:
        return None
    KS = (Cs * k * k + 15) // 16                          # 2, 4, 3, 6
    MT = 4 if O >= 128 and KS <= 4 else 2
    otiles = cdiv(O, 32 * MT)
    rows = 4
    while B * otiles * cdiv(Ho, rows) > 2048 and rows < Ho:
        rows *= 2
    groups, last, ragged = _row_groups(Ho, rows)
    return dict(kernel="f2m_mfma", MT=MT, KS=KS, otiles=otiles, rows=rows, grid=(groups, B, otiles), last_rows=last, ragged=ragged, xsegs=Wo // 32,
                idle_waves=max(0, 4 - last), live_rows_last_tile=O - (otiles - 1) * 32 * MT)


def thin_wrw_mfma_plan(B, Kb, Cs, Hb, Wb, k, stride):
    """`thin_wrw_mfma_plan`."""
    k3, k4 = k == 3 and stride == 1, k == 4 and stride == 2
    if B < 1 or Kb < 1 or Hb < 1 or Cs not in (3, 6) or not (k3 or k4) or Wb % 16 != 0 or Wb < 16:
        return None
    RT = (Cs * k * k + 31) // 32                          # 27, 54, 48, 96 -> 1, 2, 2, 3
    MT = 4 if Kb >= 128 and RT <= 2 else 2
    if Kb % 8 != 0:
        return None
    ktiles = cdiv(Kb, 32 * MT)
    rows, limit = 4, (512 if RT >= 2 else 1024)
    while B * ktiles * cdiv(Hb, rows) > limit and rows < Hb:
        rows *= 2
    gx, last, ragged = _row_groups(Hb, rows)
    return dict(kernel="wrw_mfma", MT=MT, RT=RT, ktiles=ktiles, rows=rows, gx=gx, limit=limit, grid=(gx, B, ktiles), last_rows=last, ragged=ragged,
                ws=align_up(ktiles * B * gx * (32 * MT) * (32 * RT) * 4, 256) + 256)


def thin_wrw_mfma_ws(B, Kb, Cs, Hb, Wb, k, stride):
    p = thin_wrw_mfma_plan(B, Kb, Cs, Hb, Wb, k, stride)
    return 0 if p is None else p["ws"]


def thin_io_plan(op, B, I, O, H, W, bias=False, relu=False):
    """ipsr_conv3x3_thin_io: op 0 `thin_f2m_plan`, few -> many (I in {3, 6}), op 1 `thin_m2f_plan` and the entry's refusal of an epilogue, many -> few (O in {3, 6})."""
    if B < 1 or I < 1 or O < 1 or H < 1 or W < 1:
        return None
    if op == 0:
        if O % THIN_OC != 0 or I not in (3, 6) or W % 2 != 0:
            return None
        return dict(kernel="f2m", T=I, grid=(cdiv(W, 512), H, B * (O // THIN_OC)), lds=THIN_OC * I * 9 * 4)
    if bias or relu or O not in (3, 6) or W % 4 != 0:
        return None
    lds = I * O * 9 * 4
    if lds > LDS_M2F:
        return None
    return dict(kernel="m2f", T=O, grid=(cdiv(W, 256), cdiv(H, 4), B), lds=lds)


def thin_module_pass(op, Cin, Cout):
    """(kernel op, I, O, flip) of ops.conv3x3_thin for a module pass (ops.py:874-877): op 0 Conv2d forward, 1 its input gradient,
    2 ConvTranspose2d forward, 3 its input gradient."""
    I, O = (Cin, Cout) if op in (0, 2) else (Cout, Cin)
    return (0 if I in (3, 6) and O % 16 == 0 else 1), I, O, (1 if op in (1, 2) else 0)


def thin_wrw_plan(B, Cb, Cs, H, W):
    """`thin_wrw_plan`."""
    if B < 1 or Cb < 1 or H < 1 or W < 1 or Cs not in (3, 6) or Cb % THIN_CB != 0 or W % 4 != 0:
        return None
    grid = (cdiv(W, 256), cdiv(H, THIN_ROWS), B * (Cb // THIN_CB))
    return dict(kernel="wrw", T=Cs, grid=grid, ws=align_up(grid[0] * grid[1] * grid[2] * THIN_CB * Cs * 9 * 4, 256) + 256)


def thin_wrw_ws(B, Cb, Cs, H, W):
    p = thin_wrw_plan(B, Cb, Cs, H, W)
    return 0 if p is None else p["ws"]


def to_one_plan(B, C, H, W, K, pad):
    """`to_one_plan` with the LDS sizes of both operations (a plan whose `lds_fwd` / `lds_wrw` exceeds 64 KB is refused at the launch)."""
    Ho, Wo = H + 2 * pad - K + 1, W + 2 * pad - K + 1
    if B < 1 or C < 1 or pad < 0 or Ho < 1 or Wo < 1 or K not in (3, 4) or Ho * cdiv(Wo, 4) > 256:
        return None
    psz = (H + 2 * pad) * (W + 2 * pad)
    nchunk = cdiv(C, ONE_CCH)
    return dict(kernel="one", K=K, pad=pad, Ho=Ho, Wo=Wo, groups=Ho * cdiv(Wo, 4), nchunk=nchunk, last_chunk=C - (nchunk - 1) * ONE_CCH, grid=(nchunk, B),
                ws=align_up(B * nchunk * Ho * Wo * 4, 256) + 256, lds_fwd=(2 * psz + ONE_CCH * K * K) * 4,
                lds_wrw=(2 * psz + 2 * Ho * Wo + 4 * K * K) * 4)


def to_one_ws(B, C, H, W, K, pad):
    p = to_one_plan(B, C, H, W, K, pad)
    return 0 if p is None else p["ws"]


# ---- the GPU cases and the paths they must reach ------------------------------------------------------------------------------------
# A requirement is a dict of plan fields that must match exactly.
#
# ops.conv_thin_f2m_mfma.  id: ((transposed, Cin, Cout, k, stride, B, H, W of the module's input), requirement).  A Conv2d runs its
# forward (Cs = Cin, O = Cout, on the strided grid), a ConvTranspose2d its input gradient (Cs = Cout, O = Cin, on its input's grid).
F2M_MFMA_CASES = {
    "convT128_3_k4s2_b2_5x32": ((True, 128, 3, 4, 2, 2, 5, 32), dict(MT=4, KS=3, rows=4, last_rows=1, idle_waves=3)),
    "conv6_136_k3_b1_6x32": ((False, 6, 136, 3, 1, 1, 6, 32), dict(MT=4, KS=4, otiles=2, live_rows_last_tile=8, rows=4, last_rows=2)),
    "conv3_8_k3_b1_7x64": ((False, 3, 8, 3, 1, 1, 7, 64), dict(MT=2, KS=2, xsegs=2, rows=4, last_rows=3)),
    "conv3_40_k4s2_b2_6x64": ((False, 3, 40, 4, 2, 2, 6, 64), dict(MT=2, KS=3, rows=4, last_rows=3, idle_waves=1, grid=(1, 2, 1))),
    "conv6_72_k3_b1_9x32": ((False, 6, 72, 3, 1, 1, 9, 32), dict(MT=2, KS=4, otiles=2, live_rows_last_tile=8, last_rows=1)),
    "convT24_6_k4s2_b2_5x32": ((True, 24, 6, 4, 2, 2, 5, 32), dict(MT=2, KS=6, last_rows=1)),
    "conv3_8_k3_b33_250x32": ((False, 3, 8, 3, 1, 33, 250, 32), dict(MT=2, KS=2, rows=8, last_rows=2, grid=(32, 33, 1))),
    # added to the issue's list, which names six of the seven pairs: (4, 2) with a second o tile of 8 live rows
    "convT136_3_k3_b1_5x32": ((True, 136, 3, 3, 1, 1, 5, 32), dict(MT=4, KS=2, otiles=2, live_rows_last_tile=8, last_rows=1)),
}

# ops.conv_thin_wrw_mfma.  id: ((Kb, Cs, k, B, Hb, Wb), requirement); stride = 1 for k 3, 2 for k 4.
WRW_MFMA_CASES = {
    "kb136_cs3_k3_b2_5x16": ((136, 3, 3, 2, 5, 16), dict(MT=4, RT=1, ktiles=2, rows=4, last_rows=1)),
    "kb128_cs3_k4_b1_6x48": ((128, 3, 4, 1, 6, 48), dict(MT=4, RT=2, rows=4, last_rows=2)),
    "kb8_cs3_k3_b2_7x80": ((8, 3, 3, 2, 7, 80), dict(MT=2, RT=1, rows=4, last_rows=3)),
    "kb72_cs6_k3_b1_5x16": ((72, 6, 3, 1, 5, 16), dict(MT=2, RT=2, ktiles=2, last_rows=1)),
    "kb24_cs6_k4_b2_6x16": ((24, 6, 4, 2, 6, 16), dict(MT=2, RT=3, last_rows=2)),
    "kb8_cs3_k3_b17_242x16": ((8, 3, 3, 17, 242, 16), dict(MT=2, RT=1, limit=1024, rows=8, gx=31, last_rows=2)),
    "kb8_cs6_k3_b9_230x16": ((8, 6, 3, 9, 230, 16), dict(MT=2, RT=2, limit=512, rows=8, gx=29, last_rows=6)),
}

# ops.conv3x3_thin.  id: ((B, few, many, H, W), requirement).  A few -> many case runs the four module passes that read the few side:
# Conv2d(few, many) forward, Conv2d(many, few) input gradient, ConvTranspose2d(few, many) forward, ConvTranspose2d(many, few) input
# gradient; a many -> few case the other four.
F2M_CASES = {
    "f2m_b2_3_16_1x2": ((2, 3, 16, 1, 2), dict(kernel="f2m", T=3, grid=(1, 1, 2))),
    "f2m_b1_6_32_3x514": ((1, 6, 32, 3, 514), dict(kernel="f2m", T=6, grid=(2, 3, 2))),
    "f2m_b1_3_48_2x1026": ((1, 3, 48, 2, 1026), dict(kernel="f2m", T=3, grid=(3, 2, 3))),
}
M2F_CASES = {
    "m2f_b2_16_3_1x4": ((2, 3, 16, 1, 4), dict(kernel="m2f", T=3, grid=(1, 1, 2))),
    "m2f_b1_18_6_5x260": ((1, 6, 18, 5, 260), dict(kernel="m2f", T=6, grid=(2, 2, 1))),
    "m2f_b1_455_3_2x8": ((1, 3, 455, 2, 8), dict(kernel="m2f", T=3, lds=49140)),
    "m2f_b1_227_6_3x4": ((1, 6, 227, 3, 4), dict(kernel="m2f", T=6, lds=49032)),
}
# refused: (kernel op, B, I, O, H, W)
THIN_IO_REFUSED = {
    "f2m_odd_w": (0, 1, 3, 16, 2, 7),
    "m2f_i456_o3": (1, 1, 456, 3, 2, 8),
    "m2f_i228_o6": (1, 1, 228, 6, 3, 4),
}

# ops.conv3x3_thin_wrw.  id: ((B, Cb, Cs, H, W), requirement)
WRW_CASES = {
    "wrw_b1_2_3_1x4": ((1, 2, 3, 1, 4), dict(grid=(1, 1, 1))),
    "wrw_b2_4_6_65x8": ((2, 4, 6, 65, 8), dict(grid=(1, 2, 4))),
    "wrw_b1_2_3_3x260": ((1, 2, 3, 3, 260), dict(grid=(2, 1, 1))),
    "wrw_b2_6_6_130x516": ((2, 6, 6, 130, 516), dict(grid=(3, 3, 6))),
}

# ops.conv_to_one / conv_to_one_wrw.  id: ((B, C, H, W, K, pad), requirement or None = refused)
TO_ONE_CASES = {
    "one_b1_c1_4x4_k4p0": ((1, 1, 4, 4, 4, 0), dict(Ho=1, Wo=1, groups=1)),
    "one_b2_c9_33x33_k4p1": ((2, 9, 33, 33, 4, 1), dict(groups=256, nchunk=2, last_chunk=1, grid=(2, 2))),
    "one_b1_c8_34x30_k3p0": ((1, 8, 34, 30, 3, 0), dict(Ho=32, Wo=28, groups=224)),
    "one_b2_c7_6x9_k3p1": ((2, 7, 6, 9, 3, 1), dict(Ho=6, Wo=9, groups=18)),
    "one_b1_c5_5x5_k3p2": ((1, 5, 5, 5, 3, 2), dict(Ho=7, Wo=7)),
}
TO_ONE_REFUSED = {"one_b1_c8_34x33_k4p1": (1, 8, 34, 33, 4, 1)}                         # 33 x 8 = 264 groups


def f2m_mfma_geometry(case):
    """(B, Cs, O, Ho, Wo, k, stride) of an F2M_MFMA_CASES entry in the terms of ipsr_conv_thin_f2m_mfma (ops.py:904-914)."""
    tr, Cin, Cout, k, st, B, H, W = case
    return (B, Cout, Cin, H, W, k, st) if tr else (B, Cin, Cout, H // st, W // st, k, st)


def case_plan(cid):
    if cid in F2M_MFMA_CASES:
        return thin_f2m_mfma_plan(*f2m_mfma_geometry(F2M_MFMA_CASES[cid][0]))
    if cid in WRW_MFMA_CASES:
        Kb, Cs, k, B, Hb, Wb = WRW_MFMA_CASES[cid][0]
        return thin_wrw_mfma_plan(B, Kb, Cs, Hb, Wb, k, 1 if k == 3 else 2)
    if cid in F2M_CASES:
        B, few, many, H, W = F2M_CASES[cid][0]
        return thin_io_plan(0, B, few, many, H, W)
    if cid in M2F_CASES:
        B, few, many, H, W = M2F_CASES[cid][0]
        return thin_io_plan(1, B, many, few, H, W)
    if cid in WRW_CASES:
        return thin_wrw_plan(*WRW_CASES[cid][0])
    return to_one_plan(*TO_ONE_CASES[cid][0])


ALL_TABLES = (F2M_MFMA_CASES, WRW_MFMA_CASES, F2M_CASES, M2F_CASES, WRW_CASES, TO_ONE_CASES)
ALL_CASE_IDS = tuple(cid for t in ALL_TABLES for cid in t)


def check_case(cid):
    """Assert that a case reaches the path written beside it -> its plan."""
    want = next(t[cid][1] for t in ALL_TABLES if cid in t)
    got = case_plan(cid)
    assert got is not None, "%s: refused" % cid
    miss = {k: (got.get(k), v) for k, v in want.items() if got.get(k) != v}
    assert not miss, "%s reaches another variant: (got, wanted) %s" % (cid, miss)
    return got


# ---- the variant table: (variant, the plan field of thin_conv.hip or the kernel that selects it, predicate on a plan, case ids) ----------------------------
def _fm(MT, KS):
    return lambda p: p["kernel"] == "f2m_mfma" and (p["MT"], p["KS"]) == (MT, KS)


def _wm(MT, RT):
    return lambda p: p["kernel"] == "wrw_mfma" and (p["MT"], p["RT"]) == (MT, RT)


VARIANTS = (
    ("thin_f2m_mfma_kernel<4,2>", "thin_f2m_mfma_plan (KS, MT)", _fm(4, 2), ("convT136_3_k3_b1_5x32",)),
    ("thin_f2m_mfma_kernel<4,3>", "thin_f2m_mfma_plan (KS, MT)", _fm(4, 3), ("convT128_3_k4s2_b2_5x32",)),
    ("thin_f2m_mfma_kernel<4,4>", "thin_f2m_mfma_plan (KS, MT)", _fm(4, 4), ("conv6_136_k3_b1_6x32",)),
    ("thin_f2m_mfma_kernel<2,2>", "thin_f2m_mfma_plan (KS, MT)", _fm(2, 2), ("conv3_8_k3_b1_7x64", "conv3_8_k3_b33_250x32")),
    ("thin_f2m_mfma_kernel<2,3>", "thin_f2m_mfma_plan (KS, MT)", _fm(2, 3), ("conv3_40_k4s2_b2_6x64",)),
    ("thin_f2m_mfma_kernel<2,4>", "thin_f2m_mfma_plan (KS, MT)", _fm(2, 4), ("conv6_72_k3_b1_9x32",)),
    ("thin_f2m_mfma_kernel<2,6>", "thin_f2m_mfma_plan (KS, MT)", _fm(2, 6), ("convT24_6_k4s2_b2_5x32",)),
    ("thin_f2m_mfma_kernel: a second o tile with 8 live rows", "thin_f2m_mfma_plan (otiles), thin_f2m_mfma_kernel", lambda p: p["kernel"] == "f2m_mfma" and p["otiles"] == 2 and p["live_rows_last_tile"] == 8,
     ("conv6_136_k3_b1_6x32", "conv6_72_k3_b1_9x32", "convT136_3_k3_b1_5x32")),
    ("thin_f2m_mfma_kernel: ragged last row group, a wave idle", "thin_f2m_mfma_kernel", lambda p: p["kernel"] == "f2m_mfma" and p["ragged"] and p["idle_waves"] >= 1,
     ("convT128_3_k4s2_b2_5x32", "conv6_136_k3_b1_6x32", "conv3_8_k3_b1_7x64", "conv3_40_k4s2_b2_6x64")),
    ("thin_f2m_mfma_kernel: two x segments per row", "thin_f2m_mfma_kernel", lambda p: p["kernel"] == "f2m_mfma" and p["xsegs"] == 2, ("conv3_8_k3_b1_7x64",)),
    ("thin_f2m_mfma_kernel: rows_per_wg 8, last group of 2 rows", "thin_f2m_mfma_plan (rows)", lambda p: p["kernel"] == "f2m_mfma" and p["rows"] == 8 and p["last_rows"] == 2,
     ("conv3_8_k3_b33_250x32",)),
    ("thin_wrw_mfma_kernel<4,1>", "thin_wrw_mfma_plan (RT, MT)", _wm(4, 1), ("kb136_cs3_k3_b2_5x16",)),
    ("thin_wrw_mfma_kernel<4,2>", "thin_wrw_mfma_plan (RT, MT)", _wm(4, 2), ("kb128_cs3_k4_b1_6x48",)),
    ("thin_wrw_mfma_kernel<2,1>", "thin_wrw_mfma_plan (RT, MT)", _wm(2, 1), ("kb8_cs3_k3_b2_7x80", "kb8_cs3_k3_b17_242x16")),
    ("thin_wrw_mfma_kernel<2,2>", "thin_wrw_mfma_plan (RT, MT)", _wm(2, 2), ("kb72_cs6_k3_b1_5x16", "kb8_cs6_k3_b9_230x16")),
    ("thin_wrw_mfma_kernel<2,3>", "thin_wrw_mfma_plan (RT, MT)", _wm(2, 3), ("kb24_cs6_k4_b2_6x16",)),
    ("thin_wrw_mfma_kernel: ragged last row group at rows 4", "thin_wrw_mfma_kernel", lambda p: p["kernel"] == "wrw_mfma" and p["rows"] == 4 and p["ragged"],
     ("kb136_cs3_k3_b2_5x16", "kb128_cs3_k4_b1_6x48", "kb8_cs3_k3_b2_7x80", "kb72_cs6_k3_b1_5x16", "kb24_cs6_k4_b2_6x16")),
    ("thin_wrw_mfma_kernel: limit 1024 -> rows 8, last group of 2 rows", "thin_wrw_mfma_plan (rows)", lambda p: p["kernel"] == "wrw_mfma" and (p["limit"], p["rows"], p["last_rows"]) == (1024, 8, 2),
     ("kb8_cs3_k3_b17_242x16",)),
    ("thin_wrw_mfma_kernel: limit 512 -> rows 8, last group of 6 rows", "thin_wrw_mfma_plan (rows)", lambda p: p["kernel"] == "wrw_mfma" and (p["limit"], p["rows"], p["last_rows"]) == (512, 8, 6),
     ("kb8_cs6_k3_b9_230x16",)),
    ("thin_wrw_mfma_kernel: two k tiles", "thin_wrw_mfma_plan (ktiles)", lambda p: p["kernel"] == "wrw_mfma" and p["ktiles"] == 2, ("kb136_cs3_k3_b2_5x16", "kb72_cs6_k3_b1_5x16")),
    ("thin_f2m_kernel<3>, flip 0 and 1", "thin_f2m_plan (I), ops.conv3x3_thin", lambda p: p["kernel"] == "f2m" and p["T"] == 3, ("f2m_b2_3_16_1x2", "f2m_b1_3_48_2x1026")),
    ("thin_f2m_kernel<6>, flip 0 and 1", "thin_f2m_plan (I), ops.conv3x3_thin", lambda p: p["kernel"] == "f2m" and p["T"] == 6, ("f2m_b1_6_32_3x514",)),
    ("thin_f2m_kernel: more than one block on x, y and z", "thin_f2m_plan (grid)", lambda p: p["kernel"] == "f2m" and min(p["grid"]) >= 2,
     ("f2m_b1_6_32_3x514", "f2m_b1_3_48_2x1026")),
    ("thin_m2f_kernel<3>, flip 0 and 1", "thin_m2f_plan (O), ops.conv3x3_thin", lambda p: p["kernel"] == "m2f" and p["T"] == 3, ("m2f_b2_16_3_1x4", "m2f_b1_455_3_2x8")),
    ("thin_m2f_kernel<6>, flip 0 and 1", "thin_m2f_plan (O), ops.conv3x3_thin", lambda p: p["kernel"] == "m2f" and p["T"] == 6, ("m2f_b1_18_6_5x260", "m2f_b1_227_6_3x4")),
    ("thin_m2f_kernel: two blocks on x and y", "thin_m2f_plan (grid)", lambda p: p["kernel"] == "m2f" and p["grid"][0] >= 2 and p["grid"][1] >= 2, ("m2f_b1_18_6_5x260",)),
    ("thin_m2f_kernel: two blocks on z", "thin_m2f_plan (grid)", lambda p: p["kernel"] == "m2f" and p["grid"][2] >= 2, ("m2f_b2_16_3_1x4",)),
    ("thin_m2f_kernel: the last I that fits the 48 KB of LDS", "thin_m2f_plan (lds_bytes)", lambda p: p["kernel"] == "m2f" and LDS_M2F - p["T"] * 36 < p["lds"] <= LDS_M2F,
     ("m2f_b1_455_3_2x8", "m2f_b1_227_6_3x4")),
    ("thin_wrw_kernel<3>", "thin_wrw_plan (Cs)", lambda p: p["kernel"] == "wrw" and p["T"] == 3, ("wrw_b1_2_3_1x4", "wrw_b1_2_3_3x260")),
    ("thin_wrw_kernel<6>", "thin_wrw_plan (Cs)", lambda p: p["kernel"] == "wrw" and p["T"] == 6, ("wrw_b2_4_6_65x8", "wrw_b2_6_6_130x516")),
    ("thin_wrw_kernel: a second row block (H > 64)", "thin_wrw_plan (grid)", lambda p: p["kernel"] == "wrw" and p["grid"][1] >= 2,
     ("wrw_b2_4_6_65x8", "wrw_b2_6_6_130x516")),
    ("thin_wrw_kernel: a second x block (W > 256)", "thin_wrw_plan (grid)", lambda p: p["kernel"] == "wrw" and p["grid"][0] >= 2,
     ("wrw_b1_2_3_3x260", "wrw_b2_6_6_130x516")),
    ("thin_wrw_kernel: more than one block on x, y and z", "thin_wrw_plan (grid)", lambda p: p["kernel"] == "wrw" and min(p["grid"]) >= 3,
     ("wrw_b2_6_6_130x516",)),
    ("one_fwd_kernel<4> / one_wrw_kernel<4>: a 1 x 1 output", "to_one_plan (K)", lambda p: p["kernel"] == "one" and p["K"] == 4 and p["groups"] == 1, ("one_b1_c1_4x4_k4p0",)),
    ("one_fwd_kernel<4>: exactly 256 groups, a second chunk of one channel, two samples", "to_one_plan, one_fwd_kernel", lambda p: p["kernel"] == "one" and p["K"] == 4 and p["groups"] == 256 and p["last_chunk"] == 1 and p["grid"] == (2, 2),
     ("one_b2_c9_33x33_k4p1",)),
    ("one_fwd_kernel<3> / one_wrw_kernel<3>: pad 0, 224 groups", "to_one_plan (K)", lambda p: p["kernel"] == "one" and p["K"] == 3 and p["pad"] == 0 and p["groups"] == 224, ("one_b1_c8_34x30_k3p0",)),
    ("one_fwd_kernel<3>: Wo % 4 != 0", "one_fwd_kernel", lambda p: p["kernel"] == "one" and p["K"] == 3 and p["Wo"] % 4 != 0 and p["Wo"] > 4, ("one_b2_c7_6x9_k3p1", "one_b1_c5_5x5_k3p2")),
    ("one_fwd_kernel<3>: pad 2", "one_fwd_kernel", lambda p: p["kernel"] == "one" and p["K"] == 3 and p["pad"] == 2, ("one_b1_c5_5x5_k3p2",)),
)
