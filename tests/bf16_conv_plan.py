"""The launch planners of csrc/conv_bf16.hip restated in Python: which kernel instantiation and LDS plan a shape reaches.

A plain module (like golden_cases.py, guarded.py).  tests/test_bf16_conv_plan.py ties it to the built library through the
`*_workspace_bytes` queries (kt, ktiles, nstage and nsplit all show in the byte count), tests/test_gpu_bf16_conv_variants.py
asserts through it the variant every case reaches before it compares numbers.  Each function names the lines it mirrors; integer
arithmetic is C's (all operands non-negative, so `//` is the same division).

A plan is a dict, `None` = the shape is refused (IPSR_ERR_UNSUPPORTED).  Forward / input-gradient plans:
    mode "S1" | "F2C" | "C2F" | "DF2C" | "DC2F", kt (128 | 64), ptile (256 | 512), R (lane-grid rows per tile), tiles_per_img, ptiles, ktiles, nphase,
    nsub, nstage, ntap, raw1, lds (bytes of dynamic LDS), nblocks (16-channel blocks of the reduction), nsplit (runs), bps (blocks per
    run), last_bps (blocks of the last run), uneven (last run shorter), wgs (workgroups before the cut), p512 ("taken", or why a
    <= 64-channel layer did not get the 512-pixel tile: "rows" | "lds"; None above 64 channels), Wl (lane-grid width), Hout, Wout,
    B, C, K; split (fp32 tensors, split-bf16 operands: kt 64, ptile 256, no raw buffers), items (their activation items per stage).
    One planner, data_geometry(kind, form, ...), serves the four kernels; cb_geometry / cb_geometry_s2 are its bf16 kinds.  With
    `why=True` a planner returns (plan, message fragment of the refusal).
Weight-gradient plans: RS, groups (stages per image), spw0 (the fill-the-chip value before clamping), spw (stages_per_wg), lowered
    (the `while (groups % spw)` loop ran), nsplit (slabs), ktiles, ctiles.
"""

CB_K, CB_P, CB_C, CB_THREADS = 128, 256, 16, 512          # conv_bf16.hip: CB_K, CB_P, CB_C, CB_THREADS
CB_LDS_MAX = 160 * 1024                                   # CB_LDS_MAX
WB_K, WB_C, WB_THREADS, WB_PX = 128, 64, 512, 128         # WRW_KINDS[WRW_3X3] (TK, TC, PX), WB_THREADS
WB_X_BYTES = 96 * 1024                                    # the ring's share: CB_LDS_MAX less the two a buffers
W2_K, W2_C, W2_PX = 128, 32, 64                           # WRW_KINDS[WRW_S2] (TK, TC, PX)


def cb_tr_max(ptile):                                     # cb_tr_max
    return 6 if ptile == 256 else 10


def cb_xj(ptile):                                         # cb_xj
    return 3 if ptile == 256 else 5


def align_up(x, a):
    return (x + a - 1) // a * a


def cdiv(a, b):
    return (a + b - 1) // b


# ---- the forward / input-gradient planner: data_geometry over DATA_KINDS x DATA_FORMS -----------------------------------------------
# kind: (split, widest lane grid, the width message's fragment)                                                       # DATA_KINDS
DATA_KINDS = {"k3": (False, 256, "grid width %d"), "s2": (False, 256, "grid width %d"),
              "k3_split": (True, 256, "width %d"), "s2_split": (True, 128, "coarse width %d")}
# form: (fine_in, fine_out, nsub, nphase, ntap, column-phase planes of T)                                             # DATA_FORMS
DATA_FORMS = {"S1": (False, False, 1, 1, 9, 1), "F2C": (True, False, 2, 1, 8, 2), "C2F": (False, True, 1, 2, 8, 1),
              "DF2C": (True, False, 2, 1, 8, 1), "DC2F": (False, True, 2, 1, 8, 1)}
S2_FORMS = {0: "F2C", 1: "C2F", 4: "DF2C", 5: "DC2F"}      # modes of the k4 s2 entries (c2_form)


def data_form(form, g):
    """data_form: tensors and halo of a form on the lane grid g[Hl] x g[Wl] with g[R] rows per tile."""
    fine_in, fine_out, nsub, nphase, ntap, planes = DATA_FORMS[form]
    nh, nw, R = g["Hl"], g["Wl"], g["R"]
    NR, PW = (R + 2, nw + 2) if form in ("S1", "C2F") else (R + 1, nw + 1) if form == "F2C" else (R + 1, nw + 3)
    g.update(mode=form, Hin=2 * nh if fine_in else nh, Win=2 * nw if fine_in else nw, Hout=2 * nh if fine_out else nh,
             Wout=2 * nw if fine_out else nw, nsub=nsub, nphase=nphase, ntap=ntap, planes=planes, NR=NR, PW=PW, NPOS=NR * PW)


def data_geometry(kind, form, B, C, K, Hl, Wl, why=False):
    """data_geometry: C reduction channels -> K produced on the lane grid Hl x Wl (S1: the image; k4 s2: the coarse grid)."""
    split, wmax, width_msg = DATA_KINDS[kind]

    def out(g, msg=None):
        return (g, msg) if why else g
    if C % CB_C != 0:
        return out(None, "%d reduction channels are not a multiple of %d" % (C, CB_C))
    if Wl not in (16, 32, 64, 128, wmax):
        return out(None, width_msg % Wl)
    kt = 64 if split or K <= 64 else CB_K

    def tile(ptile):
        R = ptile // Wl
        if Hl % R != 0:
            return None, "%d rows are not a multiple of the %d rows of a tile" % (Hl, R)
        g = dict(B=B, C=C, K=K, Hl=Hl, Wl=Wl, R=R, ptile=ptile, kt=kt, ktiles=cdiv(K, kt), split=split)
        data_form(form, g)
        g["tiles_per_img"] = Hl // R
        g["ptiles"] = B * g["tiles_per_img"]
        g["nstage"] = (C // CB_C) * g["nsub"]
        wgs, nblocks = g["ktiles"] * g["nphase"] * g["ptiles"], C // CB_C                    # cb_cut_reduction
        ns = 1
        if wgs < 128 and nblocks >= 8:                                                       # cb_cut_reduction
            ns = min(min(4, nblocks // 4), cdiv(256, wgs))
        bps = cdiv(nblocks, max(ns, 1))                                                      # cb_cut_reduction
        g["nsplit"] = cdiv(nblocks, bps)                                                     # cb_cut_reduction
        g["sps"] = bps * g["nsub"]
        g["wgs"], g["nblocks"], g["bps"] = wgs, nblocks, bps
        g["last_bps"] = nblocks - (g["nsplit"] - 1) * bps
        g["uneven"] = g["last_bps"] != bps
        nplane = 2 if split else 1                                                           # hi | lo
        g["a_bytes"] = nplane * g["ntap"] * 2 * kt * 16
        g["t_bytes"] = align_up(nplane * g["planes"] * 2 * g["NPOS"] * 16, 256)
        g["raw_bytes"] = 0 if split else align_up(CB_C * g["NR"] * g["Win"] * 2, 1024)
        g["raw1"] = not split and 2 * (g["a_bytes"] + g["t_bytes"] + g["raw_bytes"]) > CB_LDS_MAX
        g["lds"] = 2 * g["a_bytes"] + (1 if split else 2) * g["t_bytes"] + (1 if g["raw1"] else 2) * g["raw_bytes"]    # data_lds_bytes
        g["items"] = 2 * g["NR"] * (g["Win"] // 4)                                           # split: activation items, one per thread
        if split:
            fits = g["items"] <= CB_THREADS
        else:
            fits = 4 * g["NR"] * (g["Win"] // 16) <= 32 * cb_tr_max(ptile) and CB_C * g["NR"] * (g["Win"] // 8) <= cb_xj(ptile) * CB_THREADS
        if g["lds"] > CB_LDS_MAX or not fits:
            return None, "a tile of %d rows x %d does not fit the LDS plan" % (g["NR"], g["Win"])
        return g, None

    # bf16, <= 64 produced channels: the 512-pixel tile first; any refusal falls back to 256, silently
    p512 = None
    if not split and K <= 64:
        g, msg = tile(2 * CB_P)
        if g is not None:
            g["p512"] = "taken"
            return out(g)
        p512 = "rows" if "rows" in msg else ("lds" if "LDS" in msg else "other")
    g, msg = tile(CB_P)
    if g is not None:
        g["p512"] = p512
    return out(g, msg)


def cb_geometry(B, C, K, H, W, why=False):
    """data_geometry(DATA_K3, CB_S1): k3 s1 p1 on bf16 tensors, C reduction channels -> K produced."""
    return data_geometry("k3", "S1", B, C, K, H, W, why)


def cb_geometry_s2(form, B, C, K, nh, nw, why=False):
    """data_geometry(DATA_S2, .): k4 s2 p1 on bf16 tensors.  form 0: fine -> coarse (C = Cf, K = Kc); 1: coarse -> fine (C = Kc, K = Cf)."""
    return data_geometry("s2", S2_FORMS[form], B, C, K, nh, nw, why)


def cb_partial_bytes(g):                                  # cb_partial_bytes
    return align_up(g["nsplit"] * g["B"] * g["K"] * g["Hout"] * g["Wout"] * 4, 256) if g["nsplit"] > 1 else 0


def data_ws_bytes(g):
    """data_ws_bytes: zero page + packed weights (split: two planes) + fp32 partials of a cut reduction; 0 for a refused shape."""
    if g is None:
        return 0
    pack = g["ktiles"] * g["nphase"] * g["nstage"] * g["ntap"] * 2 * g["kt"] * 16           # data_pack_bytes: one plane
    return 256 + align_up((2 if g["split"] else 1) * pack, 256) + cb_partial_bytes(g)


def split_plan(kind, form, B, C, K, Hl, Wl):
    """The plan of a split-bf16 kind as tests/test_gpu_bf16x3_conv.py, bf16x3_s2_plan.py and bf16x3_dil_plan.py hand it out; None = refused."""
    g = data_geometry(kind, form, B, C, K, Hl, Wl)
    if g is None:
        return None
    return dict(g, ragged_k=K % 64 != 0, ws=data_ws_bytes(g))


def _spw(tiles, B, groups):
    """cb_cut_runs: one round of one workgroup per CU, lowered until it divides the stages of an image."""
    spw0 = (tiles * B * groups + 255) // 256
    spw = min(max(spw0, 1), groups)
    lowered = groups % spw != 0
    while groups % spw:
        spw -= 1
    return spw0, spw, lowered


def wb_geometry(B, Ka, Cb, H, W, why=False):
    """wrw_geometry on WRW_KINDS[WRW_3X3]: k3 weight gradient dW[Ka][Cb][3][3]."""
    def out(g, msg=None):
        return (g, msg) if why else g
    if W not in (16, 32, 64, 128):
        return out(None, "image width %d" % W)
    RS = WB_PX // W
    if H % RS != 0:
        return out(None, "%d rows are not a multiple of %d" % (H, RS))
    NSLOT, pitch = 2 * RS + 2, W // 8 + 3
    ktiles, ctiles = cdiv(Ka, WB_K), cdiv(Cb, WB_C)
    if NSLOT * WB_C * pitch * 16 > WB_X_BYTES or RS * WB_C * pitch > 5 * WB_THREADS:     # the fit check of wrw_geometry (never true for the four widths)
        return out(None, "the row ring")
    groups = H // RS
    spw0, spw, lowered = _spw(ktiles * ctiles, B, groups)
    return out(dict(B=B, Ka=Ka, Cb=Cb, H=H, W=W, RS=RS, groups=groups, spw0=spw0, spw=spw, lowered=lowered, nsplit=B * (groups // spw),
                    ktiles=ktiles, ctiles=ctiles))


def wb_ws_bytes(g):                                       # wrw_ws_bytes
    return 0 if g is None else 256 + g["nsplit"] * 9 * g["ktiles"] * WB_K * g["ctiles"] * WB_C * 4


def w2_geometry(B, Kc, Cf, nh, nw, why=False):
    """wrw_geometry on WRW_KINDS[WRW_S2]: k4 s2 p1 weight gradient dW[Kc][Cf][4][4]."""
    def out(g, msg=None):
        return (g, msg) if why else g
    if nw not in (16, 32, 64):
        return out(None, "coarse width %d" % nw)
    RS = W2_PX // nw
    if nh % RS != 0:
        return out(None, "%d coarse rows are not a multiple of %d" % (nh, RS))
    pitch = 2 * nw // 8 + 3
    ktiles, ctiles = cdiv(Kc, W2_K), cdiv(Cf, W2_C)
    if (RS + 1) * 2 * W2_C * pitch > 5 * 512:                                            # the fit check of wrw_geometry (never true for the three widths)
        return out(None, "row ring")
    groups = nh // RS
    spw0, spw, lowered = _spw(ktiles * ctiles, B, groups)
    return out(dict(B=B, Kc=Kc, Cf=Cf, nh=nh, nw=nw, RS=RS, groups=groups, spw0=spw0, spw=spw, lowered=lowered, nsplit=B * (groups // spw),
                    ktiles=ktiles, ctiles=ctiles))


def w2_ws_bytes(g):                                       # wrw_ws_bytes
    return 0 if g is None else 256 + g["nsplit"] * 16 * g["ktiles"] * W2_K * g["ctiles"] * W2_C * 4


# ---- the C entries' argument orders (conv_bf16.hip: ipsr_conv3x3_bf16_packed, ipsr_conv4x4s2_bf16, ipsr_conv4x4s2_bf16_wrw, ipsr_conv3x3_bf16_wrw) ------------------------------------
def k3_plan(op, B, Cin, H, W, Cout, why=False):
    """ipsr_conv3x3_bf16: op 0 Conv2d forward, 1 its input gradient, 2 ConvTranspose2d forward, 3 its input gradient."""
    fwd = op in (0, 2)
    return cb_geometry(B, Cin if fwd else Cout, Cout if fwd else Cin, H, W, why)


def s2_plan(mode, B, Kc, Cf, nh, nw, why=False):
    """ipsr_conv4x4s2_bf16: mode 0 fine -> coarse, 1 coarse -> fine."""
    return cb_geometry_s2(mode, B, Cf if mode == 0 else Kc, Kc if mode == 0 else Cf, nh, nw, why)


def k3_wrw_plan(transposed, B, Cin, H, W, Cout, why=False):
    return wb_geometry(B, Cin, Cout, H, W, why) if transposed else wb_geometry(B, Cout, Cin, H, W, why)


def s2_wrw_plan(B, Kc, Cf, nh, nw, why=False):
    return w2_geometry(B, Kc, Cf, nh, nw, why)


def k3_ws(op, B, Cin, H, W, Cout):
    return data_ws_bytes(k3_plan(op, B, Cin, H, W, Cout))


def s2_ws(mode, B, Kc, Cf, nh, nw):
    return data_ws_bytes(s2_plan(mode, B, Kc, Cf, nh, nw))


def k3_wrw_ws(transposed, B, Cin, H, W, Cout):
    return wb_ws_bytes(k3_wrw_plan(transposed, B, Cin, H, W, Cout))


def s2_wrw_ws(B, Kc, Cf, nh, nw):
    return w2_ws_bytes(s2_wrw_plan(B, Kc, Cf, nh, nw))


# ---- the GPU cases and the plans they must reach --------------------------------------------------------------------------------------
# A requirement is a dict of plan fields that must match exactly; REFUSED = the planner must refuse.  Passes: "fwd" / "dx" (forward,
# input gradient) and "dw".  k3: forward reduces Cin, the input gradient reduces Cout (ops 0 / 1, transposed: 2 / 3).
REFUSED = "refused"

# id: ((tr, Cin, H, W, Cout, B), {pass: requirement})
K3_CASES = {
    "k3_c64_24x32_k160_b3": ((False, 64, 24, 32, 160, 3), dict(
        fwd=dict(kt=128, ptile=256, tiles_per_img=3, raw1=False, nsplit=1),
        dx=dict(kt=64, ptile=256, p512="rows", tiles_per_img=3, nsplit=2, uneven=False),
        dw=dict(groups=6, lowered=False, nsplit=18))),
    "k3_c48_96x16_k32_b2": ((False, 48, 96, 16, 32, 2), dict(
        fwd=dict(kt=64, ptile=512, Wl=16, tiles_per_img=3, raw1=False, nsplit=1),
        dx=dict(kt=64, ptile=512, Wl=16, tiles_per_img=3, nsplit=1),
        dw=dict(groups=12, nsplit=24))),
    "k3T_c32_48x32_k64_b1": ((True, 32, 48, 32, 64, 1), dict(
        fwd=dict(kt=64, ptile=512, Wl=32, tiles_per_img=3, nsplit=1),
        dx=dict(kt=64, ptile=512, Wl=32, tiles_per_img=3, nsplit=1),
        dw=dict(groups=12, nsplit=12))),
    "k3_c32_6x256_k144_b2": ((False, 32, 6, 256, 144, 2), dict(
        fwd=dict(kt=128, ptile=256, Wl=256, R=1, raw1=True, tiles_per_img=6, nsplit=1),
        dx=dict(kt=64, ptile=512, Wl=256, R=2, raw1=True, tiles_per_img=3, nsplit=2, bps=5, last_bps=4, uneven=True),
        dw=REFUSED)),
    "k3_c256_16x16_k64_b1": ((False, 256, 16, 16, 64, 1), dict(
        fwd=dict(kt=64, ptile=256, p512="rows", nsplit=4, uneven=False),
        dx=dict(kt=128, nsplit=1),
        dw=dict(nsplit=2))),
    "k3T_c208_32x16_k48_b1": ((True, 208, 32, 16, 48, 1), dict(
        fwd=dict(kt=64, ptile=512, nsplit=3, bps=5, last_bps=3, uneven=True),
        dx=dict(kt=128),
        dw=dict(nsplit=4))),
    "k3_c64_12x64_k128_b2": ((False, 64, 12, 64, 128, 2), dict(
        fwd=dict(kt=128, Wl=64, tiles_per_img=3),
        dx=dict(kt=64, ptile=256, p512="rows", tiles_per_img=3),
        dw=dict(groups=6))),
    "k3_c32_10x128_k80_b1": ((False, 32, 10, 128, 80, 1), dict(
        fwd=dict(kt=128, Wl=128, tiles_per_img=5),
        dx=dict(kt=64, ptile=256, p512="rows", tiles_per_img=5),
        dw=dict(groups=10))),
}

# weight gradient only: id: ((tr, Cin, H, W, Cout, B), requirement) — Conv2d: Ka = Cout, Cb = Cin
K3_WRW_CASES = {
    "k3w_ka512_cb256_48x16_b9": ((False, 256, 48, 16, 512, 9), dict(groups=6, spw0=4, spw=3, lowered=True, nsplit=18)),
    "k3w_ka1024_cb1088_16x16_b1": ((False, 1088, 16, 16, 1024, 1), dict(groups=2, spw=2, nsplit=1)),
}

# id: ((Kc, Cf, nh, nw, B), {pass: requirement}); "f2c" reduces Cf and produces Kc, "c2f" reduces Kc and produces Cf
S2_CASES = {
    "s2_64_32_32x16_b2": ((64, 32, 32, 16, 2), dict(
        f2c=dict(kt=64, ptile=512, raw1=True, Wl=16), c2f=dict(kt=64, ptile=512, raw1=False), dw=dict(nsplit=16))),
    "s2_48_16_4x128_b1": ((48, 16, 4, 128, 1), dict(
        f2c=dict(kt=64, ptile=512, raw1=True, Wl=128, lds=156672), c2f=dict(kt=64, ptile=512, Wl=128), dw=REFUSED)),
    "s2_128_64_6x128_b1": ((128, 64, 6, 128, 1), dict(
        f2c=dict(kt=128, ptile=256, raw1=True, Wl=128, lds=139776, tiles_per_img=3), c2f=dict(kt=64, ptile=256, p512="rows", nsplit=2), dw=REFUSED)),
    "s2_32_80_4x128_b1": ((32, 80, 4, 128, 1), dict(
        f2c=dict(kt=64, ptile=512, raw1=True, Wl=128), c2f=dict(kt=128, ptile=256, Wl=128), dw=REFUSED)),
    "s2_16_16_2x256_b1": ((16, 16, 2, 256, 1), dict(
        f2c=REFUSED, c2f=dict(kt=64, ptile=512, raw1=True, Wl=256), dw=REFUSED)),
    "s2_128_144_16x16_b1": ((128, 144, 16, 16, 1), dict(
        f2c=dict(kt=128, nsplit=2, bps=5, last_bps=4, uneven=True, nsub=2), c2f=dict(kt=128, nsplit=2, uneven=False), dw=dict(ctiles=5))),
    "s2_64_208_16x16_b1": ((64, 208, 16, 16, 1), dict(
        f2c=dict(kt=64, nsplit=3, bps=5, last_bps=3, uneven=True), c2f=dict(kt=128, nsplit=1), dw=dict())),
    "s2_208_64_16x16_b1": ((208, 64, 16, 16, 1), dict(
        f2c=dict(kt=128, nsplit=1), c2f=dict(kt=64, nsplit=3, bps=5, last_bps=3, uneven=True), dw=dict())),
    "s2_96_48_24x32_b2": ((96, 48, 24, 32, 2), dict(
        f2c=dict(tiles_per_img=3), c2f=dict(tiles_per_img=3, nphase=2), dw=dict(groups=12))),
    # added to the issue's list: the 512-pixel fine -> coarse tile (always `raw1`) at the two widths its cases leave out
    "s2_48_32_48x32_b1": ((48, 32, 48, 32, 1), dict(
        f2c=dict(kt=64, ptile=512, raw1=True, Wl=32, tiles_per_img=3), c2f=dict(kt=64, ptile=512, Wl=32, tiles_per_img=3), dw=dict(groups=24))),
    "s2_16_16_24x64_b2": ((16, 16, 24, 64, 2), dict(
        f2c=dict(kt=64, ptile=512, raw1=True, Wl=64, tiles_per_img=3), c2f=dict(kt=64, ptile=512, Wl=64, tiles_per_img=3), dw=dict(groups=24))),
    # ... and `raw1` coarse -> fine over MORE than one stage (s2_16_16_2x256_b1 reduces 16 channels: its in-loop transposition never runs)
    "s2_48_16_4x256_b2": ((48, 16, 4, 256, 2), dict(
        f2c=REFUSED, c2f=dict(kt=64, ptile=512, raw1=True, Wl=256, nstage=3, tiles_per_img=2, nsplit=1), dw=REFUSED)),
}

S2_WRW_CASES = {
    "s2w_512_512_24x32_b5": ((512, 512, 24, 32, 5), dict(groups=12, spw=12, nsplit=5)),
    "s2w_512_1056_8x16_b1": ((512, 1056, 8, 16, 1), dict(groups=2, spw=2, nsplit=1)),
}


def case_plans(cid):
    """-> {pass: plan or None} of a case of the four tables above."""
    if cid in K3_CASES:
        (tr, Cin, H, W, Cout, B), _ = K3_CASES[cid]
        return dict(fwd=k3_plan(2 if tr else 0, B, Cin, H, W, Cout), dx=k3_plan(3 if tr else 1, B, Cin, H, W, Cout),
                    dw=k3_wrw_plan(tr, B, Cin, H, W, Cout))
    if cid in K3_WRW_CASES:
        (tr, Cin, H, W, Cout, B), _ = K3_WRW_CASES[cid]
        return dict(dw=k3_wrw_plan(tr, B, Cin, H, W, Cout))
    if cid in S2_CASES:
        (Kc, Cf, nh, nw, B), _ = S2_CASES[cid]
        return dict(f2c=s2_plan(0, B, Kc, Cf, nh, nw), c2f=s2_plan(1, B, Kc, Cf, nh, nw), dw=s2_wrw_plan(B, Kc, Cf, nh, nw))
    (Kc, Cf, nh, nw, B), _ = S2_WRW_CASES[cid]
    return dict(dw=s2_wrw_plan(B, Kc, Cf, nh, nw))


def case_requirements(cid):
    for table in (K3_CASES, S2_CASES):
        if cid in table:
            return table[cid][1]
    for table in (K3_WRW_CASES, S2_WRW_CASES):
        if cid in table:
            return dict(dw=table[cid][1])
    raise KeyError(cid)


def check_case(cid):
    """Assert that every pass of a case reaches the plan written beside it -> {pass: plan or None}."""
    plans = case_plans(cid)
    for name, want in case_requirements(cid).items():
        got = plans[name]
        if want == REFUSED:
            assert got is None, "%s/%s: should be refused, got %s" % (cid, name, got)
            continue
        assert got is not None, "%s/%s: refused" % (cid, name)
        miss = {k: (got.get(k), v) for k, v in want.items() if got.get(k) != v}
        assert not miss, "%s/%s reaches another variant: (got, wanted) %s" % (cid, name, miss)
    return plans


def same_cut(p, q):
    """Two forward / input-gradient plans (a batch and a batch of one) add their channel blocks in the same order."""
    return (p["nsplit"], p["bps"], p["kt"], p["ptile"]) == (q["nsplit"], q["bps"], q["kt"], q["ptile"])


# ---- the variant table: (variant, selecting lines, predicate on a plan, ((case id, pass), ...)) ------------------------------------------
def _multi(p):
    return p["tiles_per_img"] > 1 and p["tiles_per_img"] & (p["tiles_per_img"] - 1) != 0


VARIANTS = (
    ("S1 KT128 P256, 3 tiles per image (W 32)", "tiles_per_img, data_geometry ptiles", lambda p: p["mode"] == "S1" and p["kt"] == 128 and p["tiles_per_img"] == 3 and p["Wl"] == 32,
     (("k3_c64_24x32_k160_b3", "fwd"),)),
    ("S1 KT128 P256, 3 / 5 tiles per image at W 64 / 128", "tiles_per_img, data_geometry ptiles", lambda p: p["mode"] == "S1" and p["kt"] == 128 and _multi(p) and p["Wl"] in (64, 128),
     (("k3_c64_12x64_k128_b2", "fwd"), ("k3_c32_10x128_k80_b1", "fwd"))),
    ("S1 KT128 P256 at W 256: one row per tile, raw1, 6 tiles per image", "data_geometry rows, raw1", lambda p: p["mode"] == "S1" and p["kt"] == 128 and p["Wl"] == 256 and p["R"] == 1 and p["raw1"] and p["tiles_per_img"] == 6,
     (("k3_c32_6x256_k144_b2", "fwd"),)),
    ("S1 KT64 P512 at W 16, 3 tiles per image", "data_geometry", lambda p: p["mode"] == "S1" and p["kt"] == 64 and p["ptile"] == 512 and p["Wl"] == 16 and p["tiles_per_img"] == 3,
     (("k3_c48_96x16_k32_b2", "fwd"), ("k3_c48_96x16_k32_b2", "dx"))),
    ("S1 KT64 P512 at W 32, 3 tiles per image", "data_geometry", lambda p: p["mode"] == "S1" and p["kt"] == 64 and p["ptile"] == 512 and p["Wl"] == 32 and p["tiles_per_img"] == 3,
     (("k3T_c32_48x32_k64_b1", "fwd"), ("k3T_c32_48x32_k64_b1", "dx"))),
    ("S1 KT64, P512 refused by the rows -> P256", "data_geometry 512 -> 256", lambda p: p["mode"] == "S1" and p["kt"] == 64 and p["ptile"] == 256 and p["p512"] == "rows",
     (("k3_c64_24x32_k160_b3", "dx"), ("k3_c64_12x64_k128_b2", "dx"), ("k3_c32_10x128_k80_b1", "dx"), ("k3_c256_16x16_k64_b1", "fwd"))),
    ("S1 KT64 P256, reduction cut in 2 / in 4", "cb_cut_reduction", lambda p: p["mode"] == "S1" and p["kt"] == 64 and p["ptile"] == 256 and p["nsplit"] in (2, 4),
     (("k3_c64_24x32_k160_b3", "dx"), ("k3_c256_16x16_k64_b1", "fwd"))),
    ("S1 KT64 P512, cut in 3 uneven (5 + 5 + 3 blocks)", "cb_cut_reduction", lambda p: p["mode"] == "S1" and p["kt"] == 64 and p["ptile"] == 512 and (p["nsplit"], p["bps"], p["last_bps"]) == (3, 5, 3),
     (("k3T_c208_32x16_k48_b1", "fwd"),)),
    ("S1 KT64 P512 raw1 (W 256), cut in 2 uneven (5 + 4 blocks)", "cb_cut_reduction, data_geometry raw1", lambda p: p["mode"] == "S1" and p["kt"] == 64 and p["ptile"] == 512 and p["raw1"] and (p["nsplit"], p["bps"], p["last_bps"]) == (2, 5, 4),
     (("k3_c32_6x256_k144_b2", "dx"),)),
    ("F2C KT64 P512 raw1 at nw 16", "data_geometry raw1", lambda p: p["mode"] == "F2C" and p["kt"] == 64 and p["ptile"] == 512 and p["raw1"] and p["Wl"] == 16,
     (("s2_64_32_32x16_b2", "f2c"),)),
    ("F2C KT64 P512 raw1 at nw 32, 3 tiles per image", "data_geometry raw1", lambda p: p["mode"] == "F2C" and p["kt"] == 64 and p["ptile"] == 512 and p["raw1"] and p["Wl"] == 32 and p["tiles_per_img"] == 3,
     (("s2_48_32_48x32_b1", "f2c"),)),
    ("F2C KT64 P512 raw1 at nw 64, 3 tiles per image", "data_geometry raw1", lambda p: p["mode"] == "F2C" and p["kt"] == 64 and p["ptile"] == 512 and p["raw1"] and p["Wl"] == 64 and p["tiles_per_img"] == 3,
     (("s2_16_16_24x64_b2", "f2c"),)),
    ("F2C KT64 P512 raw1 at nw 128 (LDS 156 672 B)", "data_geometry raw1", lambda p: p["mode"] == "F2C" and p["kt"] == 64 and p["ptile"] == 512 and p["raw1"] and p["Wl"] == 128 and p["lds"] == 156672,
     (("s2_48_16_4x128_b1", "f2c"), ("s2_32_80_4x128_b1", "f2c"))),
    ("F2C KT128 P256 raw1 at nw 128 (LDS 139 776 B), 3 tiles per image", "data_geometry raw1", lambda p: p["mode"] == "F2C" and p["kt"] == 128 and p["raw1"] and p["Wl"] == 128 and p["lds"] == 139776 and p["tiles_per_img"] == 3,
     (("s2_128_64_6x128_b1", "f2c"),)),
    ("F2C cut in 2 uneven, a run = bps x nsub stages (10 + 8)", "cb_cut_reduction", lambda p: p["mode"] == "F2C" and p["nsub"] == 2 and (p["nsplit"], p["sps"], p["last_bps"] * p["nsub"]) == (2, 10, 8),
     (("s2_128_144_16x16_b1", "f2c"),)),
    ("F2C KT64 cut in 3 uneven", "cb_cut_reduction", lambda p: p["mode"] == "F2C" and p["kt"] == 64 and p["nsplit"] == 3 and p["uneven"],
     (("s2_64_208_16x16_b1", "f2c"),)),
    ("F2C 3 tiles per image (KT128)", "tiles_per_img, data_geometry ptiles", lambda p: p["mode"] == "F2C" and p["tiles_per_img"] == 3 and p["kt"] == 128,
     (("s2_96_48_24x32_b2", "f2c"),)),
    ("C2F KT64 P512 at nw 128", "data_geometry", lambda p: p["mode"] == "C2F" and p["kt"] == 64 and p["ptile"] == 512 and p["Wl"] == 128,
     (("s2_48_16_4x128_b1", "c2f"),)),
    ("C2F KT128 P256 at nw 128", "data_geometry", lambda p: p["mode"] == "C2F" and p["kt"] == 128 and p["Wl"] == 128,
     (("s2_32_80_4x128_b1", "c2f"),)),
    ("C2F KT64 P512 raw1 at nw 256", "data_geometry raw1", lambda p: p["mode"] == "C2F" and p["kt"] == 64 and p["ptile"] == 512 and p["raw1"] and p["Wl"] == 256,
     (("s2_16_16_2x256_b1", "c2f"),)),
    ("C2F KT64 P512 raw1 at nw 256 over 3 stages, 2 tiles per image", "data_geometry, the raw1 stage loop", lambda p: p["mode"] == "C2F" and p["raw1"] and p["Wl"] == 256 and p["nstage"] == 3 and p["nsplit"] == 1 and p["tiles_per_img"] == 2,
     (("s2_48_16_4x256_b2", "c2f"),)),
    ("C2F KT64 P256 (rows) cut in 2, 3 tiles per image", "cb_cut_reduction", lambda p: p["mode"] == "C2F" and p["kt"] == 64 and p["ptile"] == 256 and p["nsplit"] == 2 and p["tiles_per_img"] == 3,
     (("s2_128_64_6x128_b1", "c2f"),)),
    ("C2F KT64 cut in 3 uneven", "cb_cut_reduction", lambda p: p["mode"] == "C2F" and p["kt"] == 64 and p["nsplit"] == 3 and p["uneven"],
     (("s2_208_64_16x16_b1", "c2f"),)),
    ("C2F 3 tiles per image, both row phases", "tiles_per_img, data_geometry ptiles", lambda p: p["mode"] == "C2F" and p["tiles_per_img"] == 3 and p["nphase"] == 2,
     (("s2_96_48_24x32_b2", "c2f"), ("s2_48_32_48x32_b1", "c2f"))),
    ("k3 weight gradient: groups 6 / 10 / 12 (not a power of two)", "wrw_geometry", lambda p: "RS" in p and "Ka" in p and p["groups"] in (6, 10, 12),
     (("k3_c64_24x32_k160_b3", "dw"), ("k3_c32_10x128_k80_b1", "dw"), ("k3_c48_96x16_k32_b2", "dw"))),
    ("k3 weight gradient: stages_per_wg lowered by the loop (4 -> 3), 1 < spw < groups", "cb_cut_runs", lambda p: "Ka" in p and p["lowered"] and 1 < p["spw"] < p["groups"],
     (("k3w_ka512_cb256_48x16_b9", "dw"),)),
    ("k3 weight gradient: spw = groups, ONE slab", "cb_cut_runs", lambda p: "Ka" in p and p["nsplit"] == 1 and p["spw"] == p["groups"] > 1,
     (("k3w_ka1024_cb1088_16x16_b1", "dw"),)),
    ("k4 s2 weight gradient: groups 12 / 24 (not a power of two)", "wrw_geometry", lambda p: "Kc" in p and p["groups"] in (12, 24),
     (("s2_96_48_24x32_b2", "dw"), ("s2_48_32_48x32_b1", "dw"))),
    ("k4 s2 weight gradient: spw = groups 12, one slab per image", "cb_cut_runs", lambda p: "Kc" in p and p["spw"] == p["groups"] == 12 and p["nsplit"] == p["B"],
     (("s2w_512_512_24x32_b5", "dw"),)),
    ("k4 s2 weight gradient: ONE slab", "cb_cut_runs", lambda p: "Kc" in p and p["nsplit"] == 1 and p["spw"] == p["groups"] > 1,
     (("s2w_512_1056_8x16_b1", "dw"),)),
)

ALL_CASE_IDS = tuple(K3_CASES) + tuple(K3_WRW_CASES) + tuple(S2_CASES) + tuple(S2_WRW_CASES)
