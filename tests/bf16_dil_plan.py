"""The launch plan of the direct bf16 kernel for the DILATED 4x4 stride-2 layer Conv2d(k4, stride 2, pad 3, dilation 2) on bf16 tensors
(csrc/conv_bf16.hip: conv_bf16_kernel in the forms CB_DF2C / CB_DC2F, data_geometry / data_form on DATA_S2_DIL; ipsr_conv4x4s2_bf16_dil),
restated in Python on top of tests/bf16_conv_plan.py, and the cases of tests/test_gpu_bf16_dil.py with the variant each must reach.  No GPU, no
library: tests/test_bf16_dil_abi.py compares the library's workspace query against `ws` here.

Shapes are (B, Kc, Cf, nh, nw): fine [B,Cf,2nh,2nw] (x / dx), coarse [B,Kc,nh,nw] (y / dy), weight [Kc,Cf,4,4].  mode 0 = fine -> coarse (the
forward: reduces Cf, produces Kc), mode 1 = coarse -> fine (the input gradient: reduces Kc, produces Cf).  DATA_S2_DIL is the bf16 plan of
DATA_S2 (tile 128 x 256, or 64 produced channels x 512 / 256 pixels when K <= 64; LDS = A[2] | T[2] | raw[2 or 1]) on coarse widths 16 .. 128:
the mirror runs bf16_conv_plan's "s2" kind and applies the width limit itself.  Both forms cut a 16-channel block into two sub-stages of 8
taps, each on R + 1 input rows and a T image nw + 3 positions wide.

`raw1` (one raw buffer where two do not fit 160 KiB) never comes up in these forms, so no case can reach it: the largest plan is mode 0 at
nw = 128 on the 512-pixel tile, 2 x (16384 A + 20992 T + 40960 raw) = 156672 <= 163840 bytes (T is ONE plane here; the k4 s2 p1 form F2C,
always `raw1` on that tile, keeps two), and on the 128-row tile 2 x (32768 + 12800 + 24576) = 140288.  `check_cases` therefore asserts that
`raw1` is off in every case and `test_raw1_never` (tests/test_bf16_dil_abi.py) that it is off over the whole sweep.
"""
import bf16_conv_plan as P

WIDTHS = (16, 32, 64, 128)
FIELDS = ("mode", "kt", "ptile", "R", "NR", "PW", "tiles_per_img", "ptiles", "ktiles", "raw1", "lds", "nstage", "nsplit", "sps", "bps", "last_bps", "uneven",
          "nblocks", "p512", "Win", "Wl", "Hout", "Wout")


def plan(mode, B, Kc, Cf, nh, nw):
    """None where the planner refuses (or the entry's argument check does: the workspace query is 0 either way)."""
    if mode not in (0, 1) or min(B, Kc, Cf, nh, nw) < 1 or nw not in WIDTHS:         # DATA_KINDS[DATA_S2_DIL].wmax = 128
        return None
    C, K = (Cf, Kc) if mode == 0 else (Kc, Cf)                    # reduction / produced channels
    g = P.data_geometry("s2", P.S2_FORMS[4 + mode], B, C, K, nh, nw)
    if g is None:
        return None
    p = {k: g[k] for k in FIELDS}
    p.update(ragged_k=K % g["kt"] != 0, ws=P.data_ws_bytes(g),
             tr_blocks=4 * g["NR"] * (g["Win"] // 16), tr_room=32 * P.cb_tr_max(g["ptile"]),             # the per-thread loop bounds of a stage
             raw_chunks=P.CB_C * g["NR"] * (g["Win"] // 8), raw_room=P.cb_xj(g["ptile"]) * P.CB_THREADS)
    return p


def same_cut(p, q):
    return P.same_cut(p, q)


# id: ((B, Kc, Cf, nh, nw), {mode: the plan fields the case is there for})
CASES = {
    # one channel block in mode 0 (the two sub-stages only), ragged K, 64-row tile, P512 turned down by the rows, one tile touching all four borders
    # (halo 2 before / 1 behind, mirrored for the gradient), batch 2
    "one": ((2, 48, 16, 16, 16), {0: dict(nstage=2, kt=64, ptile=256, p512="rows", tiles_per_img=1, ragged_k=True, nsplit=1),
                                  1: dict(nstage=6, kt=64, ptile=256, p512="rows", tiles_per_img=1, ragged_k=True, nsplit=1)}),
    # 64-row tile with 512 pixels, two tiles per image
    "p512": ((2, 32, 32, 64, 16), {0: dict(kt=64, ptile=512, p512="taken", R=32, tiles_per_img=2, nsplit=1),
                                   1: dict(kt=64, ptile=512, p512="taken", R=32, tiles_per_img=2, nsplit=1)}),
    # 128-row tile, two k tiles with the last ragged, five channel blocks (the A buffers wrap), two tiles per image, batch 3
    "kt128": ((3, 160, 80, 32, 16), {0: dict(kt=128, ptile=256, ktiles=2, ragged_k=True, nstage=10, tiles_per_img=2, nsplit=1),
                                     1: dict(kt=128, ptile=256, ktiles=1, ragged_k=True, nstage=20, tiles_per_img=2, nsplit=2, sps=10)}),
    # nw = 128: R = 2 smaller than the 3 halo rows, three tiles per image; mode 0 fills the loop bounds exactly
    "wide": ((1, 64, 32, 6, 128), {0: dict(kt=64, ptile=256, p512="rows", R=2, NR=3, PW=131, tiles_per_img=3, tr_blocks=192, tr_room=192, raw_chunks=1536, raw_room=1536),
                                   1: dict(kt=64, ptile=256, p512="rows", R=2, NR=3, PW=131, tiles_per_img=3)}),
    # nw = 128 on the 512-pixel tile: the largest plan (156672 bytes in mode 0), the loop bounds exactly full again
    "wide512": ((1, 64, 32, 8, 128), {0: dict(kt=64, ptile=512, R=4, NR=5, tiles_per_img=2, raw1=False, lds=156672, tr_blocks=320, tr_room=320, raw_chunks=2560, raw_room=2560),
                                      1: dict(kt=64, ptile=512, R=4, NR=5, tiles_per_img=2, raw1=False)}),
    # nw = 128 on the 128-row tile (mode 0: 144 produced channels, two k tiles, the last ragged); mode 1 produces 32: the 512-pixel tile, cut 5 + 4
    "wide128": ((1, 144, 32, 4, 128), {0: dict(kt=128, ptile=256, ktiles=2, ragged_k=True, R=2, tiles_per_img=2, tr_blocks=192, tr_room=192),
                                       1: dict(kt=64, ptile=512, R=4, tiles_per_img=1, nstage=18, nsplit=2, bps=5, last_bps=4, uneven=True)}),
    # three tiles per image at nw = 64: the tile -> (image, row) split is a real division
    "tiles3": ((2, 64, 32, 12, 64), {0: dict(R=4, NR=5, tiles_per_img=3, ptiles=6), 1: dict(R=4, NR=5, tiles_per_img=3, ptiles=6)}),
    # eight channel blocks on one / two workgroups: the reduction is cut into equal runs + the ordered add
    "cut": ((1, 128, 128, 16, 16), {0: dict(kt=128, nsplit=2, sps=8, nstage=16, uneven=False), 1: dict(kt=128, nsplit=2, sps=8, nstage=16, uneven=False)}),
    # thirteen channel blocks in mode 0: an uneven cut (5 + 5 + 3), every run starting on sub-stage 0; mode 1 reduces 64 channels: no cut
    "cut3": ((1, 64, 208, 16, 16), {0: dict(kt=64, nsplit=3, bps=5, last_bps=3, sps=10, uneven=True), 1: dict(kt=128, ktiles=2, ragged_k=True, nsplit=1)}),
}
# the dilated down convolutions of the step (netG, one per U-Net level from 128x128 coarse down to 16x16): (Kc, Cf, n), fine side 2 n
STEP_ROWS = [(64, 64, 128), (128, 128, 64), (256, 256, 32), (512, 512, 16)]


def check_cases():
    """Every case reaches the variant it is there for; across the table and both modes every tile, cut and tile count occurs."""
    seen = dict(kt=set(), ptile=set(), raw1=set(), cut=set(), tiles=set(), ragged=set())
    plans = {}
    for cid, (shape, need) in CASES.items():
        for mode in (0, 1):
            p = plan(mode, *shape)
            assert p is not None, (cid, mode)
            assert p["lds"] <= P.CB_LDS_MAX and p["tr_blocks"] <= p["tr_room"] and p["raw_chunks"] <= p["raw_room"], (cid, mode, p)
            assert p["sps"] % 2 == 0, (cid, mode, p)              # a run starts on sub-stage 0
            assert p["raw1"] is False, (cid, mode, p)             # see the module docstring
            for k, v in need[mode].items():
                assert p[k] == v, (cid, mode, k, p[k], v)
            seen["kt"].add(p["kt"]); seen["ptile"].add(p["ptile"]); seen["raw1"].add(p["raw1"]); seen["cut"].add(p["nsplit"] > 1)
            seen["tiles"].add(p["tiles_per_img"]); seen["ragged"].add(p["ragged_k"])
            plans[cid, mode] = p
    assert seen["kt"] == {64, 128} and seen["ptile"] == {256, 512}, seen
    assert seen["cut"] == {False, True} and {1, 2, 3} <= seen["tiles"] and seen["ragged"] == {False, True}, seen
    return plans
