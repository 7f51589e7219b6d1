"""The launch plan of the split-bf16 direct kernel for the DILATED 4x4 stride-2 layer Conv2d(k4, stride 2, pad 3, dilation 2) on fp32 tensors
(csrc/conv_bf16.hip, data_geometry / data_form on DATA_S2_SPLIT), restated in Python (tests/bf16_conv_plan.py), and the cases of
tests/test_gpu_bf16x3_dil.py with the variant each must reach.  No GPU, no library: tests/test_bf16x3_dil_abi.py compares the library's workspace query against `ws` here.

Shapes are (B, Kc, Cf, nh, nw): fine [B,Cf,2nh,2nw] (x / dx), coarse [B,Kc,nh,nw] (y / dy), weight [Kc,Cf,4,4].  mode 4 = fine -> coarse
(the forward: reduces Cf, produces Kc), mode 5 = coarse -> fine (the input gradient: reduces Kc, produces Cf).  Both run on the coarse lane
grid, tile = 64 produced channels x 256 coarse pixels = R = 256 / nw coarse rows, and cut a 16-channel block into two sub-stages of 8 taps
(the weight-row pairs), each on R + 1 input rows and a T image nw + 3 positions wide (halo 2 / 1 for mode 4, 1 / 2 for mode 5).  Mode 4
loads items of 4 floats from rows 2 nw wide and keeps the two odd columns; mode 5 writes the whole fine result, so under a reduction cut
its partials are fine-sized.
"""
import bf16_conv_plan as P


def plan(mode, B, Kc, Cf, nh, nw):
    """None where the planner refuses."""
    if mode not in (4, 5) or min(B, Kc, Cf, nh, nw) < 1:
        return None
    C, K = (Cf, Kc) if mode == 4 else (Kc, Cf)                    # reduction / produced channels
    p = P.split_plan("s2_split", P.S2_FORMS[mode], B, C, K, nh, nw)
    return p and {k: p[k] for k in ("R", "NR", "PW", "ktiles", "tiles_per_img", "ptiles", "nstage", "nsplit", "sps", "lds", "t_bytes", "items", "ragged_k", "ws")}


# id: ((B, Kc, Cf, nh, nw), {mode: the plan fields the case is there for})
CASES = {
    # one channel block (mode 4: the two sub-stages only), ragged produced channels, one tile touching all four borders: the asymmetric 2 / 1 halo
    "one": ((2, 48, 16, 16, 16), {4: dict(nstage=2, ktiles=1, tiles_per_img=1, ragged_k=True, nsplit=1), 5: dict(nstage=6, ktiles=1, tiles_per_img=1, ragged_k=True, nsplit=1)}),
    # five channel blocks (the A buffers wrap), two k tiles, two tiles per image: the halo rows come from the neighbouring tile
    "wrap": ((3, 80, 80, 32, 16), {4: dict(nstage=10, ktiles=2, tiles_per_img=2, ragged_k=True, nsplit=1), 5: dict(nstage=10, ktiles=2, tiles_per_img=2, ragged_k=True, nsplit=1)}),
    # R = 2 is smaller than the 3 halo rows; the largest T, the most items
    "wide": ((1, 64, 32, 4, 128), {4: dict(R=2, NR=3, PW=131, items=384, t_bytes=25344, tiles_per_img=2, ktiles=1, ragged_k=False),
                                   5: dict(R=2, NR=3, PW=131, items=192, t_bytes=25344, tiles_per_img=2, ragged_k=True)}),
    # three tiles per image: the tile -> (image, row) split is a real division
    "tiles3": ((2, 64, 32, 12, 64), {4: dict(R=4, NR=5, tiles_per_img=3, ptiles=6), 5: dict(R=4, NR=5, tiles_per_img=3, ptiles=6)}),
    # eight channel blocks on two workgroups: the reduction is cut into two runs of four blocks + the ordered add
    "cut": ((1, 128, 128, 16, 16), {4: dict(nsplit=2, sps=8, nstage=16, ktiles=2), 5: dict(nsplit=2, sps=8, nstage=16, ktiles=2)}),
}
# the dilated down convolutions of the step (netG, one per U-Net level that the dispatcher gives "wino_dil") at batch 8: (Kc, Cf, n), fine side 2 n
STEP_ROWS = [(64, 64, 128), (128, 128, 64), (256, 256, 32), (512, 512, 16)]


def check_cases():
    seen_k, seen_p = set(), set()
    for cid, (shape, need) in CASES.items():
        for mode in (4, 5):
            p = plan(mode, *shape)
            assert p is not None, (cid, mode)
            assert p["lds"] <= 160 * 1024 and p["items"] <= 512, (cid, mode, p)
            assert p["sps"] % 2 == 0, (cid, mode, p)              # a run starts on sub-stage 0
            for k, v in need[mode].items():
                assert p[k] == v, (cid, mode, k, p[k], v)
            seen_k.add((p["ktiles"] > 1, p["ragged_k"]))
            seen_p.add(p["tiles_per_img"])
    # one and several k tiles, whole and ragged; one, two and three pixel tiles per image
    assert {(False, False), (False, True), (True, True), (True, False)} <= seen_k, seen_k
    assert {1, 2, 3} <= seen_p, seen_p
