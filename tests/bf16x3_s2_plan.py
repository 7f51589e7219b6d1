"""The launch plan of the split-bf16 direct kernel for the k4 s2 p1 layers on fp32 tensors (csrc/conv_bf16.hip, data_geometry on DATA_S2_SPLIT), restated in
Python
(tests/bf16_conv_plan.py), and the cases of tests/test_gpu_bf16x3_s2.py with the variant each must reach.  No GPU, no library: tests/test_bf16x3_s2_abi.py
compares the library's workspace query against `ws` here.

Shapes are (B, Kc, Cf, nh, nw): fine [B,Cf,2nh,2nw], coarse [B,Kc,nh,nw], weight [Kc,Cf,4,4].  mode 0 = fine -> coarse (reduces Cf, produces
Kc, two sub-stages per 16-channel block: one per input row parity), mode 1 = coarse -> fine (reduces Kc, produces Cf, one workgroup per
output row parity).  The lane grid is the coarse one in both: tile = 64 produced channels x 256 coarse pixels = R = 256 / nw coarse rows.
The plan has ONE k tile (64 rows) and ONE pixel tile (256): what varies is how many of each a launch has, the stage count and the cut.
"""
import bf16_conv_plan as P


def plan(mode, B, Kc, Cf, nh, nw):
    """None where the planner refuses."""
    if mode not in (0, 1) or min(B, Kc, Cf, nh, nw) < 1:
        return None
    C, K = (Cf, Kc) if mode == 0 else (Kc, Cf)                    # reduction / produced channels
    p = P.split_plan("s2_split", P.S2_FORMS[mode], B, C, K, nh, nw)
    return p and {k: p[k] for k in ("R", "NR", "ktiles", "tiles_per_img", "ptiles", "nstage", "nsplit", "sps", "lds", "items", "ragged_k", "ws")}


# id: ((B, Kc, Cf, nh, nw), {mode: the plan fields the case is there for})
CASES = {
    # one channel block under mode 0 (the two sub-stages only), produced channels no tile multiple, one pixel tile touching both borders
    "one": ((2, 48, 16, 16, 16), {0: dict(nstage=2, ktiles=1, tiles_per_img=1, ragged_k=True, nsplit=1), 1: dict(nstage=3, ktiles=1, tiles_per_img=1, ragged_k=True)}),
    # five channel blocks (the A buffers wrap), two k tiles, two pixel tiles per image (halo rows cross tiles)
    "wrap": ((3, 80, 80, 32, 16), {0: dict(nstage=10, ktiles=2, tiles_per_img=2, ragged_k=True, nsplit=1), 1: dict(nstage=5, ktiles=2, tiles_per_img=2, nsplit=1)}),
    # the widest grid: fewest rows per tile, the largest T, fine rows of 256 floats, the most items per thread block
    "wide": ((1, 64, 32, 4, 128), {0: dict(R=2, NR=3, items=384, tiles_per_img=2, ktiles=1, ragged_k=False), 1: dict(R=2, NR=4, items=256, tiles_per_img=2, ragged_k=True)}),
    # three tiles per image: the tile -> (image, row) split is a real division
    "tiles3": ((2, 64, 32, 12, 64), {0: dict(R=4, tiles_per_img=3, ptiles=6), 1: dict(R=4, tiles_per_img=3, ptiles=6)}),
    # eight channel blocks on two / four workgroups: the reduction is cut into two runs + the ordered add
    "cut": ((1, 128, 128, 16, 16), {0: dict(nsplit=2, sps=8, ktiles=2), 1: dict(nsplit=2, sps=4, ktiles=2)}),
}


def check_cases():
    seen_k, seen_p = set(), set()
    for cid, (shape, need) in CASES.items():
        for mode in (0, 1):
            p = plan(mode, *shape)
            assert p is not None, (cid, mode)
            assert p["lds"] <= 160 * 1024 and p["items"] <= 512, (cid, mode, p)
            for k, v in need[mode].items():
                assert p[k] == v, (cid, mode, k, p[k], v)
            seen_k.add((p["ktiles"] > 1, p["ragged_k"]))
            seen_p.add(p["tiles_per_img"])
    # one and several k tiles, whole and ragged; one, two and three pixel tiles per image
    assert {(False, False), (False, True), (True, True), (True, False)} <= seen_k, seen_k
    assert {1, 2, 3} <= seen_p, seen_p
