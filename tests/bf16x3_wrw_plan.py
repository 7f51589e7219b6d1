"""The launch plan of the split-bf16 weight gradient on fp32 tensors (csrc/conv_bf16.hip, wrw_geometry on WRW_KINDS[WRW_3X3_SPLIT]), restated in Python, and the GPU
cases of tests/test_gpu_bf16x3_wrw.py with the variant each must reach.  No GPU, no library: tests/test_bf16x3_wrw_abi.py compares the
library's workspace query against `ws` here.

Tile = 128 a-channels x 32 w-channels (Conv2d: a = dy, w = x; ConvTranspose2d: a = x, w = dy), stage = 128 pixels = RS = 128 / W whole
image rows, `spw` stages per workgroup, B * (H / RS) / spw runs, one fp32 slab [9][ktiles * 128][ctiles * 32] per run.
"""


def plan(transposed, B, Cin, H, W, Cout):
    """None where the planner refuses."""
    Ka, Cb = (Cin, Cout) if transposed else (Cout, Cin)
    if min(B, Cin, Cout, H, W) < 1 or W not in (16, 32, 64, 128) or H % (128 // W):
        return None
    RS = 128 // W
    ktiles, ctiles, groups = (Ka + 127) // 128, (Cb + 31) // 32, H // RS
    spw = max(1, min(groups, (ktiles * ctiles * B * groups + 255) // 256))          # one round of one workgroup per CU
    while groups % spw:
        spw -= 1
    nsplit = B * (groups // spw)
    lds = 2 * 128 * 128 * 2 + 2 * (RS + 2) * 32 * (W // 8 + 3) * 16
    return dict(RS=RS, ktiles=ktiles, ctiles=ctiles, groups=groups, spw=spw, runs_per_img=groups // spw, nsplit=nsplit, lds=lds,
                ragged_k=Ka % 128 != 0, ragged_c=Cb % 32 != 0, ws=nsplit * 9 * ktiles * 128 * ctiles * 32 * 4)


# id: ((transposed, B, Cin, Cout, H, W), the plan fields the case is there for).  Every reduction B * H * W <= 2048 pixels: beyond that the
# error band of the GPU test no longer tells a dropped cross term from the full arithmetic.
# "wrap" differs from the bf16 tests' (0, 3, 48, 80, 32, 16): with so few tiles this planner (like the bf16 one) gives every stage a
# workgroup of its own; two stages per workgroup need more than 256 (tile, stage) pairs, i.e. >= 33 tiles on 8 stage groups.
CASES = {
    "one": ((0, 1, 16, 48, 8, 16), dict(groups=1, spw=1, nsplit=1, ktiles=1, ctiles=1, ragged_k=True, ragged_c=True)),
    "wrap": ((0, 2, 340, 380, 32, 16), dict(RS=8, groups=4, spw=2, runs_per_img=2, nsplit=4, ktiles=3, ctiles=11, ragged_k=True, ragged_c=True)),
    "w128": ((1, 2, 32, 64, 4, 128), dict(RS=1, groups=4, spw=1, nsplit=8, ctiles=2)),
    "w64": ((0, 2, 64, 128, 6, 64), dict(RS=2, groups=3, spw=1, nsplit=6)),
    "tiles": ((1, 5, 144, 72, 12, 32), dict(RS=4, ktiles=2, ctiles=3, ragged_k=True, ragged_c=True, nsplit=15)),
}


def check_cases():
    for cid, (shape, need) in CASES.items():
        tr, B, Cin, Cout, H, W = shape
        p = plan(tr, B, Cin, H, W, Cout)
        assert p is not None, cid
        assert B * H * W <= 2048, cid
        assert p["lds"] <= 160 * 1024, (cid, p["lds"])
        for k, v in need.items():
            assert p[k] == v, (cid, k, p[k], v)
