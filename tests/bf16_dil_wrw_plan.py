"""The launch plan of the direct bf16 weight gradient of the dilated layer Conv2d(k4, stride 2, pad 3, dilation 2) on bf16 tensors
(csrc/conv_bf16.hip, wrw_geometry on WRW_KINDS[WRW_DIL]), restated in Python, and the GPU cases of tests/test_gpu_bf16_dil_wrw.py with the
variant each must reach.  No GPU, no library: tests/test_bf16_dil_wrw_abi.py compares the library's workspace query against `ws` here.

Tile = 128 coarse channels x 32 fine channels x 16 taps, stage = 64 coarse pixels = RS = 64 / nw whole coarse rows (nw = 128: half a row;
RS = 1 and the cut is by rows, two stages each), `spw` cut units per workgroup, B * (nh / RS) / spw runs, one fp32 slab
[16][ktiles * 128][ctiles * 32] per run behind a 256-byte zero page.  LDS = coarse, two buffers of 16 KB filled by LDS-DMA, + a ring of
RS + 3 rows of q = fine(odd, odd) in ONE plane, each (row, channel) nw / 8 + 3 slots of 16 bytes (one halo slot in front, one behind, an
odd pitch):
    nw = 16: 32768 + 17920 = 50688     nw = 32: 32768 + 17920 = 50688     nw = 64: 32768 + 22528 = 55296     nw = 128: 32768 + 38912 = 71680
"""


def plan(B, Kc, Cf, nh, nw):
    """None where the planner refuses."""
    if min(B, Kc, Cf, nh, nw) < 1 or nw not in (16, 32, 64, 128) or nh % max(1, 64 // nw):
        return None
    RS = max(1, 64 // nw)
    ktiles, ctiles, groups = (Kc + 127) // 128, (Cf + 31) // 32, nh // RS
    spw = max(1, min(groups, (ktiles * ctiles * B * groups + 255) // 256))          # one round of one workgroup per CU
    while groups % spw:
        spw -= 1
    nsplit = B * (groups // spw)
    ring = (RS + 3) * 32 * (nw // 8 + 3) * 16
    return dict(RS=RS, ktiles=ktiles, ctiles=ctiles, groups=groups, spw=spw, runs_per_img=groups // spw, nsplit=nsplit, ring=ring,
                lds=2 * 128 * 64 * 2 + ring, wide=nw == 128, steps=spw * (2 if nw == 128 else 1),
                ragged_k=Kc % 128 != 0, ragged_c=Cf % 32 != 0, ws=256 + nsplit * 16 * ktiles * 128 * ctiles * 32 * 4)


# id: ((B, Kc, Cf, nh, nw), the plan fields the case is there for).  Every reduction B * nh * nw <= 2048 coarse pixels.  The nine shapes of
# tests/bf16x3_dil_wrw_plan.py: tile and run cut are the same, so they reach the same variants.
CASES = {
    "one": ((1, 48, 16, 4, 16), dict(RS=4, groups=1, spw=1, steps=1, nsplit=1, ktiles=1, ctiles=1, ragged_k=True, ragged_c=True, ring=17920)),
    # several tiles, two stages per run: the coarse buffers swap, the ring takes new rows and wraps
    "wrap": ((2, 340, 380, 16, 16), dict(RS=4, groups=4, spw=2, steps=2, runs_per_img=2, nsplit=4, ktiles=3, ctiles=12, ragged_k=True, ragged_c=True)),
    "w32": ((1, 144, 72, 6, 32), dict(RS=2, groups=3, spw=1, ktiles=2, ctiles=3, ragged_k=True, ragged_c=True, nsplit=3, ring=17920)),
    "w64": ((2, 64, 128, 3, 64), dict(RS=1, groups=3, spw=1, runs_per_img=3, nsplit=6, ktiles=1, ctiles=4, ragged_k=True, ring=22528)),
    "batch": ((5, 32, 40, 4, 32), dict(RS=2, groups=2, nsplit=10, ragged_k=True, ragged_c=True)),
    # nh = 1: the row taps 0, 1 and 3 meet only rows outside the image
    "row1": ((1, 16, 32, 1, 64), dict(RS=1, groups=1, spw=1, nsplit=1, ragged_k=True)),
    "w128": ((1, 32, 64, 2, 128), dict(RS=1, wide=True, groups=2, spw=1, steps=2, nsplit=2, ring=38912, lds=71680)),
    "cut": ((8, 128, 32, 16, 16), dict(RS=4, groups=4, spw=1, nsplit=32, ktiles=1, ctiles=1, ragged_k=False, ragged_c=False)),
    # the 128-wide kernel with more than one row per run: a row arrives between two stages and the four-row ring wraps (in "w128" a run is
    # one row and every row it reads comes from the prologue)
    "w128ring": ((1, 256, 800, 16, 128), dict(RS=1, wide=True, groups=16, spw=4, steps=8, runs_per_img=4, nsplit=4, ktiles=2, ctiles=25)),
}
# netG's four dilated down convolutions as (Kc, Cf, nh, nw)
STEP_ROWS = [(64, 64, 128, 128), (128, 128, 64, 64), (256, 256, 32, 32), (512, 512, 16, 16)]
LDS = {16: 50688, 32: 50688, 64: 55296, 128: 71680}


def check_cases():
    for cid, (shape, need) in CASES.items():
        B, Kc, Cf, nh, nw = shape
        p = plan(B, Kc, Cf, nh, nw)
        assert p is not None, cid
        assert B * nh * nw <= 2048, cid
        assert p["lds"] <= 160 * 1024, (cid, p["lds"])
        for k, v in need.items():
            assert p[k] == v, (cid, k, p[k], v)
    for nw, lds in LDS.items():
        assert plan(1, 1, 1, 4, nw)["lds"] == lds
