"""The launch plan of the split-bf16 weight gradient of the k4 s2 p1 layers on fp32 tensors (csrc/conv_bf16.hip, wrw_geometry on WRW_KINDS[WRW_S2_SPLIT]), restated in
Python, and the GPU cases of tests/test_gpu_bf16x3_s2_wrw.py with the variant each must reach.  No GPU, no library:
tests/test_bf16x3_s2_wrw_abi.py compares the library's workspace query against `ws` here.

Tile = 128 coarse channels x 32 fine channels x 16 taps, stage = 64 coarse pixels = RS = 64 / nw whole coarse rows, `spw` stages per
workgroup, B * (nh / RS) / spw runs, one fp32 slab [16][ktiles * 128][ctiles * 32] per run.  LDS = coarse hi | lo (2 x 16 KB) + a ring of
RS + 1 pairs of fine rows, hi | lo.
"""


def plan(B, Kc, Cf, nh, nw):
    """None where the planner refuses (nw = 128 included: whole fine rows for a half-row stage need 176128 bytes of LDS)."""
    if min(B, Kc, Cf, nh, nw) < 1 or nw not in (16, 32, 64) or nh % (64 // nw):
        return None
    RS = 64 // nw
    ktiles, ctiles, groups = (Kc + 127) // 128, (Cf + 31) // 32, nh // RS
    spw = max(1, min(groups, (ktiles * ctiles * B * groups + 255) // 256))          # one round of one workgroup per CU
    while groups % spw:
        spw -= 1
    nsplit = B * (groups // spw)
    lds = 2 * 128 * 64 * 2 + 2 * (RS + 1) * 2 * 32 * (2 * nw // 8 + 3) * 16
    return dict(RS=RS, ktiles=ktiles, ctiles=ctiles, groups=groups, spw=spw, runs_per_img=groups // spw, nsplit=nsplit, lds=lds,
                ragged_k=Kc % 128 != 0, ragged_c=Cf % 32 != 0, ws=nsplit * 16 * ktiles * 128 * ctiles * 32 * 4)


# id: ((B, Kc, Cf, nh, nw), the plan fields the case is there for).  Every reduction B * nh * nw <= 2048 coarse pixels: beyond that the
# error band of the GPU test no longer tells a dropped cross term from the full arithmetic.  No "w128": the kernel refuses nw = 128.
CASES = {
    "one": ((1, 48, 16, 4, 16), dict(RS=4, groups=1, spw=1, nsplit=1, ktiles=1, ctiles=1, ragged_k=True, ragged_c=True)),
    "wrap": ((2, 340, 380, 16, 16), dict(RS=4, groups=4, spw=2, runs_per_img=2, nsplit=4, ktiles=3, ctiles=12, ragged_k=True, ragged_c=True)),
    "w32": ((1, 144, 72, 6, 32), dict(RS=2, groups=3, spw=1, ktiles=2, ctiles=3, ragged_k=True, ragged_c=True, nsplit=3)),
    "w64": ((2, 64, 128, 3, 64), dict(RS=1, groups=3, spw=1, runs_per_img=3, nsplit=6, ktiles=1, ctiles=4, ragged_k=True)),
    "batch": ((5, 32, 40, 4, 32), dict(RS=2, groups=2, nsplit=10, ragged_k=True, ragged_c=True)),
}


def check_cases():
    for cid, (shape, need) in CASES.items():
        B, Kc, Cf, nh, nw = shape
        p = plan(B, Kc, Cf, nh, nw)
        assert p is not None, cid
        assert B * nh * nw <= 2048, cid
        assert p["lds"] <= 160 * 1024, (cid, p["lds"])
        for k, v in need.items():
            assert p[k] == v, (cid, k, p[k], v)
    assert plan(1, 32, 64, 2, 128) is None
