"""The launch plan of the split-bf16 direct kernel for the k4 s2 p1 layers on fp32 tensors (csrc/conv_bf16.hip, c2_geometry), restated in
Python, and the cases of tests/test_gpu_bf16x3_s2.py with the variant each must reach.  No GPU, no library: tests/test_bf16x3_s2_abi.py
compares the library's workspace query against `ws` here.

Shapes are (B, Kc, Cf, nh, nw): fine [B,Cf,2nh,2nw], coarse [B,Kc,nh,nw], weight [Kc,Cf,4,4].  mode 0 = fine -> coarse (reduces Cf, produces
Kc, two sub-stages per 16-channel block: one per input row parity), mode 1 = coarse -> fine (reduces Kc, produces Cf, one workgroup per
output row parity).  The lane grid is the coarse one in both: tile = 64 produced channels x 256 coarse pixels = R = 256 / nw coarse rows.
The plan has ONE k tile (64 rows) and ONE pixel tile (256): what varies is how many of each a launch has, the stage count and the cut.
"""


def _align(v, a):
    return (v + a - 1) // a * a


def plan(mode, B, Kc, Cf, nh, nw):
    """None where the planner refuses."""
    if mode not in (0, 1) or min(B, Kc, Cf, nh, nw) < 1:
        return None
    C, K = (Cf, Kc) if mode == 0 else (Kc, Cf)                    # reduction / produced channels
    if C % 16 or nw not in (16, 32, 64, 128) or nh % (256 // nw):
        return None
    R = 256 // nw
    nsub, nphase = (2, 1) if mode == 0 else (1, 2)
    NR, PW, Win = (R + 1, nw + 1, 2 * nw) if mode == 0 else (R + 2, nw + 2, nw)
    ktiles, ptiles, nblocks = (K + 63) // 64, B * (nh // R), C // 16
    nstage = nblocks * nsub
    wgs, ns = ktiles * nphase * ptiles, 1
    if wgs < 128 and nblocks >= 8:
        ns = min(4, nblocks // 4, (256 + wgs - 1) // wgs)
    bps = (nblocks + ns - 1) // ns
    nsplit = (nblocks + bps - 1) // bps
    t_bytes = _align(2 * nsub * 2 * NR * PW * 16, 256)
    lds, items = 2 * 32768 + t_bytes, 2 * NR * (Win // 4)
    if lds > 160 * 1024 or items > 512:
        return None
    Hout, Wout = (nh, nw) if mode == 0 else (2 * nh, 2 * nw)
    pack = ktiles * nphase * nstage * 8 * 2 * 64 * 16             # one plane
    ws = 256 + _align(2 * pack, 256) + (_align(nsplit * B * K * Hout * Wout * 4, 256) if nsplit > 1 else 0)
    return dict(R=R, NR=NR, ktiles=ktiles, tiles_per_img=nh // R, ptiles=ptiles, nstage=nstage, nsplit=nsplit, sps=bps * nsub, lds=lds, items=items,
                ragged_k=K % 64 != 0, ws=ws)


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
