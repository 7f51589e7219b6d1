"""tests/fp32_conv_plan.py (the Python restatement of `sm_plan` of csrc/smallmap.hip and of `make_plan` / `choose_split` /
`launch_conv_gemm` of csrc/conv_gemm.hip) against the built library, without a GPU.

The two workspace queries are host functions of the shape, 0 exactly where the entry point refuses:
    ipsr_conv_smallmap_workspace_bytes   DATA  align256(R Tp 4) + align256(nslab Q Tp 4) + 256
                                         FWD   align256(Q Tp 4) + align256(nslab R Tp 4) + 256
                                         WRW   align256(Pp R 4) + align256(Pp Q 4) + 256
    ipsr_conv2d_workspace_bytes          sum over the launched classes of align256(nstage BK Mp 4), + align256(4 max(ksplit M ntot)) + 256
So the byte counts pin Tp (the product nb * ngroups), Pp, nslab, Mp, every class's nstage * BK (with it the class set and the channels
per stage) and the largest ksplit * ntot.  They do NOT pin: `per_slab` other than through nslab (two values that give the same slab
count are told apart only by the GPU cases); nb and ngroups separately; stages_per_split (the last split's length follows from it); the
tap tables (dy0, dys, dx0, dxs) and the class grids of a call without split-K.  Those are arithmetic restated line by line in the mirror,
and a wrong tap table or grid is what the exact regime of tests/test_gpu_fp32_conv_variants.py catches.

A retune of a plan constant fails here, before the GPU cases silently move onto a neighbouring variant.
"""
import itertools
import os

import pytest

import fp32_conv_plan as P


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    from deepinpainting_amd import _lib
    return _lib.lib()


def test_smallmap_mirror_matches_the_library_on_the_sweep(lib):
    """k 1..4, stride 1..3, dilation 1..3, pad 0..3; Cq on and off the multiples that make Cq k k a multiple of 128, R on and off 32;
    P either side of 1024 (B 1, 4, 17 on grids up to 32 x 34); the right output grid, and a wrong one."""
    bad, n, accepted = [], 0, 0
    for k, st, dil, pad in itertools.product((1, 2, 3, 4), (1, 2, 3), (1, 2, 3), (0, 1, 2, 3)):
        for (Hf, Wf), B, R, Cq in itertools.product(((1, 1), (2, 2), (3, 3), (6, 6), (8, 7), (16, 16), (32, 32), (32, 34)), (1, 4, 17), (32, 48, 224, 2),
                                                    (8, 12, 32, 100, 120, 128)):
            Ho, Wo = P.conv_out_dim(0, Hf, k, st, pad, dil), P.conv_out_dim(0, Wf, k, st, pad, dil)
            for Ho_, Wo_ in ((Ho, Wo), (Ho + 1, Wo)) if (Hf + k + pad) % 5 == 0 else ((Ho, Wo),):
                for op in (0, 1, 2, 3):
                    a = (op, B, R, Cq, Ho_, Wo_, Hf, Wf, k, st, pad, dil)
                    got, want = lib.ipsr_conv_smallmap_workspace_bytes(*a), P.sm_ws(*a)
                    n += 1
                    accepted += got > 0
                    if got != want:
                        bad.append((a, got, want))
    print("%d queries, %d accepted, %d mismatches" % (n, accepted, len(bad)))
    assert n > 20000 and accepted > 1500 and n - accepted > 1500, (n, accepted)
    assert not bad, (len(bad), bad[:8])


def test_conv2d_mirror_matches_the_library_on_the_sweep(lib):
    """All four ops; k 1..5, stride 1..3, dilation 1..3, pad 0..3; channel counts on and off the multiples of 2, 4 and 128 (1, 2, 3, 4, 6,
    30, 130, 136); maps 1 x 1 .. 24 x 23; and one shape whose input is 2 GiB (refused: the gather's offsets are 32 bits)."""
    bad, n, accepted = [], 0, 0
    chans = ((1, 4), (2, 5), (3, 12), (4, 3), (6, 136), (8, 8), (30, 2), (130, 70), (136, 6), (4, 1))
    for k, st, dil, pad in itertools.product((1, 2, 3, 4, 5), (1, 2, 3), (1, 2, 3), (0, 1, 2, 3)):
        for (Cin, Cout), (H, W), B in itertools.product(chans, ((1, 1), (2, 2), (5, 6), (9, 13), (24, 23)), (1, 3)):
            for op in range(4):
                a = (op, B, Cin, H, W, Cout, k, st, pad, dil)
                got, want = lib.ipsr_conv2d_workspace_bytes(*a), P.conv2d_ws(*a)
                n += 1
                accepted += got > 0
                if got != want:
                    bad.append((a, got, want))
    print("%d queries, %d accepted, %d mismatches" % (n, accepted, len(bad)))
    assert n > 50000 and accepted > 5000 and n - accepted > 5000, (n, accepted)
    assert not bad, (len(bad), bad[:8])
    # 2 x 64 x 2048 x 2048 floats = 2 GiB: refused by op 0, which reads it; one sample of it is served
    big = (0, 2, 64, 2048, 2048, 8, 3, 1, 1, 1)
    assert lib.ipsr_conv2d_workspace_bytes(*big) == 0 and P.conv2d_plan(*big) is None
    assert b"too large" in lib.ipsr_last_error()
    half = (0, 1, 64, 2048, 2048, 8, 3, 1, 1, 1)
    assert lib.ipsr_conv2d_workspace_bytes(*half) == P.conv2d_ws(*half) > 0


def test_mirror_matches_the_library_on_every_case_shape(lib):
    from deepinpainting_amd import ops
    for cid, (case, req) in P.SM_CASES.items():
        geo = P.sm_geometry(case)
        for op in (P.SM_DATA, P.SM_WRW, P.SM_FWD):
            assert op in req, (cid, op)
            assert lib.ipsr_conv_smallmap_workspace_bytes(op, *geo) == P.sm_plan(op, *geo)["ws"], (cid, op)
            assert ops.smallmap_supported(op, *geo)
    for cid, case in P.SM_REFUSED.items():
        geo = P.sm_geometry(case)
        for op in (P.SM_DATA, P.SM_WRW, P.SM_FWD):
            assert lib.ipsr_conv_smallmap_workspace_bytes(op, *geo) == 0 and P.sm_plan(op, *geo) is None, (cid, op)
            assert not ops.smallmap_supported(op, *geo)
    for cid, (case, req) in P.CG_CASES.items():
        for which in req:
            a = P.cg_args(case, which)
            assert lib.ipsr_conv2d_workspace_bytes(*a) == P.conv2d_plan(*a)["ws"], (cid, which)
            assert ops.conv2d_supported(*a)
    for cid, (case, refused, why) in P.CG_REFUSED.items():
        for which in refused:
            a = P.cg_args(case, which)
            assert lib.ipsr_conv2d_workspace_bytes(*a) == 0 and P.conv2d_plan(*a) is None, (cid, which, why)
            assert not ops.conv2d_supported(*a)


@pytest.mark.parametrize("pid", P.ALL_PLAN_IDS)
def test_every_gpu_case_reaches_the_path_written_beside_it(pid):
    P.check_case(pid)


def test_every_variant_is_reached():
    """Each row of the variant table is produced by every case written beside it (and names at least one)."""
    for variant, lines, pred, cases in P.VARIANTS:
        assert cases, variant
        for pid in cases:
            assert pid in P.ALL_PLAN_IDS, (variant, pid)
            plan = P.case_plan(pid)
            assert plan is not None and pred(plan), "%s: case %s reaches %s" % (variant, pid, {k: v for k, v in plan.items() if k not in ("classes", "live", "waves")})


def test_the_tables_reach_every_kernel_and_edge():
    """The coverage claims from the plans alone: every instantiation of the five kernels, blockIdx.z > 0 in both data kernels, every
    prologue branch of conv_gemm_kernel on each tap count, and the edges of the entry points (1024 positions / 1088, odd P)."""
    sm = {pid: P.case_plan(pid) for pid in P.ALL_PLAN_IDS if pid.split(":")[0] in P.SM_CASES}
    assert {p["kernel"] for p in sm.values()} == {"sm_data_kernel<1>", "sm_data_kernel<2>", "sm_fwd_kernel<1>", "sm_fwd_kernel<2>", "sm_fwd_kernel<4>", "sm_wrw_kernel"}
    for kern in ("sm_data_kernel<2>", "sm_fwd_kernel<4>"):
        assert any(p["kernel"] == kern and p["grid"][2] > 1 for p in sm.values()), kern
    assert max(p["P"] for p in sm.values()) == 1024 and any(p["P"] % 2 for p in sm.values())
    assert {p["blocks"] for p in sm.values()} >= {1, 2, 3, 4, 7, 32}
    for op in (P.SM_DATA, P.SM_FWD):
        assert any(p["op"] == op and p["short_waves"] for p in sm.values()) and any(p["op"] == op and p["nslab"] > 1 for p in sm.values())
    cg = [P.case_plan(pid) for pid in P.ALL_PLAN_IDS if pid.split(":")[0] in P.CG_CASES]
    seen = {(c["NT"], c["nstage"]) for p in cg for c in p["live"] if c["ksplit"] == 1}
    assert seen >= {(NT, n) for NT in (4, 9, 16) for n in (1, 2, 3, 5, 15)}
    # with split-K a workgroup's stage count is stages_per_split or the last split's: 1 and 2 (the short prologues) and >= 8 are met
    split = {n for p in cg for c in p["live"] if c["ksplit"] > 1 for n in (c["stages_per_split"], c["last_split_stages"])}
    assert {1, 2, 8, 9} <= split


def test_no_data_wave_is_idle_within_the_case_limits():
    """`ra == rb` in sm_data_kernel needs 4 nslab per_slab - R >= per_slab.  per_slab = even(ceil(R / 4 ns)) with ns <= R / 64, so for
    every R <= 224 (the channel limit of the GPU cases) and every ns the slabs cover R with less than one wave to spare: the only
    inexact split is R = 224, ns = 3 (per_slab 20, 16 rows over: the short wave of conv8_224_6x6_k4s2_b1).  The first R with an idle
    wave is 416 (ns = 5, per_slab 22, 24 rows over); the nets' own R (512, 1024) split exactly.  FWD, whose per_slab rounds to 8, does
    meet one at Cq = 120: conv120_32_8x8_k4s2_b1."""
    def spare(R, ns):
        per = (P.cdiv(R, 4 * ns) + 1) & ~1
        return 4 * P.cdiv(R, 4 * per) * per - R, per
    for R in range(32, 225, 32):
        for ns in range(1, max(1, R // 64) + 1):
            over, per = spare(R, ns)
            assert over < per, (R, ns, over, per)
            assert over == 0 or (R, ns, per, over) == (224, 3, 20, 16)
    assert spare(416, 5) == (24, 22) and all(spare(R, ns)[0] == 0 for R in (512, 1024) for ns in (1, 2, 4, 8))
    first = min(R for R in range(32, 1025, 32) for ns in range(1, R // 64 + 1) if spare(R, ns)[0] >= spare(R, ns)[1])
    assert first == 416
    # and the library agrees on what it can: no accepted DATA plan of the sweep's channel counts has an idle wave
    for R, Cq, B in itertools.product(range(32, 225, 32), (8, 32, 120), (1, 4, 17)):
        for Hf in (2, 6, 8, 16, 32):
            p = P.sm_plan(P.SM_DATA, B, R, Cq, Hf // 2, Hf // 2, Hf, Hf, 4, 2, 1, 1)
            assert p is None or p["idle_waves"] == 0


def test_launch_time_refusals_of_the_parity_form_cannot_fire():
    """launch_conv_gemm refuses an irregular tap set and `nr != nsx` (conv_gemm.hip:430-434) after make_plan, i.e. after the workspace
    query has answered and after earlier classes were launched.  For k <= 4 and stride 2 neither can fire: with odd dilation a parity
    holds the taps r of one parity (at most two: any two form a progression), with even dilation it holds all or none; and n taps on y
    times m on x is 4, 9 or 16 with n != m only as 1 x 4 / 4 x 1, which needs 5 taps on an axis.  Enumerated here, so that the query and
    the launch refuse the same shapes."""
    for k, pad, dil in itertools.product((1, 2, 3, 4), range(0, 8), range(1, 8)):
        taps = [P.axis_taps(k, 2, pad, dil, par) for par in (0, 1)]
        for rr, off in taps:
            assert P._progression(rr) and P._progression(off)
        for (ry, _), (rx, _) in itertools.product(taps, taps):
            assert len(ry) == len(rx) or len(ry) * len(rx) not in (4, 9, 16)


def test_the_variant_table_in_the_gpu_module_names_every_row_and_case():
    """The docstring table of tests/test_gpu_fp32_conv_variants.py is generated from VARIANTS: every row's text, lines and case ids appear."""
    src = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "test_gpu_fp32_conv_variants.py")).read()
    doc = src.split('"""')[1]
    for variant, lines, _, cases in P.VARIANTS:
        assert variant in doc and lines in doc, variant
        for pid in cases:
            assert pid in doc, pid
    for cid in list(P.SM_REFUSED) + list(P.CG_REFUSED):
        assert cid in doc, cid
