"""tests/bf16_conv_plan.py (the Python restatement of the launch planners of csrc/conv_bf16.hip) against the built library, without a GPU.

The library's workspace queries are pure functions of the shape.  Their byte counts hold the plan's k tile (kt), the number of
k tiles, the stages, the row phases and — through the fp32 partials / the slabs — the cut of the reduction:
    forward / input gradient   256 + align256(planes * ktiles * nphase * nstage * ntap * 2 * kt * 16) + align256(nsplit * B * K * Hout * Wout * 4) [nsplit > 1]
                               (planes: 1 on bf16 tensors, 2 = hi | lo on fp32 tensors with split-bf16 operands)
    k3 weight gradient         256 + nsplit * 9 * ktiles * 128 * ctiles * 64 * 4
    k4 s2 weight gradient      256 + nsplit * 16 * ktiles * 128 * ctiles * 32 * 4
and they are 0 exactly where the planner refuses.  So a retune of a planner fails here, before the GPU cases of
tests/test_gpu_bf16_conv_variants.py silently move onto other variants.

What the byte counts cannot pin: the pixel tile (256 / 512) and `raw1` of a shape that is accepted either way (neither changes the
packed weights nor the partials).  The sweep still crosses the 512 -> 256 fall-backs wherever only one of the two tile sizes is
accepted (e.g. H = 6 at W = 256: refused if the fall-back to one row per tile did not exist), and the LDS arithmetic is checked
against the figures written in conv_bf16.hip's own comments below.
"""
import itertools

import pytest

import bf16_conv_plan as P

BS = (1, 2, 3, 16)
CS = (16, 24, 48, 144, 208, 256, 512)
KS = (3, 16, 48, 64, 80, 160, 512)
HS = (2, 4, 6, 16, 24, 32, 48, 96, 128)
WS = (16, 24, 32, 64, 128, 256, 512)


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    from deepinpainting_amd import _lib
    return _lib.lib()


def _queries(lib, B, C, K, H, W):
    """The ten queries of one sweep point -> [(name, library's bytes, mirror's bytes)].  C = reduction channels of the forward forms."""
    def x3(kind, form, c, k):
        return P.data_ws_bytes(P.data_geometry(kind, form, B, c, k, H, W))
    return (("conv3x3 op0", lib.ipsr_conv3x3_bf16_workspace_bytes(0, B, C, H, W, K), P.k3_ws(0, B, C, H, W, K)),
            ("conv4x4s2 f2c", lib.ipsr_conv4x4s2_bf16_workspace_bytes(0, B, K, C, H, W), P.s2_ws(0, B, K, C, H, W)),
            ("conv4x4s2 c2f", lib.ipsr_conv4x4s2_bf16_workspace_bytes(1, B, C, K, H, W), P.s2_ws(1, B, C, K, H, W)),
            ("conv3x3 wrw", lib.ipsr_conv3x3_bf16_wrw_workspace_bytes(0, B, C, H, W, K), P.k3_wrw_ws(False, B, C, H, W, K)),
            ("conv4x4s2 wrw", lib.ipsr_conv4x4s2_bf16_wrw_workspace_bytes(B, K, C, H, W), P.s2_wrw_ws(B, K, C, H, W)),
            ("conv3x3 split op0", lib.ipsr_conv3x3_bf16x3_workspace_bytes(0, B, C, H, W, K), x3("k3_split", "S1", C, K)),
            ("conv4x4s2 split f2c", lib.ipsr_conv4x4s2_bf16x3_workspace_bytes(0, B, K, C, H, W), x3("s2_split", "F2C", C, K)),
            ("conv4x4s2 split c2f", lib.ipsr_conv4x4s2_bf16x3_workspace_bytes(1, B, C, K, H, W), x3("s2_split", "C2F", C, K)),
            ("conv4x4s2 split dilated f2c", lib.ipsr_conv4x4s2_bf16x3_workspace_bytes(4, B, K, C, H, W), x3("s2_split", "DF2C", C, K)),
            ("conv4x4s2 split dilated c2f", lib.ipsr_conv4x4s2_bf16x3_workspace_bytes(5, B, C, K, H, W), x3("s2_split", "DC2F", C, K)))


def test_mirror_matches_the_library_on_the_sweep(lib):
    n, bad, accepted, refused = 0, [], 0, 0
    for B, C, K, H, W in itertools.product(BS, CS, KS, HS, WS):
        for name, got, want in _queries(lib, B, C, K, H, W):
            n += 1
            accepted += got > 0
            refused += got == 0
            if got != want:
                bad.append((name, (B, C, K, H, W), got, want))
    print("%d queries, %d accepted, %d refused, %d mismatches" % (n, accepted, refused, len(bad)))
    assert n >= 120000 and accepted > 29000 and refused > 42000, (n, accepted, refused)
    assert not bad, (len(bad), bad[:8])


def test_mirror_matches_the_library_on_every_op_and_case_shape(lib):
    """All four ops of the k3 entry, the transposed weight gradient, and the exact shapes the GPU cases run (and their batch-of-one
    forms: nsplit depends on B through the workgroup count)."""
    bad = []
    for cid in P.ALL_CASE_IDS:
        if cid in P.K3_CASES or cid in P.K3_WRW_CASES:
            tr, Cin, H, W, Cout, B = (P.K3_CASES.get(cid) or P.K3_WRW_CASES[cid])[0]
            for b in {B, 1}:
                for op in range(4):
                    bad += [(cid, op, b)] * (lib.ipsr_conv3x3_bf16_workspace_bytes(op, b, Cin, H, W, Cout) != P.k3_ws(op, b, Cin, H, W, Cout))
                for t in (0, 1):
                    bad += [(cid, "wrw", t, b)] * (lib.ipsr_conv3x3_bf16_wrw_workspace_bytes(t, b, Cin, H, W, Cout) != P.k3_wrw_ws(t, b, Cin, H, W, Cout))
        else:
            Kc, Cf, nh, nw, B = (P.S2_CASES.get(cid) or P.S2_WRW_CASES[cid])[0]
            for b in {B, 1}:
                for mode in (0, 1):
                    bad += [(cid, mode, b)] * (lib.ipsr_conv4x4s2_bf16_workspace_bytes(mode, b, Kc, Cf, nh, nw) != P.s2_ws(mode, b, Kc, Cf, nh, nw))
                bad += [(cid, "wrw", b)] * (lib.ipsr_conv4x4s2_bf16_wrw_workspace_bytes(b, Kc, Cf, nh, nw) != P.s2_wrw_ws(b, Kc, Cf, nh, nw))
    assert not bad, bad


def test_lds_arithmetic_against_the_figures_in_the_source():
    """conv_bf16.hip, the LDS plan under CB_LDS_MAX: k3 at W <= 128: 2 x (36 + 16 + 16.3) KB; stride 2: 2 x (32 + 20 + 20.4); k3 at W = 256: 2 x 36 + 2 x 24.3 +
    ONE raw buffer of 24 KB."""
    g = P.cb_geometry(16, 128, 128, 128, 128)
    assert (g["a_bytes"], g["raw_bytes"], g["raw1"]) == (36 * 1024, 16 * 1024, False) and 16 * 1024 < g["t_bytes"] < 17 * 1024
    g = P.cb_geometry_s2(0, 16, 128, 128, 64, 64)
    assert (g["a_bytes"], g["raw_bytes"], g["raw1"]) == (32 * 1024, 20 * 1024, False) and 20 * 1024 < g["t_bytes"] < 21 * 1024
    g = P.cb_geometry(1, 64, 128, 256, 256)
    assert (g["a_bytes"], g["raw_bytes"], g["raw1"], g["R"]) == (36 * 1024, 24 * 1024, True, 1) and 24 * 1024 < g["t_bytes"] < 25 * 1024
    assert g["lds"] <= P.CB_LDS_MAX
    # the largest plan admitted: fine -> coarse, 64 produced channels, 512 pixels at nw = 128
    assert P.cb_geometry_s2(0, 1, 16, 64, 4, 128)["lds"] == 156672 <= P.CB_LDS_MAX
    # on every width a form accepts at all, the 512-pixel tile is turned down by the ROWS only: its LDS plan always fits (so the
    # "else 256" of data_geometry is reached through the rows check alone)
    for form, K, W, H in itertools.product(("k3", 0, 1), (16, 64), (16, 32, 64, 128, 256), (1, 2, 4, 8, 16, 32, 64)):
        g = P.cb_geometry(1, 16, K, H, W) if form == "k3" else P.cb_geometry_s2(form, 1, 16, K, H, W)
        assert g is None or g["p512"] in ("taken", "rows"), (form, K, W, H, g["p512"])


@pytest.mark.parametrize("cid", P.ALL_CASE_IDS)
def test_every_gpu_case_reaches_the_plan_written_beside_it(cid):
    P.check_case(cid)


@pytest.mark.parametrize("row", range(len(P.VARIANTS)), ids=lambda i: "row%02d" % i)
def test_every_row_of_the_variant_table_is_produced_by_its_cases(row):
    variant, lines, pred, cases = P.VARIANTS[row]
    assert cases, variant
    for cid, name in cases:
        plan = P.case_plans(cid)[name]
        assert plan is not None and pred(plan), "%s: case %s/%s reaches %s" % (variant, cid, name, plan)


def test_the_variant_table_in_the_gpu_module_names_every_row_and_case():
    """The docstring table of tests/test_gpu_bf16_conv_variants.py is generated from VARIANTS: every row's text and case ids appear."""
    import os
    src = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "test_gpu_bf16_conv_variants.py")).read()
    doc = src.split('"""')[1]
    for variant, lines, _, cases in P.VARIANTS:
        assert variant in doc, variant
        for cid, _ in cases:
            assert cid in doc, cid


def test_refusals_the_gpu_module_checks():
    """W 24, C % 16, rows not a multiple of R, F2C nw 256, weight gradient at W 256, s2 weight gradient at nw 128."""
    assert P.cb_geometry(1, 16, 16, 12, 24, why=True) == (None, "grid width 24")
    assert "not a multiple of 16" in P.cb_geometry(1, 24, 16, 16, 16, why=True)[1]
    assert "rows are not a multiple" in P.cb_geometry(1, 16, 128, 12, 32, why=True)[1]
    assert "LDS plan" in P.s2_plan(0, 1, 16, 16, 2, 256, why=True)[1]
    assert P.k3_wrw_plan(False, 1, 16, 4, 256, 16) is None and P.s2_wrw_plan(1, 16, 16, 4, 128) is None
