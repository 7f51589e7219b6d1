"""tests/thin_conv_plan.py (the Python restatement of the launchers of csrc/thin_conv.hip) against the built library, without a GPU.

The library's three workspace queries and `ipsr_conv_thin_f2m_mfma_supported` are host functions of the shape:
    ipsr_conv_thin_wrw_mfma_workspace_bytes   align256(ktiles * B * gx * 32 MT * 32 RT * 4) + 256: MT, RT, ktiles and — through gx — rows
    ipsr_conv3x3_thin_wrw_workspace_bytes     align256(grid.x * grid.y * grid.z * 2 * Cs * 9 * 4) + 256: the whole grid
    ipsr_conv_to_one_workspace_bytes          align256(B * ceil(C/8) * Ho * Wo * 4) + 256, 0 beyond 256 pixel groups
and each is 0 exactly where its launcher refuses.  The few -> many matrix-core launcher has no workspace: its refusal is compared,
its (MT, KS, rows) are the same arithmetic as the weight gradient's (MT, RT, rows), which the byte counts do pin.  So a retune of a
plan constant fails here, before the GPU cases of tests/test_gpu_thin_variants.py silently move onto a neighbouring variant.
"""
import itertools

import pytest

import thin_conv_plan as P


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    from deepinpainting_amd import _lib
    return _lib.lib()


def test_mirror_matches_the_library_on_the_sweep(lib):
    bad, n, accepted = [], 0, 0

    def cmp(name, args, got, want):
        nonlocal n, accepted
        n += 1
        accepted += got > 0
        if got != want:
            bad.append((name, args, got, want))

    for B, C, H, W, (k, st) in itertools.product((1, 2, 9, 17, 33), (0, 2, 3, 4, 6, 8, 12, 72, 128, 136), (1, 4, 5, 64, 65, 130, 242, 250),
                                                 (4, 16, 30, 32, 48, 256, 260), ((3, 1), (4, 2), (3, 2), (5, 1))):
        for Cs in (3, 6, 4):
            a = (B, C, Cs, H, W, k, st)
            cmp("wrw_mfma ws", a, lib.ipsr_conv_thin_wrw_mfma_workspace_bytes(*a), P.thin_wrw_mfma_ws(*a))
            f = (B, Cs, C, H, W, k, st)
            cmp("f2m_mfma supported", f, lib.ipsr_conv_thin_f2m_mfma_supported(*f), int(P.thin_f2m_mfma_plan(*f) is not None))
            if (k, st) == (3, 1):
                cmp("thin_wrw ws", a[:5], lib.ipsr_conv3x3_thin_wrw_workspace_bytes(*a[:5]), P.thin_wrw_ws(*a[:5]))
    for B, C, H, W, K, pad in itertools.product((1, 2, 16), (1, 7, 8, 9, 512), (3, 4, 5, 31, 33, 34), (3, 4, 9, 30, 33, 34, 1030), (2, 3, 4, 5), (0, 1, 2)):
        a = (B, C, H, W, K, pad)
        cmp("to_one ws", a, lib.ipsr_conv_to_one_workspace_bytes(*a), P.to_one_ws(*a))
    print("%d queries, %d accepted, %d mismatches" % (n, accepted, len(bad)))
    assert n > 15000 and 2000 < accepted < n - 2000, (n, accepted)
    assert not bad, (len(bad), bad[:8])


def test_mirror_matches_the_library_on_every_case_shape(lib):
    for cid, (case, _) in P.F2M_MFMA_CASES.items():
        assert lib.ipsr_conv_thin_f2m_mfma_supported(*P.f2m_mfma_geometry(case)) == 1, cid
    for cid, ((Kb, Cs, k, B, Hb, Wb), _) in P.WRW_MFMA_CASES.items():
        assert lib.ipsr_conv_thin_wrw_mfma_workspace_bytes(B, Kb, Cs, Hb, Wb, k, 1 if k == 3 else 2) == P.case_plan(cid)["ws"], cid
    for cid, (case, _) in P.WRW_CASES.items():
        assert lib.ipsr_conv3x3_thin_wrw_workspace_bytes(*case) == P.case_plan(cid)["ws"], cid
    for cid, (case, _) in P.TO_ONE_CASES.items():
        assert lib.ipsr_conv_to_one_workspace_bytes(*case) == P.case_plan(cid)["ws"], cid
    for cid, case in P.TO_ONE_REFUSED.items():
        assert lib.ipsr_conv_to_one_workspace_bytes(*case) == 0 and P.to_one_plan(*case) is None, cid


@pytest.mark.parametrize("cid", P.ALL_CASE_IDS)
def test_every_gpu_case_reaches_the_path_written_beside_it(cid):
    P.check_case(cid)


@pytest.mark.parametrize("row", range(len(P.VARIANTS)), ids=lambda i: "row%02d" % i)
def test_every_row_of_the_variant_table_is_produced_by_its_cases(row):
    variant, lines, pred, cases = P.VARIANTS[row]
    assert cases, variant
    for cid in cases:
        plan = P.case_plan(cid)
        assert plan is not None and pred(plan), "%s: case %s reaches %s" % (variant, cid, plan)


def test_the_tables_reach_every_variant_and_edge():
    """The coverage claims, from the plans alone: all seven (MT, KS) and all five (MT, RT) pairs, rows > 4 and a ragged last group in
    both matrix-core kernels, more than one block on every grid axis of the three vector-ALU kernels, both template arguments and
    both `flip` values of the two data kernels, the LDS edge of many -> few and the 256-group limit of conv_to_one."""
    fm = [P.case_plan(c) for c in P.F2M_MFMA_CASES]
    assert {(p["MT"], p["KS"]) for p in fm} == {(4, 2), (4, 3), (4, 4), (2, 2), (2, 3), (2, 4), (2, 6)}
    assert any(p["rows"] > 4 and p["ragged"] for p in fm) and any(p["rows"] == 4 and p["idle_waves"] == 1 for p in fm)
    assert all(p["ragged"] for p in fm)
    wm = [P.case_plan(c) for c in P.WRW_MFMA_CASES]
    assert {(p["MT"], p["RT"]) for p in wm} == {(4, 1), (4, 2), (2, 1), (2, 2), (2, 3)}
    assert {p["limit"] for p in wm if p["rows"] > 4 and p["ragged"]} == {512, 1024}
    assert any(p["rows"] == 4 and p["ragged"] for p in wm)
    for table in (P.F2M_CASES, P.M2F_CASES, P.WRW_CASES):
        plans = [P.case_plan(c) for c in table]
        assert {p["T"] for p in plans} == {3, 6}, table
        for axis in range(3):
            assert any(p["grid"][axis] >= 2 for p in plans), (list(table), axis)
    # every data case runs as Conv2d(few, many), Conv2d(many, few), ConvTranspose2d(few, many), ConvTranspose2d(many, few), forward
    # and input gradient: each kernel meets flip 0 and flip 1
    seen = set()
    for few, many in ((3, 16), (6, 32)):
        for Cin, Cout in ((few, many), (many, few)):
            for op in range(4):
                kop, I, O, flip = P.thin_module_pass(op, Cin, Cout)
                seen.add((kop, flip))
    assert seen == {(0, 0), (0, 1), (1, 0), (1, 1)}
    # the edges: the last accepted and the first refused
    assert P.thin_io_plan(1, 1, 455, 3, 2, 8)["lds"] <= P.LDS_M2F < 456 * 3 * 36 and P.thin_io_plan(1, 1, 456, 3, 2, 8) is None
    assert P.thin_io_plan(1, 1, 227, 6, 3, 4)["lds"] <= P.LDS_M2F < 228 * 6 * 36 and P.thin_io_plan(1, 1, 228, 6, 3, 4) is None
    for cid, case in P.THIN_IO_REFUSED.items():
        assert P.thin_io_plan(*case) is None, cid
    assert P.thin_io_plan(0, 1, 3, 16, 2, 8) is not None                                  # (the even width beside the refused odd one)
    ones = [P.case_plan(c) for c in P.TO_ONE_CASES]
    assert {p["groups"] for p in ones} >= {1, 256} and {p["K"] for p in ones} == {3, 4} and {p["pad"] for p in ones} == {0, 1, 2}
    assert all(max(p["lds_fwd"], p["lds_wrw"]) <= P.LDS_ONE for p in ones)
    assert P.to_one_plan(*P.TO_ONE_REFUSED["one_b1_c8_34x33_k4p1"]) is None and P.to_one_plan(1, 8, 33, 33, 4, 1)["groups"] == 256


def test_thin_supported_agrees_with_the_launcher_on_the_case_shapes(lib):
    """ops.thin_supported (ops.py:812-818) accepts every data case in all four module readings and refuses the three refused shapes."""
    from deepinpainting_amd import ops
    for table in (P.F2M_CASES, P.M2F_CASES):
        for cid, ((B, few, many, H, W), _) in table.items():
            for Cin, Cout in ((few, many), (many, few)):
                for op in range(4):
                    kop, I, O, _ = P.thin_module_pass(op, Cin, Cout)
                    assert ops.thin_supported(op, Cin, H, W, Cout) == (P.thin_io_plan(kop, B, I, O, H, W) is not None), (cid, op, Cin, Cout)
    assert not ops.thin_supported(ops.CONV_FWD, 3, 2, 7, 16)
    assert not ops.thin_supported(ops.CONV_FWD, 456, 2, 8, 3) and not ops.thin_supported(ops.CONV_FWD, 228, 3, 4, 6)


def test_the_variant_table_in_the_gpu_module_names_every_row_and_case():
    """The docstring table of tests/test_gpu_thin_variants.py is generated from VARIANTS: every row's text and case ids appear."""
    import os
    src = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "test_gpu_thin_variants.py")).read()
    doc = src.split('"""')[1]
    for variant, lines, _, cases in P.VARIANTS:
        assert variant in doc and lines in doc, variant
        for cid in cases:
            assert cid in doc, cid
