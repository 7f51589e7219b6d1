"""tests/corr_plan.py (the Python restatement of the launchers of csrc/corr_argmax.hip) against the built library, without a GPU.

The library's workspace queries are host functions of the shape:
    ipsr_corr_argmax_workspace_bytes          2 align256(B ksplit N 4) + 256: ksplit, and through it kt_per_wg = ceil(ktiles / ksplit)
                                              wherever the cost loop's choice is the smallest kt_per_wg with that ksplit
    ipsr_corr_argmax_bf16_workspace_bytes     the same plus the two packed operands
    ipsr_forward_workspace_bytes, ipsr_forward_bf16corr_workspace_bytes
                                              the layer's fifteen slices; at patch > 1 the WS_RU slice holds `window_plan`'s launched slice
                                              count (2 align256(B slices N' 4) + ...), which no other query shows
So a retune of a plan constant fails here, before the GPU cases of tests/test_gpu_corr_variants.py silently move onto a neighbouring
plan.  `innercos_workspace_bytes` is a constant (4096 doubles + 256) and pins nothing: the InnerCos plan, the backward's grid and the
index kernel's chunks are restated from the source alone.
"""
import itertools

import pytest

import corr_plan as P


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    from deepinpainting_amd import _lib
    return _lib.lib()


BATCHES = (1, 2, 3, 4, 8, 16, 32, 33, 41, 57, 64)
SIZES = tuple(sorted({n for m in range(128, 4097, 128) for n in (m - 1, m, m + 1)} | {1, 5, 100, 3844, 9600}))
GRID = (1, 2, 3, 6, 9, 10, 15, 16, 23, 30, 31, 32, 40, 44, 45, 46, 50, 57, 62)          # windows per side: 1 x 1 up to 62 x 62


def test_mirror_matches_the_library_on_the_sweep(lib):
    bad, n = [], 0
    kpw_seen, window_seen = set(), set()

    def cmp(name, args, got, want):
        nonlocal n
        n += 1
        if got != want:
            bad.append((name, args, got, want))

    for B, N in itertools.product(BATCHES, SIZES):
        _, ktiles, ks, kpw, last = P.corr_plan(B, N)
        assert 1 <= last <= kpw and (ks - 1) * kpw + last == ktiles
        kpw_seen.add("one" if kpw == 1 else "even" if last == kpw else "uneven")
        for C in (16, 64):
            cmp("corr ws", (B, C, N), lib.ipsr_corr_argmax_workspace_bytes(B, C, N), P.corr_ws(B, C, N))
            cmp("corr bf16 ws", (B, C, N), lib.ipsr_corr_argmax_bf16_workspace_bytes(B, C, N), P.corr_bf16_ws(B, C, N))
    for B, nH, nW, p, (C, M) in itertools.product((1, 2, 8, 32), GRID, GRID, (1, 2, 3), ((8, 0), (64, 16), (20, 40))):
        h, w = nH + p - 1, nW + p - 1
        if M > nH * nW:
            continue
        if p > 1:
            launched, kper, non_empty, last = P.window_plan(B, nH * nW)
            # no slice is ever empty: ceil(N' / kper) pieces of kper windows all start below N'
            assert non_empty == launched and 1 <= last <= kper and (launched - 1) * kper + last == nH * nW
            sought = P.window_split_sought(B, nH * nW)
            assert launched <= sought
            window_seen.add("all sought" if launched == sought else "trimmed")
        a = (B, C, h, w, M, p, 1)
        cmp("forward ws", a, lib.ipsr_forward_workspace_bytes(*a), P.forward_ws(B, C, h, w, M, p, False))
        cmp("forward bf16corr ws", a, lib.ipsr_forward_bf16corr_workspace_bytes(*a), P.forward_ws(B, C, h, w, M, p, True))
    print("%d queries, %d mismatches" % (n, len(bad)))
    assert n > 25000, n
    assert not bad, (len(bad), bad[:8])
    assert kpw_seen == {"one", "even", "uneven"}, kpw_seen
    # the issue expected a second outcome "one slice empty"; `window_plan` recomputes its count as ceil(N' / kper), so the two
    # outcomes that exist are "every slice sought is launched" and "fewer launched than sought", and an empty slice never occurs
    assert window_seen == {"all sought", "trimmed"}, window_seen


def test_the_window_split_between_1985_and_2016_windows_is_63_slices(lib):
    """Where the doubling loop stops at 64 slices of kper 32 but only 63 start below N' (B = 1): the library's WS_RU slice is sized for
    63, so the 64th, empty slice is not launched.  Pinned at both ends of the range and beside it."""
    for (nH, nW), sought, kper, launched in (((31, 64), 32, 62, 32), ((5, 397), 64, 32, 63), ((40, 50), 64, 32, 63), ((42, 48), 64, 32, 63),
                                             ((1, 2017), 64, 32, 64), ((32, 64), 64, 32, 64)):
        Np = nH * nW
        assert P.window_split_sought(1, Np) == sought and P.window_plan(1, Np)[:3] == (launched, kper, launched), (Np, P.window_plan(1, Np))
        a = (1, 8, nH + 2, nW + 2, 16, 3, 1)
        assert lib.ipsr_forward_workspace_bytes(*a) == P.forward_ws(1, 8, nH + 2, nW + 2, 16, 3, False), Np
        # (a 64th slice would add 2 x 4 N' bytes of partials, a multiple of 256 or not: the two counts cannot coincide)
        assert P.align_up((launched + 1) * Np * 4, 256) > P.align_up(launched * Np * 4, 256)


def test_mirror_matches_the_library_on_every_case_shape(lib):
    for cid, case in P.CORR_CASES.items():
        B, C, N = case[0]
        assert lib.ipsr_corr_argmax_workspace_bytes(B, C, N) == P.case_plan(cid)["ws"], cid
        assert P.case_plan(cid)["ws"] == 2 * P.align_up(B * case[5][0] * N * 4, 256) + 256, cid
    for cid, ((B, C, N), _) in P.BF16_CASES.items():
        assert lib.ipsr_corr_argmax_bf16_workspace_bytes(B, C, N) == P.case_plan(cid)["ws"], cid
    for cid, ((B, C, h, w), _, _) in P.LAYER_CASES.items():
        assert lib.ipsr_forward_workspace_bytes(B, C, h, w, 16, 1, 1) == P.forward_ws(B, C, h, w, 16, 1, False), cid
    for cid, ((B, C, h, w, p), _, _, bf16) in P.WINDOW_CASES.items():
        q = lib.ipsr_forward_bf16corr_workspace_bytes if bf16 else lib.ipsr_forward_workspace_bytes
        for M in (0, 9, 16):
            assert q(B, C, h, w, M, p, 1) == P.forward_ws(B, C, h, w, M, p, bf16), (cid, M)


@pytest.mark.parametrize("cid", P.ALL_CASE_IDS)
def test_every_gpu_case_reaches_the_path_written_beside_it(cid):
    P.check_case(cid)


@pytest.mark.parametrize("row", range(len(P.REACHABLE)), ids=lambda i: "row%02d" % i)
def test_every_reachable_instantiation_is_claimed_by_its_cases(row):
    variant, lines, cases = P.REACHABLE[row]
    assert cases, variant
    for cid in cases:
        assert variant in P.case_plan(cid)["kernels"], "%s: case %s launches %s" % (variant, cid, sorted(P.case_plan(cid)["kernels"]))


@pytest.mark.parametrize("row", range(len(P.EDGES)), ids=lambda i: "row%02d" % i)
def test_every_plan_row_of_the_variant_table_is_produced_by_its_cases(row):
    variant, lines, pred, cases = P.EDGES[row]
    assert cases, variant
    for cid in cases:
        assert pred(P.case_plan(cid)), "%s: case %s reaches %s" % (variant, cid, P.case_plan(cid))


def test_the_tables_reach_every_variant_and_edge():
    """The coverage claims, from the plans alone: every instantiation of corr_argmax.hip is launched by a case (none is left that
    no call can select); (kt_per_wg 1 | >= 2 with an even | uneven last split) x (fast | generic); the fast
    kernel below, at and past its ring; both outcomes of the window plan; every path of the two InnerCos kernels."""
    launched = set().union(*(P.case_plan(c)["kernels"] for c in P.ALL_CASE_IDS))
    assert launched == {v for v, _, _ in P.REACHABLE}
    assert not P.UNREACHABLE
    combos = set()
    for cid in list(P.CORR_CASES) + list(P.LAYER_CASES):
        p = P.case_plan(cid)
        ks, kpw, last = p["split"]
        combos.add((p["kind"], "one" if kpw == 1 else "even" if last == kpw else "uneven"))
    assert combos == set(itertools.product(("fast", "generic"), ("one", "even", "uneven")))     # (kt_per_wg 1 has no uneven split)
    assert {P.case_plan(c)["stages"] for c in P.FAST_STAGES} == {1, 2, 3, 5}
    assert {kind for kind, S in ((P.case_plan(c)["kind"], P.case_plan(c)["want_S"]) for c in P.CORR_CASES) if S} == {"fast", "generic"}
    wins = [P.case_plan(c) for c in P.WINDOW_CASES]
    assert any(p["window"][0] == p["sought"] > 1 for p in wins) and any(p["window"][0] < p["sought"] for p in wins)
    assert all(p["window"][2] == p["window"][0] for p in wins)
    assert {p["corr_kind"] for p in wins} == {"fast", "generic", "bf16"}
    ics = [P.case_plan(c) for c in P.IC_CASES]
    assert {p["vector"] for p in ics} == {False, True}
    assert {(p["vector"], p["rpb"], p["last"]) for p in ics} >= {(False, 2, 1), (True, 2, 1)}
    assert any(p["bwd_strides"] for p in ics) and any(p["cx_wider"] for p in ics) and any(p["fused_rpb"] > 1 for p in ics)
    ips = [P.case_plan(c) for c in P.INDEX_PREP_CASES]
    assert {p["chunks"] for p in ips} == {1, 2} and {p["args"][1] for p in ips} == {1, 2} and {p["args"][0] for p in ips} == {1, 2, 3, 4}


def test_the_variant_table_in_the_gpu_module_names_every_row_and_case():
    """The docstring table of tests/test_gpu_corr_variants.py is `corr_plan.variant_table()`: every line of it appears."""
    import os
    src = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "test_gpu_corr_variants.py")).read()
    doc = src.split('"""')[1]
    for line in P.variant_table().split("\n"):
        assert line.rstrip() in doc, line
