"""`ipsr_window_corr_plan` against its restatement (tests/window_stencil_plan.py), without a GPU: the query launches nothing.

Over h, w in {p .. 12, 31, 32, 33, 64, 96, 116, 117, 120}, p in {2, 3, 4}, B in {1, 3, 4, 8} and ipsr_debug_set_option(8, 0 | 1 | 2):
the variant, the workgroups, the k-row split and the LDS bytes are the restatement's; option 1 never leaves the streaming kernel; the
split never exceeds the slices `window_plan` sized the partials' workspace for; the forward's workspace does not depend on the option.
"""
import ctypes

import pytest

import corr_plan as P
import window_stencil_plan as W

OPTION = 8


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    from deepinpainting_amd import _lib
    L = _lib.lib()
    yield L
    L.ipsr_debug_set_option(OPTION, 0)


def query(L, B, h, w, p):
    out = (ctypes.c_int * 4)()
    rc = L.ipsr_window_corr_plan(B, h, w, p, ctypes.cast(out, ctypes.c_void_p))
    assert rc == 0, (rc, L.ipsr_last_error())
    return {"variant": out[0], "workgroups": out[1], "split": out[2], "lds_bytes": out[3]}


def sweep():
    for p in (2, 3, 4):
        for h in W.EXTENTS[p]:
            for w in W.EXTENTS[p]:
                for B in W.BATCHES:
                    yield B, h, w, p


@pytest.mark.parametrize("option", W.OPTIONS)
def test_plan_matches_the_restatement(lib, option):
    assert lib.ipsr_debug_set_option(OPTION, option) == 0
    try:
        tiled = 0
        for B, h, w, p in sweep():
            got, want = query(lib, B, h, w, p), W.plan(B, h, w, p, option)
            assert got == want, ((B, h, w, p), option, got, want)
            slices = P.window_plan(B, (h - p + 1) * (w - p + 1))[0]
            assert 1 <= got["split"] <= slices, ((B, h, w, p), got, slices)
            if option == 1:
                assert got["variant"] == W.STREAMING
            if got["variant"] == W.LDS_TILED:
                tiled += 1
                assert W.envelope(h, w, p) and got["lds_bytes"] <= W.LDS_LIMIT and got["workgroups"] == B * (h - p + 1) * got["split"]
            if option == 2:
                assert got["variant"] == (W.LDS_TILED if W.envelope(h, w, p) else W.STREAMING)
        assert (tiled == 0) == (option == 1)
    finally:
        lib.ipsr_debug_set_option(OPTION, 0)


def test_the_envelope_ends_where_the_blocks_outgrow_the_lds():
    assert W.envelope(116, 116, 3) and not W.envelope(117, 117, 3) and not W.envelope(4, 120, 3)
    assert W.envelope(96, 96, 4) and W.envelope(120, 120, 2) and not W.envelope(5, 5, 1)
    # h does not enter: the blocks are w x w
    assert W.envelope(120, 116, 3) and not W.envelope(116, 120, 3)


def test_the_gpu_cases_are_what_they_say():
    plans = {cid: W.plan(B, h, w, p, 2) for cid, (B, _, h, w, p) in W.GPU_CASES.items()}
    assert all(pl["variant"] == W.LDS_TILED for pl in plans.values())
    assert plans["many_per_thread_split"]["split"] > 1 and plans["one_range_no_merge"]["split"] == 1
    assert plans["one_window"]["workgroups"] == 1
    # both buffer modes run: one buffer of 3 * 70 * 70 + 70 floats, two of 3 * 33 * 33 + 33
    assert plans["wider_than_a_wave"]["lds_bytes"] == 4 * 14770 and plans["many_per_thread_split"]["lds_bytes"] == 8 * 3300
    B, _, h, w, p = W.FALLBACK_CASE
    assert W.plan(B, h, w, p, 2)["variant"] == W.STREAMING


def test_invalid_arguments_are_refused(lib):
    out = (ctypes.c_int * 4)()
    ptr = ctypes.cast(out, ctypes.c_void_p)
    for B, h, w, p, o in ((1, 8, 8, 0, ptr), (1, 2, 8, 3, ptr), (1, 8, 2, 3, ptr), (1, 8, 8, 3, None)):
        assert lib.ipsr_window_corr_plan(B, h, w, p, o) == -1, (B, h, w, p)
        assert b"ipsr_window_corr_plan" in lib.ipsr_last_error()
    assert lib.ipsr_window_corr_plan(1, 8, 8, 1, ptr) == 0 and out[0] == W.STREAMING       # shift_sz = 1 is valid and never tiled


def test_the_forward_workspace_does_not_follow_the_option(lib):
    sizes = {}
    try:
        for option in (1, 2):
            assert lib.ipsr_debug_set_option(OPTION, option) == 0
            sizes[option] = [(lib.ipsr_forward_workspace_bytes(B, 16, h, w, 4, p, 1), lib.ipsr_forward_bf16corr_workspace_bytes(B, 64, h, w, 4, p, 1))
                             for B, h, w, p in sweep()]
    finally:
        lib.ipsr_debug_set_option(OPTION, 0)
    assert sizes[1] == sizes[2] and all(a > 0 for a, _ in sizes[1])
    assert lib.ipsr_abi_version() == 15


def test_ops_wrapper_returns_the_query(lib):
    from deepinpainting_amd import ops
    assert ops.window_corr_plan(4, 64, 64, 3) == query(lib, 4, 64, 64, 3) == W.plan(4, 64, 64, 3, 0)
