"""The split-bf16 weight gradient of the k4 s2 p1 layers on fp32 tensors (ipsr_conv4x4s2_bf16x3_wrw, ops.conv4x4s2_bf16x3_wrw, engine
"bf16x3w" under `set_conv_math(fp32="direct_bf16x3_s2_dw")`) without a GPU: header, exports and binding table, the workspace query against
the restated plan, the refusals that come before any HIP call, and the dispatcher's opt-in rule.  Nothing here launches a kernel; the
calls on fake addresses run in a child process with every GPU hidden, as in tests/test_bf16x3_s2_abi.py.
"""
import os
import re

import pytest

import bf16x3_s2_wrw_plan as X
from bf16x3_harness import ROOT, fake_pointers, hipconv, lib, refused_calls  # noqa: F401  (fixtures by name)

IPSR_ERR_INVALID, IPSR_ERR_UNSUPPORTED, IPSR_ERR_WORKSPACE = -1, -2, -3
ENTRIES = ("ipsr_conv4x4s2_bf16x3_wrw_workspace_bytes", "ipsr_conv4x4s2_bf16x3_wrw")
# every k4 s2 p1 layer of the step at batch 8 as (transposed, Cin, H, Cout) of the module, and what select_wrw answered for it on the parent
# commit under "fp32", "direct_bf16x3", "direct_bf16x3_dw" and "direct_bf16x3_s2" alike
STEP_ROWS = {
    (False, 64, 128, 128): "wino_s2", (False, 128, 64, 256): "wino_s2", (False, 256, 32, 512): "wino_s2", (False, 512, 16, 512): "miopen",
    (False, 512, 8, 512): "smallmap", (True, 64, 128, 64): "miopen", (True, 128, 64, 128): "wino_s2", (True, 256, 32, 256): "wino_s2",
    (True, 512, 16, 512): "wino_s2", (True, 256, 64, 64): "wino_s2", (True, 512, 32, 128): "wino_s2", (True, 1024, 16, 256): "wino_s2",
    (True, 1024, 8, 512): "miopen", (True, 512, 8, 512): "miopen", (False, 3, 256, 64): "thin_mfma", (True, 128, 128, 3): "thin_mfma",
}
# the rows of the rule (profiles/direct_bf16x3_s2_wrw_layers.txt)
RULE_ROWS = [k for k, v in STEP_ROWS.items() if v == "wino_s2"]


def test_the_cases_reach_their_variants():
    X.check_cases()


def test_header_exports_and_bindings_carry_both_entries(lib):
    from deepinpainting_amd import _lib
    header = open(os.path.join(ROOT, "include", "ipsr_hip.h")).read()
    for name in ENTRIES:
        assert re.search(r"\b%s\(" % name, header), name
        assert name in _lib.SIGNATURES and getattr(lib, name).argtypes == _lib.SIGNATURES[name][1]
    assert lib.ipsr_abi_version() == 15


def test_workspace_query_equals_the_plan(lib):
    for cid, (shape, _) in X.CASES.items():
        assert lib.ipsr_conv4x4s2_bf16x3_wrw_workspace_bytes(*shape) == X.plan(*shape)["ws"] > 0, cid
    refused = 0
    for B in range(1, 6):
        for Kc in (1, 127, 128, 129, 340):
            for Cf in (1, 31, 32, 33, 380):
                for nw in (8, 16, 24, 32, 64, 128, 256):
                    rs = max(1, 64 // nw)
                    for nh in (rs, 3 * rs, 3 * rs + 1, 4 * rs, 16):
                        p = X.plan(B, Kc, Cf, nh, nw)
                        got = lib.ipsr_conv4x4s2_bf16x3_wrw_workspace_bytes(B, Kc, Cf, nh, nw)
                        assert got == (p["ws"] if p else 0), (B, Kc, Cf, nh, nw, got)
                        if p is None:
                            refused += 1
                            assert lib.ipsr_last_error().decode("utf-8", "replace").startswith("split-bf16 4x4 stride-2 weight gradient"), (B, Kc, Cf, nh, nw)
    assert refused


@pytest.mark.parametrize("shape,msg", [((1, 16, 16, 4, 24), "coarse width 24"), ((1, 16, 16, 8, 8), "coarse width 8"), ((1, 16, 16, 1, 256), "coarse width 256"),
                                       ((1, 32, 64, 2, 128), "coarse width 128"), ((1, 16, 16, 6, 16), "6 coarse rows are not a multiple of the 4 rows of a stage"),
                                       ((2, 16, 16, 3, 32), "3 coarse rows are not a multiple of the 2 rows of a stage"),
                                       ((0, 16, 16, 4, 16), "bad argument"), ((1, 16, 0, 4, 16), "bad argument")],
                         ids=["w24", "w8", "w256", "w128", "rows16", "rows32", "b0", "cf0"])
def test_workspace_query_refuses_with_a_message(lib, shape, msg):
    assert X.plan(*shape) is None
    assert lib.ipsr_conv4x4s2_bf16x3_wrw_workspace_bytes(*shape) == 0
    assert msg in lib.ipsr_last_error().decode("utf-8", "replace")


@pytest.fixture(scope="module")
def refusals(lib):
    good = (2, 48, 16, 8, 16)
    need = lib.ipsr_conv4x4s2_bf16x3_wrw_workspace_bytes(*good)
    # name: (shape, (fine, coarse, dw, ws) offsets or None for a null pointer, workspace bytes)
    calls = {"w24": ((1, 16, 16, 4, 24), (0, 0, 0, 0), 1 << 30), "w128": ((1, 32, 64, 2, 128), (0, 0, 0, 0), 1 << 30), "rows": ((1, 16, 16, 6, 16), (0, 0, 0, 0), 1 << 30),
             "b0": ((0, 48, 16, 8, 16), (0, 0, 0, 0), 1 << 30), "null_fine": (good, (None, 0, 0, 0), 1 << 30), "null_dw": (good, (0, 0, None, 0), 1 << 30),
             "null_ws": (good, (0, 0, 0, None), 1 << 30), "fine+8": (good, (8, 0, 0, 0), 1 << 30), "coarse+4": (good, (0, 4, 0, 0), 1 << 30),
             "dw+8": (good, (0, 0, 8, 0), 1 << 30), "ws+4": (good, (0, 0, 0, 4), 1 << 30), "ws_short": (good, (0, 0, 0, 0), need - 1)}
    table = {}
    for name, (shape, off, nbytes) in calls.items():
        ptr = fake_pointers(off)
        table[name] = ("ipsr_conv4x4s2_bf16x3_wrw", (ptr[0], ptr[1], ptr[2], *shape, ptr[3], nbytes, None))
    return refused_calls(table)


@pytest.mark.parametrize("case,rc,msg", [("w24", IPSR_ERR_UNSUPPORTED, "coarse width 24"), ("w128", IPSR_ERR_UNSUPPORTED, "coarse width 128"),
                                         ("rows", IPSR_ERR_UNSUPPORTED, "6 coarse rows are not a multiple"), ("b0", IPSR_ERR_INVALID, "bad argument"),
                                         ("null_fine", IPSR_ERR_INVALID, "null pointer"), ("null_dw", IPSR_ERR_INVALID, "null pointer"),
                                         ("null_ws", IPSR_ERR_INVALID, "null pointer"), ("fine+8", IPSR_ERR_INVALID, "align"),
                                         ("coarse+4", IPSR_ERR_INVALID, "align"), ("dw+8", IPSR_ERR_INVALID, "align"), ("ws+4", IPSR_ERR_INVALID, "align"),
                                         ("ws_short", IPSR_ERR_WORKSPACE, "workspace")])
def test_refused_before_any_hip_call(refusals, case, rc, msg):
    got, text = refusals[case]
    assert got == rc and msg in text, (got, text)


def _wrw(hc, row, B=8):
    tr, Cin, H, Cout = row
    return hc.select_wrw(tr, B, Cin, H, H, Cout, 4, 2, 1, 1)


def test_the_older_names_select_what_they_did(hipconv):
    """The answers of the parent commit, recorded in STEP_ROWS."""
    for name in ("fp32", "direct_bf16x3", "direct_bf16x3_dw", "direct_bf16x3_s2"):
        hipconv.set_conv_math(fp32=name)
        assert {row: _wrw(hipconv, row) for row in STEP_ROWS} == STEP_ROWS, name


def test_selection_is_opt_in(hipconv):
    from deepinpainting_amd import ops
    sel, wrw = hipconv.select, hipconv.select_wrw
    k3, k4 = (3, 1, 1, 1), (4, 2, 1, 1)
    others = {
        "k3_fwd": lambda: sel(ops.CONV_FWD, 8, 128, 128, 128, 128, *k3),
        "k3_wrw": lambda: wrw(False, 8, 128, 128, 128, 128, *k3),
        "k3_wrw_512_32": lambda: wrw(False, 8, 512, 32, 32, 512, *k3),
        "s2_fwd": lambda: sel(ops.CONV_FWD, 8, 64, 128, 128, 128, *k4),
        "s2T_dx_128": lambda: sel(ops.CONVT_BWD_DATA, 8, 64, 128, 128, 64, *k4),
        "s2_fwd_8": lambda: sel(ops.CONV_FWD, 8, 512, 16, 16, 512, *k4),
        "dil_wrw": lambda: wrw(False, 8, 128, 64, 64, 128, 4, 2, 3, 2),
        "k4s1_wrw": lambda: wrw(False, 8, 256, 32, 32, 512, 4, 1, 1, 1),
        "one_wrw": lambda: wrw(False, 8, 512, 31, 31, 1, 4, 1, 1, 1),
        "s2_wrw_bf16": lambda: wrw(False, 8, 64, 128, 128, 128, *k4, True),
    }
    hipconv.set_conv_math(fp32="direct_bf16x3_s2")
    before = {k: f() for k, f in others.items()}
    assert before["dil_wrw"] == before["k4s1_wrw"] == "wino_dil" and before["one_wrw"] == "one", before
    hipconv.set_conv_math(fp32="direct_bf16x3_s2_dw")
    now = {row: _wrw(hipconv, row) for row in STEP_ROWS}
    assert RULE_ROWS and all(now[row] == "bf16x3w" for row in RULE_ROWS), now
    # 8x8 grids and below, the 3-channel ends, MIOpen's 64 -> 64 on the 128-wide coarse grid: today's engine
    assert {row: e for row, e in now.items() if row not in RULE_ROWS} == {row: e for row, e in STEP_ROWS.items() if row not in RULE_ROWS}
    # everything "direct_bf16x3_s2" does still holds; the dilated family, k4 s1, the one-channel head and bf16 activations stay
    assert {k: f() for k, f in others.items()} == before
    # a forced engine is not overridden
    for force in ("winograd", "miopen", "direct"):
        hipconv._FORCE = force
        assert all(_wrw(hipconv, row) == "miopen" for row in RULE_ROWS), force
        hipconv._FORCE = None
    os.environ["IPSR_CONV_ENGINE"] = "miopen"
    try:
        hipconv.reload_env()
        assert all(_wrw(hipconv, row) == "miopen" for row in RULE_ROWS)
    finally:
        del os.environ["IPSR_CONV_ENGINE"]
        hipconv.reload_env()
    assert _wrw(hipconv, RULE_ROWS[0]) == "bf16x3w"
    hipconv.set_conv_math(fp32="fp32")
    assert {row: _wrw(hipconv, row) for row in STEP_ROWS} == STEP_ROWS
    assert ops.MATH_CODE["direct_bf16x3_s2_dw"] == ops.MATH_CODE["fp32"] == 0
    e = hipconv._ENGINES["bf16x3w"]
    assert e.data is None and e.wrw is not None and e.sink and not e.bf16_io and not e.fp32_copies


def test_the_engine_dispatches_on_the_kernel_size(hipconv, monkeypatch):
    from deepinpainting_amd import ops
    calls = []
    monkeypatch.setattr(ops, "conv3x3_bf16x3_wrw", lambda *a, **k: calls.append(("k3", a, k)))
    monkeypatch.setattr(ops, "conv4x4s2_bf16x3_wrw", lambda *a, **k: calls.append(("k4", a, k)))
    run = hipconv._ENGINES["bf16x3w"].wrw
    run("x", "dy", (False, 8, 64, 32, 32, 128, 3, 1, 1, 1), "fp32", "sink")
    run("x", "dy", (False, 8, 64, 32, 32, 128, 4, 2, 1, 1), "fp32", "sink")
    run("x", "dy", (True, 8, 128, 16, 16, 64, 4, 2, 1, 1), "fp32", None)
    assert calls == [("k3", (False, "x", "dy", 128), {"out": "sink"}),
                     ("k4", ("x", "dy", 8, 128, 64, 16, 16), {"out": "sink"}),          # Conv2d: (fine, coarse) = (x, dy)
                     ("k4", ("dy", "x", 8, 128, 64, 16, 16), {"out": None})]            # ConvTranspose2d: (dy, x)


def test_the_new_name_is_fp32_only(hipconv):
    with pytest.raises(ValueError):
        hipconv.set_conv_math(bf16="direct_bf16x3_s2_dw")
    assert hipconv._MATH == {"fp32": "fp32", "bf16": "bf16x3"}
