"""The split-bf16 weight gradient of the dilated layer Conv2d(k4, stride 2, pad 3, dilation 2) on fp32 tensors
(ipsr_conv4x4s2_bf16x3_dil_wrw, ops.conv4x4s2_bf16x3_dil_wrw, engine "bf16x3w" under `hipconv.set_direct_dilated_dw(True)`) without a GPU:
header, exports and binding table, the workspace query against the restated plan, the refusals that come before any HIP call, and the
dispatcher's opt-in rule.  Nothing here launches a kernel; the calls on fake addresses run in a child process with every GPU hidden, as in
tests/test_bf16x3_s2_wrw_abi.py.
"""
import os
import re

import pytest

import bf16x3_dil_wrw_plan as X
from bf16x3_harness import ROOT, fake_pointers, hipconv, lib, refused_calls  # noqa: F401  (fixtures by name)

IPSR_ERR_INVALID, IPSR_ERR_UNSUPPORTED, IPSR_ERR_WORKSPACE = -1, -2, -3
ENTRIES = ("ipsr_conv4x4s2_bf16x3_dil_wrw_workspace_bytes", "ipsr_conv4x4s2_bf16x3_dil_wrw")
WHO = "split-bf16 dilated 4x4 stride-2 weight gradient"
DIL, K4S1 = (4, 2, 3, 2), (4, 1, 1, 1)
# (channels, H = W of the module's input) of netG's four dilated down convolutions, and what select_wrw answers for each at batch 8 today
STEP = {(64, 256): "miopen", (128, 128): "wino_dil", (256, 64): "wino_dil", (512, 32): "wino_dil"}
# the rows the switch moves: every "wino_dil" row, and MIOpen's 64 -> 64 @256 (profiles/direct_bf16x3_dil_wrw_layers.txt)
MOVED = [(64, 256), (128, 128), (256, 64), (512, 32)]


@pytest.fixture
def switch(hipconv):
    assert hipconv.direct_dilated_dw() is False and hipconv.direct_dilated() is False
    yield hipconv
    hipconv.set_direct_dilated_dw(False)
    hipconv.set_direct_dilated(False)


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
        assert lib.ipsr_conv4x4s2_bf16x3_dil_wrw_workspace_bytes(*shape) == X.plan(*shape)["ws"] > 0, cid
    for row in X.STEP_ROWS:
        assert lib.ipsr_conv4x4s2_bf16x3_dil_wrw_workspace_bytes(8, *row) == X.plan(8, *row)["ws"] > 0, row
    refused = 0
    for B in range(1, 6):
        for Kc in (1, 127, 128, 129, 340):
            for Cf in (1, 31, 32, 33, 380):
                for nw in (8, 16, 24, 32, 64, 128, 256):
                    rs = max(1, 64 // nw)
                    for nh in (rs, 3 * rs, 3 * rs + 1, 4 * rs, 16):
                        p = X.plan(B, Kc, Cf, nh, nw)
                        got = lib.ipsr_conv4x4s2_bf16x3_dil_wrw_workspace_bytes(B, Kc, Cf, nh, nw)
                        assert got == (p["ws"] if p else 0), (B, Kc, Cf, nh, nw, got)
                        if p is None:
                            refused += 1
                            assert lib.ipsr_last_error().decode("utf-8", "replace").startswith(WHO), (B, Kc, Cf, nh, nw)
    assert refused


def test_the_k4_s2_p1_kernel_still_refuses_the_128_wide_grid(lib):
    assert lib.ipsr_conv4x4s2_bf16x3_wrw_workspace_bytes(1, 32, 64, 2, 128) == 0
    assert lib.ipsr_conv4x4s2_bf16x3_dil_wrw_workspace_bytes(1, 32, 64, 2, 128) > 0


@pytest.mark.parametrize("shape,msg", [((1, 16, 16, 4, 24), "coarse width 24"), ((1, 16, 16, 8, 8), "coarse width 8"), ((1, 16, 16, 1, 256), "coarse width 256"),
                                       ((1, 16, 16, 6, 16), "6 coarse rows are not a multiple of the 4 rows of a stage"),
                                       ((2, 16, 16, 3, 32), "3 coarse rows are not a multiple of the 2 rows of a stage"),
                                       ((0, 16, 16, 4, 16), "bad argument"), ((1, 16, 0, 4, 16), "bad argument")],
                         ids=["w24", "w8", "w256", "rows16", "rows32", "b0", "cf0"])
def test_workspace_query_refuses_with_a_message(lib, shape, msg):
    assert X.plan(*shape) is None
    assert lib.ipsr_conv4x4s2_bf16x3_dil_wrw_workspace_bytes(*shape) == 0
    assert msg in lib.ipsr_last_error().decode("utf-8", "replace")


@pytest.fixture(scope="module")
def refusals(lib):
    good = (2, 48, 16, 8, 16)
    need = lib.ipsr_conv4x4s2_bf16x3_dil_wrw_workspace_bytes(*good)
    assert need > 1
    big = 1 << 30
    # name: (shape, (fine, coarse, dw, ws) offsets or None for a null pointer, workspace bytes)
    calls = {"w24": ((1, 16, 16, 4, 24), (0, 0, 0, 0), big), "w8": ((1, 16, 16, 8, 8), (0, 0, 0, 0), big), "w256": ((1, 16, 16, 1, 256), (0, 0, 0, 0), big),
             "rows": ((1, 16, 16, 6, 16), (0, 0, 0, 0), big), "b0": ((0, 48, 16, 8, 16), (0, 0, 0, 0), big),
             "null_fine": (good, (None, 0, 0, 0), big), "null_coarse": (good, (0, None, 0, 0), big), "null_dw": (good, (0, 0, None, 0), big),
             "null_ws": (good, (0, 0, 0, None), big), "fine+8": (good, (8, 0, 0, 0), big), "coarse+8": (good, (0, 8, 0, 0), big),
             "dw+8": (good, (0, 0, 8, 0), big), "ws+4": (good, (0, 0, 0, 4), big), "ws_short": (good, (0, 0, 0, 0), need - 1)}
    table = {}
    for name, (shape, off, nbytes) in calls.items():
        ptr = fake_pointers(off)
        table[name] = ("ipsr_conv4x4s2_bf16x3_dil_wrw", (ptr[0], ptr[1], ptr[2], *shape, ptr[3], nbytes, None))
    return refused_calls(table)


@pytest.mark.parametrize("case,rc,msg", [("w24", IPSR_ERR_UNSUPPORTED, "coarse width 24"), ("w8", IPSR_ERR_UNSUPPORTED, "coarse width 8"),
                                         ("w256", IPSR_ERR_UNSUPPORTED, "coarse width 256"),
                                         ("rows", IPSR_ERR_UNSUPPORTED, "6 coarse rows are not a multiple"), ("b0", IPSR_ERR_INVALID, "bad argument"),
                                         ("null_fine", IPSR_ERR_INVALID, "null pointer"), ("null_coarse", IPSR_ERR_INVALID, "null pointer"),
                                         ("null_dw", IPSR_ERR_INVALID, "null pointer"), ("null_ws", IPSR_ERR_INVALID, "null pointer"),
                                         ("fine+8", IPSR_ERR_INVALID, "align"), ("coarse+8", IPSR_ERR_INVALID, "align"), ("dw+8", IPSR_ERR_INVALID, "align"),
                                         ("ws+4", IPSR_ERR_INVALID, "align"), ("ws_short", IPSR_ERR_WORKSPACE, "workspace")])
def test_refused_before_any_hip_call(refusals, case, rc, msg):
    got, text = refusals[case]
    assert got == rc and msg in text, (got, text)


def test_the_data_entry_keeps_refusing_the_weight_gradient_modes(lib):
    from deepinpainting_amd import ops
    for mode in (2, 3, 6):
        assert lib.ipsr_conv4x4s2_bf16x3_workspace_bytes(mode, 2, 48, 16, 16, 16) == 0
        assert not ops.conv4x4s2_bf16x3_supported(mode, 2, 48, 16, 16, 16)


def test_ops_supported(lib):
    from deepinpainting_amd import ops
    for row in X.STEP_ROWS:
        assert ops.conv4x4s2_bf16x3_dil_wrw_supported(8, *row), row
    assert not ops.conv4x4s2_bf16x3_dil_wrw_supported(1, 16, 16, 4, 24)
    assert not ops.conv4x4s2_bf16x3_dil_wrw_supported(1, 16, 16, 6, 16)


def _probes(hc):
    from deepinpainting_amd import ops
    sel, wrw = hc.select, hc.select_wrw
    p = {}
    for C, H in list(STEP) + [(512, 16), (64, 128), (64, 64)]:
        p["wrw_%d@%d" % (C, H)] = lambda C=C, H=H: wrw(False, 8, C, H, H, C, *DIL)
        p["wrw_bf16_%d@%d" % (C, H)] = lambda C=C, H=H: wrw(False, 8, C, H, H, C, *DIL, True)
        p["fwd_%d@%d" % (C, H)] = lambda C=C, H=H: sel(ops.CONV_FWD, 8, C, H, H, C, *DIL)
        p["dx_%d@%d" % (C, H)] = lambda C=C, H=H: sel(ops.CONV_BWD_DATA, 8, C, H, H, C, *DIL)
    p["wrw_64->128@256"] = lambda: wrw(False, 8, 64, 256, 256, 128, *DIL)      # MIOpen's, and not the one row of MIOpen's that moves
    p["k4s1_wrw"] = lambda: wrw(False, 8, 256, 32, 32, 512, *K4S1)
    p["k3_wrw"] = lambda: wrw(False, 8, 128, 128, 128, 128, 3, 1, 1, 1)
    p["s2_wrw"] = lambda: wrw(False, 8, 64, 128, 128, 128, 4, 2, 1, 1)
    p["s2T_wrw"] = lambda: wrw(True, 8, 128, 64, 64, 128, 4, 2, 1, 1)
    p["smallmap_wrw"] = lambda: wrw(False, 8, 512, 8, 8, 512, 4, 2, 1, 1)
    p["one_wrw"] = lambda: wrw(False, 8, 512, 31, 31, 1, *K4S1)
    return p


@pytest.mark.parametrize("math", ["fp32", "direct_bf16x3_s2_dw"])
def test_selection_is_opt_in(switch, math):
    from deepinpainting_amd import ops
    hc = switch
    hc.set_conv_math(fp32=math)
    probes = _probes(hc)
    moved = ["wrw_%d@%d" % row for row in MOVED]
    today = {k: f() for k, f in probes.items()}
    assert {row: today["wrw_%d@%d" % row] for row in STEP} == STEP, today
    assert today["k4s1_wrw"] == "wino_dil" and today["one_wrw"] == "one" and today["smallmap_wrw"] == "smallmap", today
    assert today["s2_wrw"] == ("bf16x3w" if math == "direct_bf16x3_s2_dw" else "wino_s2"), today
    # the switch on: the dilated weight gradients of the rule move, everything else answers as before
    hc.set_direct_dilated_dw(True)
    assert hc.direct_dilated_dw() is True and hc.direct_dilated() is False
    now = {k: f() for k, f in probes.items()}
    assert all(now[k] == "bf16x3w" for k in moved), now
    assert {k: v for k, v in now.items() if k not in moved} == {k: v for k, v in today.items() if k not in moved}
    assert hc._MATH == {"fp32": math, "bf16": "bf16x3"}            # independent of set_conv_math
    # independent of the data switch: each moves its own passes
    hc.set_direct_dilated(True)
    both = {k: f() for k, f in probes.items()}
    assert all(both[k] == "bf16x3w" for k in moved) and both["fwd_128@128"] == both["dx_128@128"] == "bf16x3d", both
    hc.set_direct_dilated(False)
    # a forced engine is not overridden
    for force in ("winograd", "miopen", "direct"):
        hc._FORCE = force
        assert all(hc.select_wrw(False, 8, C, H, H, C, *DIL) == "miopen" for C, H in MOVED), force
        hc._FORCE = None
    os.environ["IPSR_CONV_ENGINE"] = "miopen"
    try:
        hc.reload_env()
        assert all(hc.select_wrw(False, 8, C, H, H, C, *DIL) == "miopen" for C, H in MOVED)
    finally:
        del os.environ["IPSR_CONV_ENGINE"]
        hc.reload_env()
    assert probes[moved[-1]]() == "bf16x3w"
    # off again: every answer of today
    hc.set_direct_dilated_dw(False)
    assert {k: f() for k, f in probes.items()} == today
    assert len(ops.DIRECT_PASSES) == 4 and "direct_dilated_dw" not in ops.MATH_CODE


def test_flipping_the_switch_invalidates_the_memo(switch):
    hc = switch
    ask = lambda: hc.select_wrw(False, 8, 128, 128, 128, 128, *DIL)
    assert ask() == "wino_dil" and hc._SEL
    hc.set_direct_dilated_dw(True)
    assert not hc._SEL
    assert ask() == "bf16x3w" and hc._SEL
    hc.set_direct_dilated_dw(False)
    assert not hc._SEL and ask() == "wino_dil"


def test_the_engine_dispatches_on_the_geometry(hipconv, monkeypatch):
    from deepinpainting_amd import ops
    calls = []
    monkeypatch.setattr(ops, "conv4x4s2_bf16x3_wrw", lambda *a, **k: calls.append(("s2", a, k)))
    monkeypatch.setattr(ops, "conv4x4s2_bf16x3_dil_wrw", lambda *a, **k: calls.append(("dil", a, k)))
    run = hipconv._ENGINES["bf16x3w"].wrw
    run("x", "dy", (False, 8, 64, 32, 32, 128, 4, 2, 1, 1), "fp32", "sink")
    run("x", "dy", (False, 8, 64, 32, 32, 128, 4, 2, 3, 2), "fp32", "sink")
    run("x", "dy", (False, 2, 128, 256, 256, 128, 4, 2, 3, 2), "fp32", None)
    assert calls == [("s2", ("x", "dy", 8, 128, 64, 16, 16), {"out": "sink"}),
                     ("dil", ("x", "dy", 8, 128, 64, 16, 16), {"out": "sink"}),         # (fine, coarse) = (x, dy)
                     ("dil", ("x", "dy", 2, 128, 128, 128, 128), {"out": None})]


def test_the_trainer_reads_the_option():
    src = open(os.path.join(ROOT, "deepinpainting_amd", "models", "IPSR.py")).read()
    assert "set_direct_dilated_dw(bool(getattr(opt, 'direct_dilated_dw', False)))" in src
