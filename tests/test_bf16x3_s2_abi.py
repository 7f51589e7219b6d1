"""The split-bf16 direct kernel for the k4 s2 p1 layers on fp32 tensors (ipsr_conv4x4s2_bf16x3, ops.conv4x4s2_bf16x3, engine "bf16x3d"
under `set_conv_math(fp32="direct_bf16x3_s2")`) without a GPU: its workspace query against the restated plan, the refusals that come
before any HIP call, and the dispatcher's opt-in rule.  Nothing here launches a kernel; the calls on fake addresses run in a child process
with every GPU hidden, as in tests/test_bf16x3_abi.py.
"""
import os

import pytest

import bf16_conv_plan as P
import bf16x3_s2_plan as S
from bf16x3_harness import fake_pointers, hipconv, lib, refused_calls  # noqa: F401  (fixtures by name)

IPSR_ERR_INVALID, IPSR_ERR_UNSUPPORTED, IPSR_ERR_WORKSPACE = -1, -2, -3
# the k4 s2 p1 data rows of the step at batch 8 that "wino_s2" has today: (Kc, Cf, n)
STEP_ROWS = [(128, 64, 64), (256, 128, 32), (512, 256, 16), (128, 128, 64), (256, 256, 32), (512, 512, 16), (256, 64, 64), (512, 128, 32), (1024, 256, 16)]


def test_the_cases_reach_their_variants():
    S.check_cases()
    assert S.plan(0, *S.CASES["cut"][0])["nsplit"] == S.plan(1, *S.CASES["cut"][0])["nsplit"] == 2
    for cid in ("wrap", "tiles3"):
        assert all(S.plan(m, *S.CASES[cid][0])["tiles_per_img"] > 1 for m in (0, 1)), cid


def test_workspace_query_equals_the_plan(lib):
    for cid, (shape, _) in S.CASES.items():
        for mode in (0, 1):
            assert lib.ipsr_conv4x4s2_bf16x3_workspace_bytes(mode, *shape) == S.plan(mode, *shape)["ws"] > 0, (cid, mode)
    for Kc, Cf, n in STEP_ROWS + [(64, 64, 128)]:
        for mode in (0, 1):
            assert lib.ipsr_conv4x4s2_bf16x3_workspace_bytes(mode, 8, Kc, Cf, n, n) == S.plan(mode, 8, Kc, Cf, n, n)["ws"] > 0, (mode, Kc, Cf, n)


@pytest.mark.parametrize("shape,msg", [((0, 1, 16, 16, 12, 24), "coarse width 24"), ((1, 1, 16, 16, 12, 24), "coarse width 24"), ((0, 1, 16, 16, 8, 8), "coarse width 8"),
                                       ((1, 1, 16, 16, 1, 256), "coarse width 256"),
                                       ((0, 1, 16, 8, 16, 16), "8 reduction channels are not a multiple of 16"),
                                       ((1, 1, 8, 16, 16, 16), "8 reduction channels are not a multiple of 16"),
                                       ((0, 1, 16, 16, 12, 16), "12 rows are not a multiple of the 16 rows of a tile"),
                                       ((1, 2, 16, 16, 3, 128), "3 rows are not a multiple of the 2 rows of a tile"),
                                       ((2, 1, 16, 16, 16, 16), "bad argument"), ((0, 0, 16, 16, 16, 16), "bad argument")],
                         ids=["w24", "w24_c2f", "w8", "w256", "c8", "c8_c2f", "rows", "rows_c2f", "mode2", "b0"])
def test_workspace_query_refuses_with_a_message(lib, shape, msg):
    assert S.plan(*shape) is None
    assert lib.ipsr_conv4x4s2_bf16x3_workspace_bytes(*shape) == 0
    assert msg in lib.ipsr_last_error().decode("utf-8", "replace")


def test_the_bf16_query_answers_as_before(lib):
    for B in (1, 3, 8):
        for Kc, Cf in ((48, 16), (64, 64), (80, 80), (128, 64), (512, 256), (1024, 256)):
            for nh, nw in ((16, 16), (32, 16), (8, 32), (12, 64), (4, 128), (2, 128), (12, 24), (8, 8)):
                for mode in (0, 1):
                    assert lib.ipsr_conv4x4s2_bf16_workspace_bytes(mode, B, Kc, Cf, nh, nw) == P.s2_ws(mode, B, Kc, Cf, nh, nw), (mode, B, Kc, Cf, nh, nw)


@pytest.fixture(scope="module")
def refusals(lib):
    need = lib.ipsr_conv4x4s2_bf16x3_workspace_bytes(0, 2, 48, 16, 16, 16)
    good = (2, 48, 16, 16, 16)
    # name: (mode, shape, (in, weight, out, ws) offsets or None for a null pointer, workspace bytes)
    calls = {"w24": (0, (1, 16, 16, 12, 24), (0, 0, 0, 0), 1 << 30), "c8": (0, (1, 16, 8, 16, 16), (0, 0, 0, 0), 1 << 30),
             "rows": (1, (1, 16, 16, 12, 16), (0, 0, 0, 0), 1 << 30), "mode2": (2, good, (0, 0, 0, 0), 1 << 30), "mode-1": (-1, good, (0, 0, 0, 0), 1 << 30),
             "null_in": (0, good, (None, 0, 0, 0), 1 << 30), "null_ws": (1, good, (0, 0, 0, None), 1 << 30),
             "in+8": (0, good, (8, 0, 0, 0), 1 << 30), "out+8": (1, good, (0, 0, 8, 0), 1 << 30), "ws+4": (0, good, (0, 0, 0, 4), 1 << 30),
             "ws_short": (0, good, (0, 0, 0, 0), need - 1)}
    table = {}
    for name, (mode, shape, off, nbytes) in calls.items():
        ptr = fake_pointers(off)
        table[name] = ("ipsr_conv4x4s2_bf16x3", (mode, ptr[0], ptr[1], ptr[2], *shape, ptr[3], nbytes, None))
    return refused_calls(table)


@pytest.mark.parametrize("case,rc,msg", [("w24", IPSR_ERR_UNSUPPORTED, "coarse width 24"), ("c8", IPSR_ERR_UNSUPPORTED, "8 reduction channels"),
                                         ("rows", IPSR_ERR_UNSUPPORTED, "12 rows are not a multiple"), ("mode2", IPSR_ERR_INVALID, "mode 2"),
                                         ("mode-1", IPSR_ERR_INVALID, "mode -1"), ("null_in", IPSR_ERR_INVALID, "null pointer"),
                                         ("null_ws", IPSR_ERR_INVALID, "null pointer"), ("in+8", IPSR_ERR_INVALID, "align"),
                                         ("out+8", IPSR_ERR_INVALID, "align"), ("ws+4", IPSR_ERR_INVALID, "align"),
                                         ("ws_short", IPSR_ERR_WORKSPACE, "workspace")])
def test_refused_before_any_hip_call(refusals, case, rc, msg):
    got, text = refusals[case]
    assert got == rc and msg in text, (got, text)


def test_selection_is_opt_in(hipconv):
    from deepinpainting_amd import ops
    k3, k4 = (3, 1, 1, 1), (4, 2, 1, 1)
    sel, wrw = hipconv.select, hipconv.select_wrw
    probes = {
        "k3_fwd": lambda: sel(ops.CONV_FWD, 8, 128, 128, 128, 128, *k3),
        "k3_dx": lambda: sel(ops.CONV_BWD_DATA, 8, 128, 128, 128, 128, *k3),
        "k3_wrw": lambda: wrw(False, 8, 128, 128, 128, 128, *k3),
        "k3_wrw_512_32": lambda: wrw(False, 8, 512, 32, 32, 512, *k3),
        "k3_fwd_bf16": lambda: sel(ops.CONV_FWD, 8, 128, 128, 128, 128, *k3, True),
        "k3_thin": lambda: sel(ops.CONV_FWD, 8, 3, 256, 256, 64, *k3),
        # the step's "wino_s2" rows: Conv2d 64 -> 128 @128, 256 -> 512 @32; ConvTranspose2d 128 -> 128 @64, 1024 -> 256 @16, 64 -> 64 @128 (forward only)
        "s2_fwd": lambda: sel(ops.CONV_FWD, 8, 64, 128, 128, 128, *k4),
        "s2_dx": lambda: sel(ops.CONV_BWD_DATA, 8, 64, 128, 128, 128, *k4),
        "s2_fwd_16": lambda: sel(ops.CONV_FWD, 8, 256, 32, 32, 512, *k4),
        "s2T_fwd": lambda: sel(ops.CONVT_FWD, 8, 128, 64, 64, 128, *k4),
        "s2T_dx": lambda: sel(ops.CONVT_BWD_DATA, 8, 128, 64, 64, 128, *k4),
        "s2T_dx_16": lambda: sel(ops.CONVT_BWD_DATA, 8, 1024, 16, 16, 256, *k4),
        "s2T_fwd_128": lambda: sel(ops.CONVT_FWD, 8, 64, 128, 128, 64, *k4),
        "s2T_dx_128": lambda: sel(ops.CONVT_BWD_DATA, 8, 64, 128, 128, 64, *k4),             # MIOpen's today: the one row of its that moves
        # and what must stay: weight gradients, the 8x8 grids, the innermost levels, thin, dilated, k4 s1, bf16 activations, other MIOpen rows
        "s2_wrw": lambda: wrw(False, 8, 64, 128, 128, 128, *k4),
        "s2T_wrw": lambda: wrw(True, 8, 128, 64, 64, 128, *k4),
        "s2_fwd_8": lambda: sel(ops.CONV_FWD, 8, 512, 16, 16, 512, *k4),
        "s2T_fwd_8": lambda: sel(ops.CONVT_FWD, 8, 1024, 8, 8, 512, *k4),
        "s2_small": lambda: sel(ops.CONV_FWD, 8, 512, 4, 4, 512, *k4),
        "s2_thin": lambda: sel(ops.CONV_FWD, 8, 3, 256, 256, 64, *k4),
        "s2_dx_thin": lambda: sel(ops.CONV_BWD_DATA, 8, 3, 256, 256, 64, *k4),
        "s2T_fwd_thin": lambda: sel(ops.CONVT_FWD, 8, 128, 128, 128, 3, *k4),
        "s2_fwd_64_64": lambda: sel(ops.CONV_FWD, 8, 64, 128, 128, 64, *k4),                 # MIOpen's, 64 x 64 grid: not measured, stays
        "dil_fwd": lambda: sel(ops.CONV_FWD, 8, 128, 64, 64, 128, 4, 2, 3, 2),
        "k4s1_fwd": lambda: sel(ops.CONV_FWD, 8, 256, 32, 32, 512, 4, 1, 1, 1),
        "s2_fwd_bf16": lambda: sel(ops.CONV_FWD, 8, 64, 128, 128, 128, *k4, True),
        "s2T_fwd_bf16": lambda: sel(ops.CONVT_FWD, 8, 128, 64, 64, 128, *k4, True),
    }
    s2_moved = ("s2_fwd", "s2_dx", "s2_fwd_16", "s2T_fwd", "s2T_dx", "s2T_dx_16", "s2T_fwd_128", "s2T_dx_128")
    k3_moved = ("k3_fwd", "k3_dx", "k3_wrw")
    assert hipconv._MATH == {"fp32": "fp32", "bf16": "bf16x3"}
    today = {k: f() for k, f in probes.items()}
    assert all(today[k] == "wino_s2" for k in s2_moved[:-1]) and today["s2T_dx_128"] == "miopen", today
    assert today["s2_wrw"] == today["s2T_wrw"] == "wino_s2" and today["s2_small"] == "smallmap" and today["dil_fwd"] == today["k4s1_fwd"] == "wino_dil", today
    assert today["s2_fwd_8"] == today["s2T_fwd_8"] == today["s2_fwd_64_64"] == "miopen", today
    assert "bf16x3d" not in today.values() and "bf16x3w" not in today.values()
    # the four older names: nothing of the k4 family moves, the k3 probes answer as they did
    older = {}
    for name in ("fp32", "bf16x3", "direct_bf16x3", "direct_bf16x3_dw"):
        hipconv.set_conv_math(fp32=name)
        older[name] = {k: f() for k, f in probes.items()}
        assert {k: v for k, v in older[name].items() if k not in k3_moved} == {k: v for k, v in today.items() if k not in k3_moved}, name
    assert older["fp32"] == older["bf16x3"] == today
    assert older["direct_bf16x3"]["k3_fwd"] == "bf16x3d" and older["direct_bf16x3"]["k3_wrw"] == today["k3_wrw"]
    assert older["direct_bf16x3_dw"]["k3_fwd"] == older["direct_bf16x3_dw"]["k3_dx"] == "bf16x3d" and older["direct_bf16x3_dw"]["k3_wrw"] == "bf16x3w"
    # the new name: the k3 probes as under "direct_bf16x3_dw", the rule's k4 data rows on "bf16x3d", everything else as today
    hipconv.set_conv_math(fp32="direct_bf16x3_s2")
    now = {k: f() for k, f in probes.items()}
    assert all(now[k] == "bf16x3d" for k in s2_moved), now
    assert {k: v for k, v in now.items() if k not in s2_moved} == {k: v for k, v in older["direct_bf16x3_dw"].items() if k not in s2_moved}
    # a forced engine is not overridden
    for force in ("winograd", "miopen", "direct"):
        hipconv._FORCE = force
        assert sel(ops.CONV_FWD, 8, 64, 128, 128, 128, *k4) == hipconv._select(ops.CONV_FWD, (False, 8, 64, 128, 128, 128, *k4)) != "bf16x3d"
        assert sel(ops.CONVT_BWD_DATA, 8, 64, 128, 128, 64, *k4) != "bf16x3d"
        hipconv._FORCE = None
    os.environ["IPSR_CONV_ENGINE"] = "miopen"
    try:
        hipconv.reload_env()
        assert sel(ops.CONV_FWD, 8, 64, 128, 128, 128, *k4) == "miopen" and sel(ops.CONVT_BWD_DATA, 8, 64, 128, 128, 64, *k4) == "miopen"
    finally:
        del os.environ["IPSR_CONV_ENGINE"]
        hipconv.reload_env()
    assert probes["s2_fwd"]() == "bf16x3d"
    hipconv.set_conv_math(fp32="fp32")
    assert {k: f() for k, f in probes.items()} == today
    assert ops.MATH_CODE["direct_bf16x3_s2"] == ops.MATH_CODE["fp32"] == 0
    e = hipconv._ENGINES["bf16x3d"]
    assert e.data is not None and e.wrw is None and not e.bf16_io and not e.fp32_copies


def test_the_new_name_is_fp32_only(hipconv):
    with pytest.raises(ValueError):
        hipconv.set_conv_math(bf16="direct_bf16x3_s2")
    assert hipconv._MATH == {"fp32": "fp32", "bf16": "bf16x3"}
