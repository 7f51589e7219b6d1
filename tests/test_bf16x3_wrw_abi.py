"""The split-bf16 weight gradient on fp32 tensors (forms 2 / 3 of ipsr_conv3x3_bf16_wrw, ops.conv3x3_bf16x3_wrw, engine "bf16x3w")
without a GPU: its workspace query, the refusals that come before any HIP call, and the dispatcher's opt-in rule
(`set_conv_math(fp32="direct_bf16x3_dw")`).  Nothing here launches a kernel; the calls on fake addresses run in a child process with
every GPU hidden, as in tests/test_bf16x3_abi.py.
"""
import os

import pytest

import bf16_conv_plan as P
import bf16x3_wrw_plan as X
from bf16x3_harness import fake_pointers, hipconv, lib, refused_calls  # noqa: F401  (fixtures by name)

IPSR_ERR_INVALID = -1


def test_the_cases_reach_their_variants():
    X.check_cases()


def test_workspace_query_accepts_the_gpu_shapes(lib):
    for cid, ((tr, B, Cin, Cout, H, W), _) in X.CASES.items():
        assert lib.ipsr_conv3x3_bf16x3_wrw_workspace_bytes(tr, B, Cin, H, W, Cout) == X.plan(tr, B, Cin, H, W, Cout)["ws"] > 0, cid
    # the step's shapes at batch 8
    for tr, Cin, H, Cout in ((0, 128, 128, 128), (0, 256, 64, 256), (0, 512, 32, 512), (1, 512, 64, 128), (0, 512, 16, 512)):
        assert lib.ipsr_conv3x3_bf16x3_wrw_workspace_bytes(tr, 8, Cin, H, H, Cout) == X.plan(tr, 8, Cin, H, H, Cout)["ws"] > 0


@pytest.mark.parametrize("shape,msg", [((0, 1, 16, 12, 24, 16), "width 24"), ((1, 1, 16, 12, 24, 16), "width 24"), ((0, 1, 64, 4, 256, 64), "width 256"),
                                       ((0, 2, 16, 12, 16, 16), "12 rows are not a multiple of the 8 rows of a stage"),
                                       ((0, 0, 16, 16, 16, 16), "bad argument")],
                         ids=["w24", "w24T", "w256", "rows", "b0"])
def test_workspace_query_refuses_with_a_message(lib, shape, msg):
    assert X.plan(*shape) is None
    assert lib.ipsr_conv3x3_bf16x3_wrw_workspace_bytes(*shape) == 0
    assert msg in lib.ipsr_last_error().decode("utf-8", "replace")


def test_the_bf16_plan_is_untouched(lib):
    for cid, ((tr, B, Cin, Cout, H, W), _) in X.CASES.items():
        assert lib.ipsr_conv3x3_bf16_wrw_workspace_bytes(tr, B, Cin, H, W, Cout) == P.k3_wrw_ws(tr, B, Cin, H, W, Cout) > 0, cid


@pytest.fixture(scope="module")
def refusals(lib):
    calls = {}
    for name, form, off in (("x+8", 2, (8, 0, 0, 0)), ("dy+8", 3, (0, 8, 0, 0)), ("ws+8", 2, (0, 0, 0, 8)), ("form4", 4, (0, 0, 0, 0)), ("form-1", -1, (0, 0, 0, 0))):
        x, dy, dw, ws = fake_pointers(off, stride=1 << 24)
        calls[name] = ("ipsr_conv3x3_bf16_wrw", (form, x, dy, dw, 2, 32, 16, 16, 48, ws, 1 << 40, None))
    return refused_calls(calls)


@pytest.mark.parametrize("case", ["x+8", "dy+8", "ws+8", "form4", "form-1"])
def test_refused_before_any_hip_call(refusals, case):
    rc, msg = refusals[case]
    want = {"form4": "form code 4", "form-1": "form code -1"}.get(case, "align")
    assert rc == IPSR_ERR_INVALID and want in msg, (rc, msg)


def test_selection_is_opt_in(hipconv):
    from deepinpainting_amd import ops
    k3 = (3, 1, 1, 1)
    probes = {
        "fwd": lambda: hipconv.select(ops.CONV_FWD, 8, 128, 128, 128, 128, *k3),
        "dx": lambda: hipconv.select(ops.CONV_BWD_DATA, 8, 128, 128, 128, 128, *k3),
        "wrw_miopen": lambda: hipconv.select_wrw(False, 8, 128, 128, 128, 128, *k3),
        "wrw_wino": lambda: hipconv.select_wrw(False, 8, 256, 64, 64, 256, *k3),
        "wrw_32": lambda: hipconv.select_wrw(False, 8, 256, 32, 32, 256, *k3),
        "wrw_512_32": lambda: hipconv.select_wrw(False, 8, 512, 32, 32, 512, *k3),          # loses to the Winograd weight gradient: outside the rule
        "wrwT": lambda: hipconv.select_wrw(True, 8, 512, 64, 64, 128, *k3),
        "wrw_w256": lambda: hipconv.select_wrw(False, 8, 64, 256, 256, 64, *k3),             # a width the kernel refuses
        "wrw_16": lambda: hipconv.select_wrw(False, 8, 512, 16, 16, 512, *k3),               # below the 1024-pixel floor
        "wrw_thin": lambda: hipconv.select_wrw(False, 8, 3, 128, 128, 64, *k3),
        "wrw_small": lambda: hipconv.select_wrw(False, 8, 512, 8, 8, 512, 4, 2, 1, 1),      # 512 @ 4x4 coarse grid
        "wrw_k4": lambda: hipconv.select_wrw(False, 8, 128, 64, 64, 256, 4, 2, 1, 1),
        "wrw_dil": lambda: hipconv.select_wrw(False, 8, 128, 64, 64, 128, 4, 2, 3, 2),
        "wrw_bf16": lambda: hipconv.select_wrw(False, 8, 128, 128, 128, 128, *k3, True),
        "fwd_bf16": lambda: hipconv.select(ops.CONV_FWD, 8, 128, 128, 128, 128, *k3, True),
        "fwd_k4": lambda: hipconv.select(ops.CONV_FWD, 8, 128, 64, 64, 256, 4, 2, 1, 1),
    }
    moved = ("fwd", "dx", "wrw_miopen", "wrw_wino", "wrw_32", "wrwT")
    assert hipconv._MATH == {"fp32": "fp32", "bf16": "bf16x3"}
    today = {k: f() for k, f in probes.items()}
    assert today["fwd"] == today["dx"] == "winograd" and today["wrw_miopen"] == "miopen" and today["wrw_wino"] == "winograd", today
    assert today["wrw_thin"] == "thin_mfma" and today["wrw_small"] == "smallmap", today
    assert "bf16x3w" not in today.values()
    hipconv.set_conv_math(fp32="direct_bf16x3_dw")
    now = {k: f() for k, f in probes.items()}                       # (the memo was not stale)
    assert now["fwd"] == now["dx"] == "bf16x3d"
    assert now["wrw_miopen"] == now["wrw_wino"] == now["wrw_32"] == now["wrwT"] == "bf16x3w", now
    assert now["wrw_512_32"] == today["wrw_512_32"] == "winograd"
    assert {k: v for k, v in now.items() if k not in moved} == {k: v for k, v in today.items() if k not in moved}
    # a forced engine is not overridden
    for force in ("winograd", "miopen"):
        hipconv._FORCE = force
        assert hipconv.select_wrw(False, 8, 128, 128, 128, 128, *k3) == force
        hipconv._FORCE = None
    os.environ["IPSR_CONV_ENGINE"] = "winograd"
    try:
        hipconv.reload_env()
        assert hipconv.select_wrw(False, 8, 128, 128, 128, 128, *k3) == "winograd"
        assert hipconv.select(ops.CONV_FWD, 8, 128, 128, 128, 128, *k3) == "winograd"
    finally:
        del os.environ["IPSR_CONV_ENGINE"]
        hipconv.reload_env()
    assert probes["wrw_miopen"]() == "bf16x3w"
    # "direct_bf16x3" keeps the weight gradients where they are
    hipconv.set_conv_math(fp32="direct_bf16x3")
    mid = {k: f() for k, f in probes.items()}
    assert mid["fwd"] == "bf16x3d" and {k: v for k, v in mid.items() if k not in ("fwd", "dx")} == {k: v for k, v in today.items() if k not in ("fwd", "dx")}
    hipconv.set_conv_math(fp32="fp32")
    assert {k: f() for k, f in probes.items()} == today
    assert ops.MATH_CODE["direct_bf16x3_dw"] == ops.MATH_CODE["fp32"] == 0
    e = hipconv._ENGINES["bf16x3w"]
    assert e.data is None and e.wrw is not None and e.sink and not e.bf16_io and not e.fp32_copies and not e.wrw_x_as_dy


def test_the_new_name_is_fp32_only(hipconv):
    with pytest.raises(ValueError):
        hipconv.set_conv_math(bf16="direct_bf16x3_dw")
    assert hipconv._MATH == {"fp32": "fp32", "bf16": "bf16x3"}
