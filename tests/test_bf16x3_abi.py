"""The split-bf16 direct convolution (io code 2 of ipsr_conv3x3_bf16) without a GPU: its workspace query, the refusals that come
before any HIP call, and the dispatcher's opt-in rule.  Nothing here launches a kernel; the calls on fake addresses run in a child
process with every GPU hidden, as in tests/test_abi_alignment.py.
"""
import os

import pytest

import bf16_conv_plan as P
from bf16x3_harness import fake_pointers, hipconv, lib, refused_calls  # noqa: F401  (fixtures by name)

IPSR_ERR_INVALID = -1
# (B, Cin, Cout, H, W): the shapes of tests/test_gpu_bf16x3_conv.py
SHAPES = [(2, 16, 48, 16, 16), (3, 48, 80, 32, 16), (2, 64, 64, 2, 256), (2, 32, 64, 12, 64), (1, 128, 128, 16, 16)]


def test_workspace_query_accepts_the_gpu_shapes(lib):
    for B, Cin, Cout, H, W in SHAPES:
        for op in range(4):
            n = lib.ipsr_conv3x3_bf16x3_workspace_bytes(op, B, Cin, H, W, Cout)
            C, K = (Cin, Cout) if op in (0, 2) else (Cout, Cin)
            # at least the zero page and the two planes of packed weights (64-row k tiles, 9 taps, 16 bytes per (row, 8 channels))
            assert n >= 256 + 2 * ((K + 63) // 64) * (C // 16) * 9 * 2 * 64 * 16 and n % 256 == 0, (op, B, Cin, Cout, H, W, n)


@pytest.mark.parametrize("shape,msg", [((0, 1, 16, 12, 24, 16), "width 24"), ((0, 1, 24, 16, 16, 16), "24 reduction channels are not a multiple of 16"),
                                       ((1, 1, 16, 16, 16, 24), "24 reduction channels are not a multiple of 16"),
                                       ((0, 2, 16, 12, 32, 128), "12 rows are not a multiple of the 8 rows of a tile")],
                         ids=["w24", "cin24", "dx_cout24", "rows"])
def test_workspace_query_refuses_with_a_message(lib, shape, msg):
    assert lib.ipsr_conv3x3_bf16x3_workspace_bytes(*shape) == 0
    assert msg in lib.ipsr_last_error().decode("utf-8", "replace")


def test_the_bf16_plan_is_untouched(lib):
    for B, Cin, Cout, H, W in SHAPES:
        for op in range(4):
            assert lib.ipsr_conv3x3_bf16_workspace_bytes(op, B, Cin, H, W, Cout) == P.k3_ws(op, B, Cin, H, W, Cout) > 0


@pytest.fixture(scope="module")
def refusals(lib):
    calls = {}
    for name, io, off in (("in+8", 2, (8, 0, 0, 0)), ("out+8", 2, (0, 0, 8, 0)), ("ws+8", 2, (0, 0, 0, 8)), ("io7", 7, (0, 0, 0, 0))):
        inp, w, out, ws = fake_pointers(off, stride=1 << 20)
        for entry, extra in (("ipsr_conv3x3_bf16", ()), ("ipsr_conv3x3_bf16_packed", (0,))):
            calls["%s:%s" % (entry, name)] = (entry, (0, inp, w, out, 2, 32, 16, 16, 48, io, *extra, ws, 1 << 40, None))
    return refused_calls(calls)


@pytest.mark.parametrize("entry", ["ipsr_conv3x3_bf16", "ipsr_conv3x3_bf16_packed"])
@pytest.mark.parametrize("case", ["in+8", "out+8", "ws+8", "io7"])
def test_refused_before_any_hip_call(refusals, entry, case):
    rc, msg = refusals["%s:%s" % (entry, case)]
    assert rc == IPSR_ERR_INVALID and ("io code 7" if case == "io7" else "align") in msg, (rc, msg)


def test_selection_is_opt_in(hipconv):
    from deepinpainting_amd import ops
    lay = (8, 64, 256, 256, 64, 3, 1, 1, 1)
    probes = {
        "fwd": lambda: hipconv.select(ops.CONV_FWD, *lay),
        "dx": lambda: hipconv.select(ops.CONV_BWD_DATA, *lay),
        "bf16": lambda: hipconv.select(ops.CONV_FWD, *lay, True),
        "wrw": lambda: hipconv.select_wrw(False, *lay),
        "wrw512": lambda: hipconv.select_wrw(False, 8, 512, 32, 32, 512, 3, 1, 1, 1),
        "w24": lambda: hipconv.select(ops.CONV_FWD, 8, 128, 24, 24, 128, 3, 1, 1, 1),       # "winograd" today, a width the direct kernel refuses
        "k4": lambda: hipconv.select(ops.CONV_FWD, 8, 128, 64, 64, 256, 4, 2, 1, 1),
    }
    assert hipconv._MATH["fp32"] == "fp32"
    today = {k: f() for k, f in probes.items()}
    assert today["fwd"] == "winograd" and today["dx"] == "winograd" and today["w24"] == "winograd"
    hipconv.set_conv_math(fp32="direct_bf16x3")
    now = {k: f() for k, f in probes.items()}                       # (the memo was not stale)
    assert now["fwd"] == "bf16x3d" and now["dx"] == "bf16x3d"
    assert {k: now[k] for k in ("bf16", "wrw", "wrw512", "w24", "k4")} == {k: today[k] for k in ("bf16", "wrw", "wrw512", "w24", "k4")}
    # a forced engine is not overridden
    hipconv._FORCE = "winograd"
    assert hipconv.select(ops.CONV_FWD, *lay) == "winograd"
    hipconv._FORCE = None
    os.environ["IPSR_CONV_ENGINE"] = "winograd"
    try:
        hipconv.reload_env()
        assert hipconv.select(ops.CONV_FWD, *lay) == "winograd"
    finally:
        del os.environ["IPSR_CONV_ENGINE"]
        hipconv.reload_env()
    assert hipconv.select(ops.CONV_FWD, *lay) == "bf16x3d"
    hipconv.set_conv_math(fp32="fp32")
    assert {k: f() for k, f in probes.items()} == today
    # the arithmetic handed to the Winograd engines under the opt-in is fp32's
    assert ops.MATH_CODE["direct_bf16x3"] == ops.MATH_CODE["fp32"] == 0
    e = hipconv._ENGINES["bf16x3d"]
    assert e.data is not None and e.wrw is None and not e.bf16_io and not e.fp32_copies


def test_unknown_arithmetic_still_raises(hipconv):
    with pytest.raises(ValueError):
        hipconv.set_conv_math(fp32="nonsense")
    with pytest.raises(ValueError):
        hipconv.set_conv_math(bf16="direct_bf16x3")                 # bf16 activations have the direct bf16 kernel ("bf16d")
    assert hipconv._MATH == {"fp32": "fp32", "bf16": "bf16x3"}


def test_the_direct_names_are_a_chain_of_supersets(hipconv):
    """ops.DIRECT_PASSES is the one table of the opt-in names: each moves what the one before it moves plus more, none is a Winograd
    arithmetic (code 0), none is for bf16 activations."""
    from deepinpainting_amd import ops
    chain = ["direct_bf16x3", "direct_bf16x3_dw", "direct_bf16x3_s2", "direct_bf16x3_s2_dw"]
    assert list(ops.DIRECT_PASSES) == chain
    assert all(ops.DIRECT_PASSES[a] < ops.DIRECT_PASSES[b] for a, b in zip(chain, chain[1:]))       # strict subsets
    assert ops.DIRECT_PASSES[chain[-1]] == {"k3_data", "k3_wrw", "s2_data", "s2_wrw"}
    assert set(ops.MATH_CODE) == {None, "fp32", "bf16x3", "bf16x6", *chain} and all(ops.MATH_CODE[n] == 0 for n in chain)
    for name in chain:
        with pytest.raises(ValueError):
            hipconv.set_conv_math(bf16=name)
    assert hipconv._MATH == {"fp32": "fp32", "bf16": "bf16x3"}
