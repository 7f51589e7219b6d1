"""The split-bf16 direct convolution (io code 2 of ipsr_conv3x3_bf16) without a GPU: its workspace query, the refusals that come
before any HIP call, and the dispatcher's opt-in rule.  Nothing here launches a kernel; the calls on fake addresses run in a child
process with every GPU hidden, as in tests/test_abi_alignment.py.
"""
import json
import os
import subprocess
import sys

import pytest

import bf16_conv_plan as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
IPSR_ERR_INVALID = -1
# (B, Cin, Cout, H, W): the shapes of tests/test_gpu_bf16x3_conv.py
SHAPES = [(2, 16, 48, 16, 16), (3, 48, 80, 32, 16), (2, 64, 64, 2, 256), (2, 32, 64, 12, 64), (1, 128, 128, 16, 16)]


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    from deepinpainting_amd import _lib
    return _lib.lib()


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


def _child():
    sys.path.insert(0, ROOT)
    from deepinpainting_amd import _lib
    L = _lib.lib()
    base, out = 1 << 40, {}
    for name, io, off in (("in+8", 2, (8, 0, 0)), ("out+8", 2, (0, 8, 0)), ("ws+8", 2, (0, 0, 8)), ("io7", 7, (0, 0, 0))):
        for entry, extra in (("ipsr_conv3x3_bf16", ()), ("ipsr_conv3x3_bf16_packed", (0,))):
            rc = getattr(L, entry)(0, base + off[0], base + (1 << 20), base + (2 << 20) + off[1], 2, 32, 16, 16, 48, io, *extra, base + (3 << 20) + off[2], 1 << 40, None)
            out["%s:%s" % (entry, name)] = (rc, L.ipsr_last_error().decode("utf-8", "replace"))
    print(json.dumps(out))


@pytest.fixture(scope="module")
def refusals(lib):
    env = dict(os.environ, HIP_VISIBLE_DEVICES="-1", CUDA_VISIBLE_DEVICES="-1", ROCR_VISIBLE_DEVICES="-1")
    res = subprocess.run([sys.executable, os.path.abspath(__file__), "--child"], env=env, cwd=ROOT, capture_output=True, text=True, timeout=120)
    assert res.returncode == 0, res.stderr[-2000:]
    return json.loads(res.stdout.strip().splitlines()[-1])


@pytest.mark.parametrize("entry", ["ipsr_conv3x3_bf16", "ipsr_conv3x3_bf16_packed"])
@pytest.mark.parametrize("case", ["in+8", "out+8", "ws+8", "io7"])
def test_refused_before_any_hip_call(refusals, entry, case):
    rc, msg = refusals["%s:%s" % (entry, case)]
    assert rc == IPSR_ERR_INVALID and ("io code 7" if case == "io7" else "align") in msg, (rc, msg)


@pytest.fixture
def hipconv(lib, monkeypatch):
    from deepinpainting_amd.models import hipconv as hc
    monkeypatch.setattr(hc, "_FORCE", None)
    monkeypatch.delenv("IPSR_CONV_ENGINE", raising=False)
    hc.reload_env()
    was = hc._MATH["fp32"]
    yield hc
    hc._FORCE = None
    hc.set_conv_math(fp32=was)
    hc.reload_env()


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


if __name__ == "__main__" and sys.argv[1:] == ["--child"]:
    _child()
