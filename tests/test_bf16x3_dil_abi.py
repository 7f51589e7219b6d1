"""The split-bf16 direct kernel for the dilated down convolution Conv2d(k4, stride 2, pad 3, dilation 2) on fp32 tensors (modes 4 / 5 of
ipsr_conv4x4s2_bf16x3, ops.conv4x4s2_bf16x3 with ops.S2_DILATED, engine "bf16x3d" under `hipconv.set_direct_dilated(True)`) without a
GPU: the workspace query against the restated plan, the refusals that come before any HIP call, and the dispatcher's switch.  Nothing here
launches a kernel; the calls on fake addresses run in a child process with every GPU hidden, as in tests/test_bf16x3_s2_abi.py.
"""
import pytest

import bf16x3_dil_plan as D
from bf16x3_harness import fake_pointers, hipconv, lib, refused_calls  # noqa: F401  (fixtures by name)

IPSR_ERR_INVALID, IPSR_ERR_UNSUPPORTED, IPSR_ERR_WORKSPACE = -1, -2, -3
DIL, K4S1 = (4, 2, 3, 2), (4, 1, 1, 1)
STEP = [(64, 256), (128, 128), (256, 64), (512, 32)]               # (channels, H = W) of the step's dilated down convolutions


@pytest.fixture
def switch(hipconv):
    assert hipconv.direct_dilated() is False
    yield hipconv
    hipconv.set_direct_dilated(False)


def test_the_cases_reach_their_variants():
    D.check_cases()
    assert D.plan(4, *D.CASES["cut"][0])["nsplit"] == D.plan(5, *D.CASES["cut"][0])["nsplit"] == 2
    for cid in ("wrap", "tiles3", "wide"):
        assert all(D.plan(m, *D.CASES[cid][0])["tiles_per_img"] > 1 for m in (4, 5)), cid
    assert D.plan(4, *D.CASES["wide"][0])["R"] < 3                 # fewer rows in a tile than halo rows around it


def test_workspace_query_equals_the_plan(lib):
    for cid, (shape, _) in D.CASES.items():
        for mode in (4, 5):
            assert lib.ipsr_conv4x4s2_bf16x3_workspace_bytes(mode, *shape) == D.plan(mode, *shape)["ws"] > 0, (cid, mode)
    for Kc, Cf, n in D.STEP_ROWS:
        for mode in (4, 5):
            assert lib.ipsr_conv4x4s2_bf16x3_workspace_bytes(mode, 8, Kc, Cf, n, n) == D.plan(mode, 8, Kc, Cf, n, n)["ws"] > 0, (mode, Kc, Cf, n)


@pytest.mark.parametrize("shape,msg", [((4, 1, 16, 16, 12, 24), "coarse width 24"), ((5, 1, 16, 16, 12, 24), "coarse width 24"), ((4, 1, 16, 16, 8, 8), "coarse width 8"),
                                       ((5, 1, 16, 16, 1, 256), "coarse width 256"),
                                       ((4, 1, 16, 8, 16, 16), "8 reduction channels are not a multiple of 16"),
                                       ((5, 1, 8, 16, 16, 16), "8 reduction channels are not a multiple of 16"),
                                       ((4, 1, 16, 16, 12, 16), "12 rows are not a multiple of the 16 rows of a tile"),
                                       ((5, 2, 16, 16, 3, 128), "3 rows are not a multiple of the 2 rows of a tile"),
                                       ((2, 1, 16, 16, 16, 16), "bad argument"), ((3, 1, 16, 16, 16, 16), "bad argument"),
                                       ((6, 1, 16, 16, 16, 16), "bad argument"), ((4, 0, 16, 16, 16, 16), "bad argument")],
                         ids=["w24", "w24_c2f", "w8", "w256", "c8", "c8_c2f", "rows", "rows_c2f", "mode2", "mode3", "mode6", "b0"])
def test_workspace_query_refuses_with_a_message(lib, shape, msg):
    assert D.plan(*shape) is None
    assert lib.ipsr_conv4x4s2_bf16x3_workspace_bytes(*shape) == 0
    assert msg in lib.ipsr_last_error().decode("utf-8", "replace")


def test_the_bf16_tensor_entry_keeps_refusing_the_dilated_modes(lib):
    from deepinpainting_amd import ops
    for mode in (4, 5):
        assert lib.ipsr_conv4x4s2_bf16_workspace_bytes(mode, 2, 48, 16, 16, 16) == 0
        assert not ops.conv4x4s2_bf16_supported(mode, 2, 48, 16, 16, 16)
    assert lib.ipsr_abi_version() == 15


@pytest.fixture(scope="module")
def refusals(lib):
    good = (2, 48, 16, 16, 16)
    need = lib.ipsr_conv4x4s2_bf16x3_workspace_bytes(4, *good)
    # name: (entry, mode, shape, (in, weight, out, ws) offsets or None for a null pointer, workspace bytes)
    x3 = "ipsr_conv4x4s2_bf16x3"
    calls = {"w24": (x3, 4, (1, 16, 16, 12, 24), (0, 0, 0, 0), 1 << 30), "w8": (x3, 5, (1, 16, 16, 8, 8), (0, 0, 0, 0), 1 << 30),
             "w256": (x3, 4, (1, 16, 16, 1, 256), (0, 0, 0, 0), 1 << 30),
             "c8": (x3, 4, (1, 16, 8, 16, 16), (0, 0, 0, 0), 1 << 30), "c8_c2f": (x3, 5, (1, 8, 16, 16, 16), (0, 0, 0, 0), 1 << 30),
             "rows": (x3, 5, (1, 16, 16, 12, 16), (0, 0, 0, 0), 1 << 30),
             "mode2": (x3, 2, good, (0, 0, 0, 0), 1 << 30), "mode3": (x3, 3, good, (0, 0, 0, 0), 1 << 30), "mode6": (x3, 6, good, (0, 0, 0, 0), 1 << 30),
             "null_in": (x3, 4, good, (None, 0, 0, 0), 1 << 30), "null_ws": (x3, 5, good, (0, 0, 0, None), 1 << 30),
             "in+8": (x3, 4, good, (8, 0, 0, 0), 1 << 30), "out+8": (x3, 5, good, (0, 0, 8, 0), 1 << 30), "ws+4": (x3, 4, good, (0, 0, 0, 4), 1 << 30),
             "ws_short": (x3, 4, good, (0, 0, 0, 0), need - 1),
             "bf16_mode4": ("ipsr_conv4x4s2_bf16", 4, good, (0, 0, 0, 0), 1 << 30), "bf16_mode5": ("ipsr_conv4x4s2_bf16", 5, good, (0, 0, 0, 0), 1 << 30)}
    table = {}
    for name, (entry, mode, shape, off, nbytes) in calls.items():
        ptr = fake_pointers(off)
        io = (0,) if entry == "ipsr_conv4x4s2_bf16" else ()
        table[name] = (entry, (mode, ptr[0], ptr[1], ptr[2], *shape, *io, ptr[3], nbytes, None))
    return refused_calls(table)


@pytest.mark.parametrize("case,rc,msg", [("w24", IPSR_ERR_UNSUPPORTED, "coarse width 24"), ("w8", IPSR_ERR_UNSUPPORTED, "coarse width 8"),
                                         ("w256", IPSR_ERR_UNSUPPORTED, "coarse width 256"), ("c8", IPSR_ERR_UNSUPPORTED, "8 reduction channels"),
                                         ("c8_c2f", IPSR_ERR_UNSUPPORTED, "8 reduction channels"),
                                         ("rows", IPSR_ERR_UNSUPPORTED, "12 rows are not a multiple"), ("mode2", IPSR_ERR_INVALID, "mode 2"),
                                         ("mode3", IPSR_ERR_INVALID, "mode 3"), ("mode6", IPSR_ERR_INVALID, "mode 6"),
                                         ("null_in", IPSR_ERR_INVALID, "null pointer"), ("null_ws", IPSR_ERR_INVALID, "null pointer"),
                                         ("in+8", IPSR_ERR_INVALID, "align"), ("out+8", IPSR_ERR_INVALID, "align"), ("ws+4", IPSR_ERR_INVALID, "align"),
                                         ("ws_short", IPSR_ERR_WORKSPACE, "workspace"),
                                         ("bf16_mode4", IPSR_ERR_INVALID, "bad argument"), ("bf16_mode5", IPSR_ERR_INVALID, "bad argument")])
def test_refused_before_any_hip_call(refusals, case, rc, msg):
    got, text = refusals[case]
    assert got == rc and msg in text, (got, text)


def test_ops_modes(lib):
    from deepinpainting_amd import ops
    assert ops.S2_DILATED == 4 and (ops.S2_FINE_TO_COARSE, ops.S2_COARSE_TO_FINE, ops.S2_WEIGHT_GRAD) == (0, 1, 2)
    good = (2, 48, 16, 16, 16)
    for mode in (0, 1, ops.S2_DILATED | ops.S2_FINE_TO_COARSE, ops.S2_DILATED | ops.S2_COARSE_TO_FINE):
        assert ops.conv4x4s2_bf16x3_supported(mode, *good), mode
    for mode in (2, 3, 6, 7, -1):
        assert not ops.conv4x4s2_bf16x3_supported(mode, *good), mode
    assert not ops.conv4x4s2_bf16x3_supported(4, 1, 16, 16, 12, 24)


def _probes(hc):
    from deepinpainting_amd import ops
    sel, wrw = hc.select, hc.select_wrw
    p = {}
    for C, H in STEP + [(512, 16)]:
        p["fwd_%d@%d" % (C, H)] = lambda C=C, H=H: sel(ops.CONV_FWD, 8, C, H, H, C, *DIL)
        p["dx_%d@%d" % (C, H)] = lambda C=C, H=H: sel(ops.CONV_BWD_DATA, 8, C, H, H, C, *DIL)
        p["wrw_%d@%d" % (C, H)] = lambda C=C, H=H: wrw(False, 8, C, H, H, C, *DIL)
        p["fwd_bf16_%d@%d" % (C, H)] = lambda C=C, H=H: sel(ops.CONV_FWD, 8, C, H, H, C, *DIL, True)
        p["dx_bf16_%d@%d" % (C, H)] = lambda C=C, H=H: sel(ops.CONV_BWD_DATA, 8, C, H, H, C, *DIL, True)
    p["k4s1_fwd"] = lambda: sel(ops.CONV_FWD, 8, 256, 32, 32, 512, *K4S1)
    p["k4s1_dx"] = lambda: sel(ops.CONV_BWD_DATA, 8, 256, 32, 32, 512, *K4S1)
    p["k4s1_wrw"] = lambda: wrw(False, 8, 256, 32, 32, 512, *K4S1)
    p["k3_fwd"] = lambda: sel(ops.CONV_FWD, 8, 128, 128, 128, 128, 3, 1, 1, 1)
    p["s2_fwd"] = lambda: sel(ops.CONV_FWD, 8, 64, 128, 128, 128, 4, 2, 1, 1)
    p["s2T_dx"] = lambda: sel(ops.CONVT_BWD_DATA, 8, 128, 64, 64, 128, 4, 2, 1, 1)
    return p


def test_selection_is_opt_in(switch):
    from deepinpainting_amd import ops
    hc = switch
    probes = _probes(hc)
    moved = ["%s_%d@%d" % (k, C, H) for C, H in STEP for k in ("fwd", "dx")]
    passes_before = {k: set(v) for k, v in ops.DIRECT_PASSES.items()}
    today = {k: f() for k, f in probes.items()}
    assert all(today[k] == "wino_dil" for k in moved), today
    assert today["k4s1_fwd"] == today["k4s1_dx"] == today["k4s1_wrw"] == "wino_dil", today
    assert all(today["wrw_%d@%d" % (C, H)] == "wino_dil" for C, H in STEP[1:]), today
    assert "bf16x3d" not in today.values() and "bf16x3w" not in today.values()
    # the switch on: forward and input gradient of the four step shapes move; everything else answers as today
    hc.set_direct_dilated(True)
    assert hc.direct_dilated() is True
    now = {k: f() for k, f in probes.items()}
    assert all(now[k] == "bf16x3d" for k in moved), now
    assert {k: v for k, v in now.items() if k not in moved} == {k: v for k, v in today.items() if k not in moved}
    assert hc._MATH == {"fp32": "fp32", "bf16": "bf16x3"}          # independent of set_conv_math
    # ... also under every arithmetic name: the switch adds its rows to whatever the name moves
    for name in ("bf16x3", "direct_bf16x3_s2_dw"):
        hc.set_conv_math(fp32=name)
        assert all(probes[k]() == "bf16x3d" for k in moved), name
        assert probes["wrw_128@128"]() == "wino_dil" and probes["k4s1_fwd"]() == "wino_dil"
    hc.set_conv_math(fp32="fp32")
    assert hc.direct_dilated() is True
    # a forced engine is not overridden
    for force in ("winograd", "miopen", "direct"):
        hc._FORCE = force
        for op in (ops.CONV_FWD, ops.CONV_BWD_DATA):
            assert hc.select(op, 8, 128, 128, 128, 128, *DIL) == hc._select(op, (False, 8, 128, 128, 128, 128, *DIL)) != "bf16x3d"
        hc._FORCE = None
    # off again: every answer of today
    hc.set_direct_dilated(False)
    assert {k: f() for k, f in probes.items()} == today
    assert {k: set(v) for k, v in ops.DIRECT_PASSES.items()} == passes_before and len(ops.DIRECT_PASSES) == 4
    assert "direct_dilated" not in ops.MATH_CODE


def test_flipping_the_switch_invalidates_the_memo(switch):
    from deepinpainting_amd import ops
    hc = switch
    ask = lambda: hc.select(ops.CONV_FWD, 8, 128, 128, 128, 128, *DIL)
    assert ask() == "wino_dil" and hc._SEL
    hc.set_direct_dilated(True)
    assert not hc._SEL
    assert ask() == "bf16x3d" and hc._SEL
    hc.set_direct_dilated(False)
    assert not hc._SEL and ask() == "wino_dil"

