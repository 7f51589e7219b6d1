"""The direct bf16 kernel for the dilated down convolution Conv2d(k4, stride 2, pad 3, dilation 2) on bf16 tensors (ipsr_conv4x4s2_bf16_dil,
ops.conv4x4s2_bf16_dil, engine "bf16d" under `hipconv.set_direct_dilated_bf16(True)`) without a GPU: header, exports and binding table, the
workspace query against the restated plan (tests/bf16_dil_plan.py), the refusals that come before any HIP call, and the dispatcher's switch.
Nothing here launches a kernel; the calls on fake addresses run in a child process with every GPU hidden, as in tests/test_bf16x3_dil_abi.py.
"""
import inspect
import os
import re

import pytest

import bf16_dil_plan as D
from bf16x3_harness import ROOT, fake_pointers, hipconv, lib, refused_calls  # noqa: F401  (fixtures by name)

IPSR_ERR_INVALID, IPSR_ERR_UNSUPPORTED, IPSR_ERR_WORKSPACE = -1, -2, -3
DIL, K4S1 = (4, 2, 3, 2), (4, 1, 1, 1)
STEP = [(64, 256), (128, 128), (256, 64), (512, 32)]               # (channels, H = W) of the step's dilated down convolutions
B16 = 16                                                           # the batch of the bf16 configuration
# what `select` answers for the forward and the input gradient of those four under bf16 activations while the switch is off: MIOpen for
# the two large maps, the split-bf16 Winograd engine where `_bf16_wins` keeps it (>= 256 channels up to 64x64)
OFF = {(64, 256): "miopen", (128, 128): "miopen", (256, 64): "wino_dil", (512, 32): "wino_dil"}
ENTRIES = ("ipsr_conv4x4s2_bf16_dil_workspace_bytes", "ipsr_conv4x4s2_bf16_dil")


@pytest.fixture
def switch(hipconv):
    assert hipconv.direct_dilated_bf16() is False
    yield hipconv
    hipconv.set_direct_dilated_bf16(False)
    hipconv._FORCE = None


def test_header_exports_and_bindings(lib):
    import ctypes
    from deepinpainting_amd import _lib
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ipsr_hip.h")).read(), flags=re.S)
    src = re.sub(r"\s+", " ", src)
    assert "size_t ipsr_conv4x4s2_bf16_dil_workspace_bytes(int mode, int B, int Kc, int Cf, int nh, int nw);" in src
    assert ("int ipsr_conv4x4s2_bf16_dil(int mode, const void* in, const float* weight, void* out, int B, int Kc, int Cf, int nh, int nw, int out_bf16, "
            "void* ws, size_t ws_bytes, void* stream);") in src
    for name in ENTRIES:
        assert hasattr(lib, name), name
    # the argument lists of ipsr_conv4x4s2_bf16, entry for entry
    assert _lib.SIGNATURES[ENTRIES[0]] == _lib.SIGNATURES["ipsr_conv4x4s2_bf16_workspace_bytes"] == (ctypes.c_size_t, [ctypes.c_int] * 6)
    assert _lib.SIGNATURES[ENTRIES[1]] == _lib.SIGNATURES["ipsr_conv4x4s2_bf16"]
    assert lib.ipsr_abi_version() == 15 == _lib.ABI_VERSION


def test_the_cases_reach_their_variants():
    plans = D.check_cases()
    assert plans["one", 0]["nstage"] == 2 and plans["wide", 0]["R"] < 3
    assert plans["cut3", 0]["uneven"] and plans["cut", 0]["nsplit"] == plans["cut", 1]["nsplit"] == 2
    assert len(D.CASES) == 9


def test_workspace_query_equals_the_plan(lib):
    q = lib.ipsr_conv4x4s2_bf16_dil_workspace_bytes
    for cid, (shape, _) in D.CASES.items():
        for mode in (0, 1):
            assert q(mode, *shape) == D.plan(mode, *shape)["ws"] > 0, (cid, mode)
    chans = sorted({c for row in D.STEP_ROWS for c in row[:2]})
    for nw in D.WIDTHS:
        for B in (1, 3, 16):
            for Kc in chans:
                for Cf in chans:
                    for mode in (0, 1):
                        p = D.plan(mode, B, Kc, Cf, nw, nw)
                        assert p is not None and q(mode, B, Kc, Cf, nw, nw) == p["ws"] > 0, (mode, B, Kc, Cf, nw)
    for Kc, Cf, n in D.STEP_ROWS:
        for mode in (0, 1):
            assert q(mode, B16, Kc, Cf, n, n) == D.plan(mode, B16, Kc, Cf, n, n)["ws"] > 0


def test_raw1_never():
    """Two raw buffers always fit: the largest plan of either form is 156672 bytes (tests/bf16_dil_plan.py)."""
    worst = 0
    for nw in D.WIDTHS:
        for K in (16, 48, 64, 80, 128, 512):
            for C in (16, 64, 512):
                for rows in (256 // nw, 512 // nw, 1024 // nw, 3 * (256 // nw)):
                    for mode in (0, 1):
                        p = D.plan(mode, 2, K if mode == 0 else C, C if mode == 0 else K, rows, nw)
                        assert p is not None and p["raw1"] is False, (nw, K, C, rows, mode, p)
                        worst = max(worst, p["lds"])
    assert worst == 156672


@pytest.mark.parametrize("shape,msg", [((0, 1, 16, 16, 12, 24), "coarse width 24"), ((1, 1, 16, 16, 12, 24), "coarse width 24"),
                                       ((0, 1, 16, 16, 1, 256), "coarse width 256"), ((1, 1, 16, 16, 1, 256), "coarse width 256"),
                                       ((0, 1, 16, 8, 16, 16), "8 reduction channels are not a multiple of 16"),
                                       ((1, 1, 8, 16, 16, 16), "8 reduction channels are not a multiple of 16"),
                                       ((0, 1, 16, 16, 12, 16), "12 rows are not a multiple of the 16 rows of a tile"),
                                       ((1, 2, 16, 16, 3, 128), "3 rows are not a multiple of the 2 rows of a tile")],
                         ids=["w24", "w24_c2f", "w256", "w256_c2f", "cf8", "kc8_c2f", "rows", "rows_c2f"])
def test_workspace_query_refuses_with_a_message(lib, shape, msg):
    assert D.plan(*shape) is None
    assert lib.ipsr_conv4x4s2_bf16_dil_workspace_bytes(*shape) == 0
    text = lib.ipsr_last_error().decode("utf-8", "replace")
    assert msg in text and "dilated" in text, text


@pytest.mark.parametrize("shape", [(2, 2, 48, 16, 16, 16), (4, 2, 48, 16, 16, 16), (5, 2, 48, 16, 16, 16), (-1, 2, 48, 16, 16, 16), (0, 0, 48, 16, 16, 16),
                                   (1, 2, 0, 16, 16, 16), (0, 2, 48, 0, 16, 16), (0, 2, 48, 16, 0, 16), (1, 2, 48, 16, 16, 0)],
                         ids=["mode2", "mode4", "mode5", "mode-1", "b0", "kc0", "cf0", "nh0", "nw0"])
def test_workspace_query_is_zero_for_a_bad_argument(lib, shape):
    from deepinpainting_amd import ops
    assert D.plan(*shape) is None
    assert lib.ipsr_conv4x4s2_bf16_dil_workspace_bytes(*shape) == 0
    assert not ops.conv4x4s2_bf16_dil_supported(*shape)


def test_the_k4s2p1_entry_keeps_refusing_the_dilated_modes(lib):
    from deepinpainting_amd import ops
    for mode in (4, 5):
        assert lib.ipsr_conv4x4s2_bf16_workspace_bytes(mode, 2, 48, 16, 16, 16) == 0
        assert not ops.conv4x4s2_bf16_supported(mode, 2, 48, 16, 16, 16)
    good = (2, 48, 16, 16, 16)
    assert ops.conv4x4s2_bf16_dil_supported(ops.S2_FINE_TO_COARSE, *good) and ops.conv4x4s2_bf16_dil_supported(ops.S2_COARSE_TO_FINE, *good)
    assert not ops.conv4x4s2_bf16_dil_supported(ops.S2_DILATED | ops.S2_FINE_TO_COARSE, *good)
    assert not ops.conv4x4s2_bf16_dil_supported(ops.S2_WEIGHT_GRAD, *good)


@pytest.fixture(scope="module")
def refusals(lib):
    good = (2, 48, 16, 16, 16)
    need = lib.ipsr_conv4x4s2_bf16_dil_workspace_bytes(0, *good)
    assert need > 0
    e = "ipsr_conv4x4s2_bf16_dil"
    big = 1 << 30
    # name: (mode, shape, (in, weight, out, ws) offsets or None for a null pointer, workspace bytes)
    calls = {"w24": (0, (1, 16, 16, 12, 24), (0, 0, 0, 0), big), "w256": (1, (1, 16, 16, 1, 256), (0, 0, 0, 0), big),
             "cf8": (0, (1, 16, 8, 16, 16), (0, 0, 0, 0), big), "kc8_c2f": (1, (1, 8, 16, 16, 16), (0, 0, 0, 0), big),
             "rows": (1, (1, 16, 16, 12, 16), (0, 0, 0, 0), big),
             "mode2": (2, good, (0, 0, 0, 0), big), "mode4": (4, good, (0, 0, 0, 0), big), "mode5": (5, good, (0, 0, 0, 0), big),
             "b0": (0, (0, 48, 16, 16, 16), (0, 0, 0, 0), big),
             "null_in": (0, good, (None, 0, 0, 0), big), "null_w": (1, good, (0, None, 0, 0), big), "null_out": (0, good, (0, 0, None, 0), big),
             "null_ws": (1, good, (0, 0, 0, None), big),
             "in+8": (0, good, (8, 0, 0, 0), big), "out+8": (1, good, (0, 0, 8, 0), big), "ws+4": (0, good, (0, 0, 0, 4), big),
             "ws_short": (0, good, (0, 0, 0, 0), need - 1)}
    table = {}
    for name, (mode, shape, off, nbytes) in calls.items():
        ptr = fake_pointers(off)
        for out_bf16 in (0, 1):
            table["%s/%d" % (name, out_bf16)] = (e, (mode, ptr[0], ptr[1], ptr[2], *shape, out_bf16, ptr[3], nbytes, None))
    return refused_calls(table)


@pytest.mark.parametrize("out_bf16", [0, 1], ids=["fp32_out", "bf16_out"])
@pytest.mark.parametrize("case,rc,msg", [("w24", IPSR_ERR_UNSUPPORTED, "coarse width 24"), ("w256", IPSR_ERR_UNSUPPORTED, "coarse width 256"),
                                         ("cf8", IPSR_ERR_UNSUPPORTED, "8 reduction channels"), ("kc8_c2f", IPSR_ERR_UNSUPPORTED, "8 reduction channels"),
                                         ("rows", IPSR_ERR_UNSUPPORTED, "12 rows are not a multiple"),
                                         ("mode2", IPSR_ERR_INVALID, "bad argument"), ("mode4", IPSR_ERR_INVALID, "bad argument"),
                                         ("mode5", IPSR_ERR_INVALID, "bad argument"), ("b0", IPSR_ERR_INVALID, "bad argument"),
                                         ("null_in", IPSR_ERR_INVALID, "null pointer"), ("null_w", IPSR_ERR_INVALID, "null pointer"),
                                         ("null_out", IPSR_ERR_INVALID, "null pointer"), ("null_ws", IPSR_ERR_INVALID, "null pointer"),
                                         ("in+8", IPSR_ERR_INVALID, "align"), ("out+8", IPSR_ERR_INVALID, "align"), ("ws+4", IPSR_ERR_INVALID, "align"),
                                         ("ws_short", IPSR_ERR_WORKSPACE, "workspace")])
def test_refused_before_any_hip_call(refusals, case, rc, msg, out_bf16):
    got, text = refusals["%s/%d" % (case, out_bf16)]
    assert got == rc and msg in text, (got, text)


# ---- the switch ----------------------------------------------------------------------------------------------------------------------------
def _probes(hc, B=B16):
    from deepinpainting_amd import ops
    sel, wrw = hc.select, hc.select_wrw
    p = {}
    for C, H in STEP + [(512, 16)]:                                # 512 @16: a coarse grid 8 wide
        for bf16 in (True, False):
            tag = "%s_%d@%d" % ("bf16" if bf16 else "fp32", C, H)
            p["fwd_" + tag] = lambda C=C, H=H, bf16=bf16: sel(ops.CONV_FWD, B, C, H, H, C, *DIL, bf16)
            p["dx_" + tag] = lambda C=C, H=H, bf16=bf16: sel(ops.CONV_BWD_DATA, B, C, H, H, C, *DIL, bf16)
            p["wrw_" + tag] = lambda C=C, H=H, bf16=bf16: wrw(False, B, C, H, H, C, *DIL, bf16)
    p["k4s1_fwd"] = lambda: sel(ops.CONV_FWD, B, 256, 32, 32, 512, *K4S1, True)
    p["k4s1_dx"] = lambda: sel(ops.CONV_BWD_DATA, B, 256, 32, 32, 512, *K4S1, True)
    p["k3_fwd"] = lambda: sel(ops.CONV_FWD, B, 128, 128, 128, 128, 3, 1, 1, 1, True)
    p["s2_fwd"] = lambda: sel(ops.CONV_FWD, B, 64, 128, 128, 128, 4, 2, 1, 1, True)
    p["s2T_dx"] = lambda: sel(ops.CONVT_BWD_DATA, B, 128, 64, 64, 128, 4, 2, 1, 1, True)
    p["smallmap_fwd"] = lambda: sel(ops.CONV_FWD, 8, 512, 4, 4, 512, *DIL, True)      # 32 positions per batch
    return p


MOVED = ["%s_bf16_%d@%d" % (k, C, H) for C, H in STEP for k in ("fwd", "dx")]


def test_default_off_and_the_option_reaches_it(switch):
    from deepinpainting_amd.models import IPSR
    from deepinpainting_amd.options import Option
    assert switch.direct_dilated_bf16() is False
    assert Option(direct_dilated_bf16=True).direct_dilated_bf16 is True
    src = inspect.getsource(IPSR)
    assert "hipconv.set_direct_dilated_bf16(bool(getattr(opt, 'direct_dilated_bf16', False)))" in src
    switch.set_direct_dilated_bf16(1)
    assert switch.direct_dilated_bf16() is True
    switch.set_direct_dilated_bf16(0)
    assert switch.direct_dilated_bf16() is False


def test_off_answers_as_before(switch):
    from deepinpainting_amd import ops
    hc = switch
    today = {k: f() for k, f in _probes(hc).items()}
    for (C, H), eng in OFF.items():
        assert today["fwd_bf16_%d@%d" % (C, H)] == today["dx_bf16_%d@%d" % (C, H)] == eng, (C, H, today)
        lay = (False, B16, C, H, H, C, *DIL)
        for op in (ops.CONV_FWD, ops.CONV_BWD_DATA):
            assert hc.engine_takes("bf16d", "data", op, lay, True) is False
        assert hc.engine_takes("bf16d", "wrw", None, lay, True) is False
        # `_direct_case` answers from the geometry alone; what keeps the dilated entry out of reach is the entry's switch, which is off
        assert hc._direct_case(lay) == ("dil", (C, C, H // 2, H // 2))
        assert hc._DIRECT_TAKES_SWITCH[False, "dil", "data"] == "bf16_dil_data" and "bf16_dil_data" not in hc._direct_passes_on()
    assert "bf16d" not in [today[k] for k in today if "@" in k and "_fp32_" not in k]


def test_on_moves_the_data_passes_only(switch, monkeypatch):
    from deepinpainting_amd import ops
    hc = switch
    probes = _probes(hc)
    today = {k: f() for k, f in probes.items()}
    hc.set_direct_dilated_bf16(True)
    assert hc.direct_dilated_bf16() is True and not hc.direct_dilated() and not hc.direct_dilated_dw()
    assert hc._MATH == {"fp32": "fp32", "bf16": "bf16x3"}          # independent of set_conv_math
    now = {k: f() for k, f in probes.items()}
    assert all(now[k] == "bf16d" for k in MOVED), now
    # weight gradients, fp32 activations, the coarse grid 8 wide, "smallmap" grids, k4 s1 p1 and the other families: as before
    assert {k: v for k, v in now.items() if k not in MOVED} == {k: v for k, v in today.items() if k not in MOVED}
    for C, H in STEP:
        lay = (False, B16, C, H, H, C, *DIL)
        assert hc.engine_takes("bf16d", "data", ops.CONV_FWD, lay, True) and hc.engine_takes("bf16d", "data", ops.CONV_BWD_DATA, lay, True)
        assert not hc.engine_takes("bf16d", "wrw", None, lay, True)
        assert not hc.engine_takes("bf16d", "data", ops.CONV_FWD, lay, False)                # bf16 activations only
        assert hc._direct_case(lay) == ("dil", (C, C, H // 2, H // 2))
    assert not hc.engine_takes("bf16d", "data", ops.CONV_FWD, (False, B16, 512, 16, 16, 512, *DIL), True)
    # independent of the fp32 switches and of the arithmetic name
    hc.set_direct_dilated(True)
    hc.set_direct_dilated_dw(True)
    try:
        assert all(probes[k]() == "bf16d" for k in MOVED)
        assert probes["fwd_fp32_128@128"]() == "bf16x3d" and probes["wrw_bf16_256@64"]() == today["wrw_bf16_256@64"]
    finally:
        hc.set_direct_dilated(False)
        hc.set_direct_dilated_dw(False)
    # a forced engine is not overridden
    for force in ("miopen", "winograd", "direct"):
        hc._FORCE = force
        assert all(probes[k]() == "miopen" for k in MOVED), force
        hc._FORCE = None
    # ... nor the A/B switch of the bf16 engines
    for val, want in (("none", {k: "miopen" for k in MOVED}), ("all", {k: "wino_dil" for k in MOVED})):
        monkeypatch.setenv("IPSR_BF16_ENGINES", val)
        hc.reload_env()
        assert {k: probes[k]() for k in MOVED} == want, val
    monkeypatch.delenv("IPSR_BF16_ENGINES")
    hc.reload_env()
    assert all(probes[k]() == "bf16d" for k in MOVED)
    # off again: every answer of before
    hc.set_direct_dilated_bf16(False)
    assert {k: f() for k, f in probes.items()} == today


def test_flipping_the_switch_invalidates_the_memo(switch):
    from deepinpainting_amd import ops
    hc = switch
    ask = lambda: hc.select(ops.CONV_FWD, B16, 128, 128, 128, 128, *DIL, True)
    assert ask() == "miopen" and hc._SEL
    hc.set_direct_dilated_bf16(True)
    assert not hc._SEL
    assert ask() == "bf16d" and hc._SEL
    hc.set_direct_dilated_bf16(False)
    assert not hc._SEL and ask() == "miopen"


def test_no_new_engine_and_no_new_opt_in_row(switch):
    assert sorted(switch._ENGINES) == sorted(["winograd", "wino_dil", "wino_s2", "thin", "thin_f2m", "thin_mfma", "smallmap", "direct", "one", "bf16d",
                                              "bf16x3d", "bf16x3w", "miopen"])
    assert sorted(r.key for r in switch._DIRECT_OPT_INS) == sorted(["k3_data", "s2_data", "dil_data", "k3_wrw", "s2_wrw", "dil_wrw", "bf16_dil_data", "bf16_dil_wrw"])
