"""The direct bf16 weight gradient of the dilated layer Conv2d(k4, stride 2, pad 3, dilation 2) on bf16 tensors
(ipsr_conv4x4s2_bf16_dil_wrw, ops.conv4x4s2_bf16_dil_wrw, engine "bf16d" under `hipconv.set_direct_dilated_bf16_dw(True)`) without a GPU:
header, exports and binding table, the workspace query against the restated plan (tests/bf16_dil_wrw_plan.py), the refusals that come
before any HIP call, and the dispatcher's switch.  Nothing here launches a kernel; the calls on fake addresses run in a child process with
every GPU hidden, as in tests/test_bf16_dil_abi.py.
"""
import inspect
import os
import re

import pytest

import bf16_dil_wrw_plan as X
from bf16x3_harness import ROOT, fake_pointers, hipconv, lib, refused_calls  # noqa: F401  (fixtures by name)
from test_bf16_dil_abi import B16, DIL, STEP, _probes

IPSR_ERR_INVALID, IPSR_ERR_UNSUPPORTED, IPSR_ERR_WORKSPACE = -1, -2, -3
ENTRIES = ("ipsr_conv4x4s2_bf16_dil_wrw_workspace_bytes", "ipsr_conv4x4s2_bf16_dil_wrw")
WHO = "bf16 dilated 4x4 stride-2 weight gradient"
MOVED = ["wrw_bf16_%d@%d" % row for row in STEP]
# what `select_wrw` answers for those four under bf16 activations at batch 16 while the switch is off
OFF = {(64, 256): "miopen", (128, 128): "miopen", (256, 64): "wino_dil", (512, 32): "wino_dil"}


@pytest.fixture
def switch(hipconv):
    assert hipconv.direct_dilated_bf16_dw() is False and hipconv.direct_dilated_bf16() is False
    yield hipconv
    hipconv.set_direct_dilated_bf16_dw(False)
    hipconv.set_direct_dilated_bf16(False)
    hipconv.set_direct_dilated(False)
    hipconv.set_direct_dilated_dw(False)
    hipconv._FORCE = None


def test_the_cases_reach_their_variants():
    X.check_cases()
    assert len(X.CASES) == 9


def test_header_exports_and_bindings(lib):
    from deepinpainting_amd import _lib
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ipsr_hip.h")).read(), flags=re.S)
    src = re.sub(r"\s+", " ", src)
    assert "size_t ipsr_conv4x4s2_bf16_dil_wrw_workspace_bytes(int B, int Kc, int Cf, int nh, int nw);" in src
    assert ("int ipsr_conv4x4s2_bf16_dil_wrw(const void* fine, const void* coarse, float* dw, int B, int Kc, int Cf, int nh, int nw, "
            "void* ws, size_t ws_bytes, void* stream);") in src
    for name in ENTRIES:
        assert hasattr(lib, name), name
        assert getattr(lib, name).argtypes == _lib.SIGNATURES[name][1]
    # the argument lists of the split-bf16 sibling, entry for entry
    assert _lib.SIGNATURES[ENTRIES[0]] == _lib.SIGNATURES["ipsr_conv4x4s2_bf16x3_dil_wrw_workspace_bytes"]
    assert _lib.SIGNATURES[ENTRIES[1]] == _lib.SIGNATURES["ipsr_conv4x4s2_bf16x3_dil_wrw"]
    assert lib.ipsr_abi_version() == 15 == _lib.ABI_VERSION


def test_workspace_query_equals_the_plan(lib):
    q = lib.ipsr_conv4x4s2_bf16_dil_wrw_workspace_bytes
    for cid, (shape, _) in X.CASES.items():
        assert q(*shape) == X.plan(*shape)["ws"] > 256, cid
    for row in X.STEP_ROWS:
        assert q(B16, *row) == X.plan(B16, *row)["ws"] > 256, row
    refused = 0
    for B in range(1, 6):
        for Kc in (1, 127, 128, 129, 340):
            for Cf in (1, 31, 32, 33, 380):
                for nw in (8, 16, 24, 32, 64, 128, 256):
                    rs = max(1, 64 // nw)
                    for nh in (rs, 3 * rs, 3 * rs + 1, 4 * rs, 16):
                        p = X.plan(B, Kc, Cf, nh, nw)
                        got = q(B, Kc, Cf, nh, nw)
                        assert got == (p["ws"] if p else 0), (B, Kc, Cf, nh, nw, got)
                        if p is None:
                            refused += 1
                            assert lib.ipsr_last_error().decode("utf-8", "replace").startswith(WHO), (B, Kc, Cf, nh, nw)
    assert refused


def test_the_lds_plan_is_the_one_plane_ring():
    """Half the split-bf16 sibling's ring: one plane instead of hi | lo."""
    import bf16x3_dil_wrw_plan as S
    for nw in (16, 32, 64, 128):
        p, s = X.plan(2, 64, 64, 4, nw), S.plan(2, 64, 64, 4, nw)
        assert p["lds"] == X.LDS[nw] and 2 * p["ring"] == s["ring"] and p["ws"] == s["ws"] + 256
        assert {k: p[k] for k in ("RS", "spw", "nsplit", "steps")} == {k: s[k] for k in ("RS", "spw", "nsplit", "steps")}


@pytest.mark.parametrize("shape,msg", [((1, 16, 16, 4, 24), "coarse width 24"), ((1, 16, 16, 8, 8), "coarse width 8"), ((1, 16, 16, 1, 256), "coarse width 256"),
                                       ((1, 16, 16, 6, 16), "6 coarse rows are not a multiple of the 4 rows of a stage"),
                                       ((2, 16, 16, 3, 32), "3 coarse rows are not a multiple of the 2 rows of a stage"),
                                       ((0, 16, 16, 4, 16), "bad argument"), ((1, 0, 16, 4, 16), "bad argument"), ((1, 16, 0, 4, 16), "bad argument"),
                                       ((1, 16, 16, 0, 16), "bad argument"), ((1, 16, 16, 4, 0), "bad argument")],
                         ids=["w24", "w8", "w256", "rows16", "rows32", "b0", "kc0", "cf0", "nh0", "nw0"])
def test_workspace_query_refuses_with_a_message(lib, shape, msg):
    from deepinpainting_amd import ops
    assert X.plan(*shape) is None
    assert lib.ipsr_conv4x4s2_bf16_dil_wrw_workspace_bytes(*shape) == 0
    text = lib.ipsr_last_error().decode("utf-8", "replace")
    assert msg in text and ("dil" in text), text
    assert not ops.conv4x4s2_bf16_dil_wrw_supported(*shape)


@pytest.fixture(scope="module")
def refusals(lib):
    good = (2, 48, 16, 8, 16)
    need = lib.ipsr_conv4x4s2_bf16_dil_wrw_workspace_bytes(*good)
    assert need > 256
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
        table[name] = ("ipsr_conv4x4s2_bf16_dil_wrw", (ptr[0], ptr[1], ptr[2], *shape, ptr[3], nbytes, None))
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


def test_ops_supported(lib):
    from deepinpainting_amd import ops
    for row in X.STEP_ROWS:
        assert ops.conv4x4s2_bf16_dil_wrw_supported(B16, *row), row
    assert not ops.conv4x4s2_bf16_dil_wrw_supported(1, 16, 16, 4, 24)
    assert not ops.conv4x4s2_bf16_dil_wrw_supported(1, 16, 16, 6, 16)
    # the k4 s2 p1 kernel keeps refusing the 128-wide grid
    assert not ops.conv4x4s2_bf16_wrw_supported(1, 32, 64, 2, 128) and ops.conv4x4s2_bf16_dil_wrw_supported(1, 32, 64, 2, 128)


# ---- the switch ----------------------------------------------------------------------------------------------------------------------------
def test_default_off_and_the_option_reaches_it(switch):
    from deepinpainting_amd.models import IPSR
    from deepinpainting_amd.options import Option
    assert switch.direct_dilated_bf16_dw() is False
    assert Option(direct_dilated_bf16_dw=True).direct_dilated_bf16_dw is True
    src = inspect.getsource(IPSR)
    assert "hipconv.set_direct_dilated_bf16_dw(bool(getattr(opt, 'direct_dilated_bf16_dw', False)))" in src
    assert src.index("set_direct_dilated_bf16(") < src.index("set_direct_dilated_bf16_dw(")
    switch.set_direct_dilated_bf16_dw(1)
    assert switch.direct_dilated_bf16_dw() is True
    switch.set_direct_dilated_bf16_dw(0)
    assert switch.direct_dilated_bf16_dw() is False


def test_off_answers_as_before(switch):
    from deepinpainting_amd import ops
    hc = switch
    today = {k: f() for k, f in _probes(hc).items()}
    for (C, H), eng in OFF.items():
        assert today["wrw_bf16_%d@%d" % (C, H)] == eng, (C, H, today)
        lay = (False, B16, C, H, H, C, *DIL)
        assert hc.engine_takes("bf16d", "wrw", None, lay, True) is False
        # `_direct_case` answers from the geometry alone; what keeps the dilated entry out of reach is the entry's switch, which is off
        assert hc._direct_case(lay) == ("dil", (C, C, H // 2, H // 2))
        assert hc._DIRECT_TAKES_SWITCH[False, "dil", "wrw"] == "bf16_dil_wrw" and "bf16_dil_wrw" not in hc._direct_passes_on()
    assert "bf16d" not in [today[k] for k in today if "@" in k and "_fp32_" not in k]
    # only the data switch: the weight gradient's own switch is still off, it is still not taken and answers as before
    hc.set_direct_dilated_bf16(True)
    assert "bf16_dil_wrw" not in hc._direct_passes_on()
    for (C, H), eng in OFF.items():
        lay = (False, B16, C, H, H, C, *DIL)
        assert hc._direct_case(lay) == ("dil", (C, C, H // 2, H // 2))
        assert hc.engine_takes("bf16d", "wrw", None, lay, True) is False
        assert hc.engine_takes("bf16d", "data", ops.CONV_FWD, lay, True) is True
        assert hc.select_wrw(False, B16, C, H, H, C, *DIL, True) == eng


def test_on_moves_the_four_weight_gradients_only(switch, monkeypatch):
    from deepinpainting_amd import ops
    hc = switch
    probes = _probes(hc)
    today = {k: f() for k, f in probes.items()}
    hc.set_direct_dilated_bf16_dw(True)
    assert hc.direct_dilated_bf16_dw() is True and not hc.direct_dilated_bf16() and not hc.direct_dilated() and not hc.direct_dilated_dw()
    assert hc._MATH == {"fp32": "fp32", "bf16": "bf16x3"}          # independent of set_conv_math
    now = {k: f() for k, f in probes.items()}
    assert sorted(k for k in now if now[k] != today[k]) == sorted(MOVED), now
    assert all(now[k] == "bf16d" for k in MOVED), now
    for C, H in STEP:
        lay = (False, B16, C, H, H, C, *DIL)
        assert hc.engine_takes("bf16d", "wrw", None, lay, True)
        assert not hc.engine_takes("bf16d", "wrw", None, lay, False)                         # bf16 activations only
        assert not hc.engine_takes("bf16d", "data", ops.CONV_FWD, lay, True) and not hc.engine_takes("bf16d", "data", ops.CONV_BWD_DATA, lay, True)
        assert hc._direct_case(lay) == ("dil", (C, C, H // 2, H // 2))
    # the coarse grid 8 wide, a transposed layer of the same numbers and netD's k4 s1 p1 are not taken
    assert not hc.engine_takes("bf16d", "wrw", None, (False, B16, 512, 16, 16, 512, *DIL), True)
    assert not hc.engine_takes("bf16d", "wrw", None, (True, B16, 128, 64, 64, 128, *DIL), True)
    assert hc.select_wrw(False, B16, 256, 32, 32, 512, 4, 1, 1, 1, True) != "bf16d"
    assert hc.select_wrw(False, 8, 512, 4, 4, 512, *DIL, True) == "smallmap"                # "smallmap" grids stay
    # independent of the three other dilated switches: each moves its own passes
    base_fp32 = {k: today[k] for k in today if "_fp32_" in k}
    hc.set_direct_dilated_bf16(True)
    both = {k: f() for k, f in probes.items()}
    assert all(both["%s_bf16_%d@%d" % (kind, C, H)] == "bf16d" for C, H in STEP for kind in ("fwd", "dx", "wrw")), both
    assert {k: both[k] for k in base_fp32} == base_fp32
    hc.set_direct_dilated_bf16(False)
    hc.set_direct_dilated(True)
    hc.set_direct_dilated_dw(True)
    try:
        mixed = {k: f() for k, f in probes.items()}
        assert all(mixed[k] == "bf16d" for k in MOVED)
        assert mixed["fwd_fp32_128@128"] == "bf16x3d" and mixed["wrw_fp32_128@128"] == "bf16x3w"
        assert all(mixed["%s_bf16_%d@%d" % (kind, C, H)] == today["%s_bf16_%d@%d" % (kind, C, H)] for C, H in STEP for kind in ("fwd", "dx"))
    finally:
        hc.set_direct_dilated(False)
        hc.set_direct_dilated_dw(False)
    # a forced engine is not overridden
    for force in ("miopen", "winograd", "direct"):
        hc._FORCE = force
        assert all(probes[k]() == "miopen" for k in MOVED), force
        hc._FORCE = None
    # ... nor the A/B switch of the bf16 engines
    for val, want in (("none", {k: "miopen" for k in MOVED}), ("all", {"wrw_bf16_64@256": "miopen", "wrw_bf16_128@128": "wino_dil",
                                                                      "wrw_bf16_256@64": "wino_dil", "wrw_bf16_512@32": "wino_dil"})):
        monkeypatch.setenv("IPSR_BF16_ENGINES", val)
        hc.reload_env()
        assert {k: probes[k]() for k in MOVED} == want, val
    monkeypatch.delenv("IPSR_BF16_ENGINES")
    hc.reload_env()
    assert all(probes[k]() == "bf16d" for k in MOVED)
    # off again: every answer of before
    hc.set_direct_dilated_bf16_dw(False)
    assert {k: f() for k, f in probes.items()} == today


def test_flipping_the_switch_invalidates_the_memo(switch):
    hc = switch
    ask = lambda: hc.select_wrw(False, B16, 128, 128, 128, 128, *DIL, True)
    assert ask() == "miopen" and hc._SEL
    hc.set_direct_dilated_bf16_dw(True)
    assert not hc._SEL
    assert ask() == "bf16d" and hc._SEL
    hc.set_direct_dilated_bf16_dw(False)
    assert not hc._SEL and ask() == "miopen"


def test_the_engine_dispatches_on_the_geometry(switch, monkeypatch):
    from deepinpainting_amd import ops
    hc = switch
    calls = []
    monkeypatch.setattr(ops, "conv4x4s2_bf16_wrw", lambda *a, **k: calls.append(("s2", a, k)))
    monkeypatch.setattr(ops, "conv4x4s2_bf16_dil_wrw", lambda *a, **k: calls.append(("dil", a, k)))
    hc.set_direct_dilated_bf16_dw(True)
    run = hc._ENGINES["bf16d"].wrw
    run("x", "dy", (False, 8, 64, 32, 32, 128, 4, 2, 1, 1), "bf16x3", "sink")
    run("x", "dy", (False, 8, 64, 32, 32, 128, 4, 2, 3, 2), "bf16x3", "sink")
    run("x", "dy", (False, 2, 128, 256, 256, 128, 4, 2, 3, 2), "bf16x3", None)
    assert calls == [("s2", ("x", "dy", 8, 128, 64, 16, 16), {"out": "sink"}),
                     ("dil", ("x", "dy", 8, 128, 64, 16, 16), {"out": "sink"}),         # (fine, coarse) = (x, dy)
                     ("dil", ("x", "dy", 2, 128, 128, 128, 128), {"out": None})]


def test_no_new_engine_and_no_new_opt_in_row(switch):
    assert sorted(switch._ENGINES) == sorted(["winograd", "wino_dil", "wino_s2", "thin", "thin_f2m", "thin_mfma", "smallmap", "direct", "one", "bf16d",
                                              "bf16x3d", "bf16x3w", "miopen"])
    assert sorted(r.key for r in switch._DIRECT_OPT_INS) == sorted(["k3_data", "s2_data", "dil_data", "k3_wrw", "s2_wrw", "dil_wrw", "bf16_dil_data", "bf16_dil_wrw"])
