"""The weight gradient of the k3 s1 p1 layers on fp32 tensors with split-bf16 operands (forms 2 / 3 of ipsr_conv3x3_bf16_wrw,
ops.conv3x3_bf16x3_wrw, engine "bf16x3w", opt-in `set_conv_math(fp32="direct_bf16x3_dw")`) against fp64 on the GPU.

The error band is derived, not measured (as in tests/test_gpu_bf16x3_conv.py).  For fp32 a: hi = RNE-bf16(a) leaves |a - hi| <= 2^-9 |a|,
lo = RNE-bf16(a - hi) leaves |a - hi - lo| <= 2^-18 |a|; bf16 x bf16 is exact in fp32.  The kernel adds lo*hi + hi*lo + hi*hi, so a
product is off by lo*lo and the two residual terms: <= 3 * 2^-18 |a||b| < 2^-16 |a||b|.  Per element of dW therefore

    |dW - dW64| <= 2^-16 * wrw(|x|, |dy|) + 1e-5 * max|dW64|

with dW64 the fp64 weight gradient of the UNROUNDED operands, wrw(|x|, |dy|) the same reduction of the absolute values and the second term
the fp32-accumulation floor of that file.  Operands: normal draws times a per-channel power of two in 2^-6 .. 2^6.  Every case reduces
B * H * W <= 2048 pixels: there a dropped cross term lands 12-43x outside the band (emulated on the CPU); at 32768 pixels only 2.9x.

The cases and the launch variant each one reaches are in tests/bf16x3_wrw_plan.py (`CASES`, asserted against the restated planner).
"""
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

import bf16x3_wrw_plan as X
from bf16x3_harness import NAN_BITS, _bits, _module_pass, _same, check_bf16_representable, check_guarded, check_out_slice, draw
from bf16x3_harness import _in_band as _in_band_of
from bf16x3_harness import direct_math_deterministic  # noqa: F401  (the fixture `direct_math`)

pytestmark = pytest.mark.gpu

IPSR_ERR_INVALID, IPSR_ERR_UNSUPPORTED, IPSR_ERR_WORKSPACE = -1, -2, -3
F32, BF16 = torch.float32, torch.bfloat16


def _operands(B, Cin, Cout, H, W, seed):
    """(x, dy): normal draws times a per-channel power of two in 2^-6 .. 2^6."""
    g = torch.Generator(device="cuda").manual_seed(seed)
    return draw(g, (B, Cin, H, W), 1), draw(g, (B, Cout, H, W), 1)


def _wrw64(tr, x, dy):
    """fp64 autograd: the weight gradient of the module (Conv2d [Cout][Cin][3][3], ConvTranspose2d [Cin][Cout][3][3]) for grad_output dy."""
    Cin, Cout = x.shape[1], dy.shape[1]
    w = torch.zeros((Cin, Cout, 3, 3) if tr else (Cout, Cin, 3, 3), dtype=torch.float64, device=x.device, requires_grad=True)
    y = F.conv_transpose2d(x.double(), w, None, 1, 1) if tr else F.conv2d(x.double(), w, None, 1, 1)
    return torch.autograd.grad(y, w, dy.double())[0]


def _band(tr, x, dy, d64):
    return 2.0 ** -16 * _wrw64(tr, x.abs(), dy.abs()) + 1e-5 * d64.abs().max()


def _in_band(tag, d, d64, band):
    _in_band_of(tag, d, d64, band, ref="dW64")


_REF = {}


def _case(cid):
    """(x, dy, dW64, band) of a case, computed once and never written."""
    if cid not in _REF:
        tr, B, Cin, Cout, H, W = X.CASES[cid][0]
        x, dy = _operands(B, Cin, Cout, H, W, 97 + len(cid))
        d64 = _wrw64(tr, x, dy)
        _REF[cid] = (x, dy, d64, _band(tr, x, dy, d64))
    return _REF[cid]


def test_the_cases_reach_their_variants():
    X.check_cases()


@pytest.mark.parametrize("cid", list(X.CASES))
def test_split_bf16_weight_gradient(cid, monkeypatch):
    from deepinpainting_amd import _lib, ops
    L = _lib.lib()
    tr, B, Cin, Cout, H, W = X.CASES[cid][0]
    plan = X.plan(tr, B, Cin, H, W, Cout)
    assert ops.conv3x3_bf16x3_wrw_supported(tr, B, Cin, H, W, Cout)
    assert L.ipsr_conv3x3_bf16x3_wrw_workspace_bytes(tr, B, Cin, H, W, Cout) == plan["ws"], (cid, plan)
    x, dy, d64, band = _case(cid)
    wshape = (Cin, Cout, 3, 3) if tr else (Cout, Cin, 3, 3)
    d = ops.conv3x3_bf16x3_wrw(tr, x, dy, Cout)
    torch.cuda.synchronize()
    assert d.dtype == F32 and tuple(d.shape) == wshape
    _in_band(cid, d, d64, band)
    # a second call: the same bits
    assert _same(ops.conv3x3_bf16x3_wrw(tr, x, dy, Cout), d), "%s: two calls differ" % cid
    run = lambda a, b: ops.conv3x3_bf16x3_wrw(tr, a, b, Cout)
    check_guarded(monkeypatch, run, (x, dy), ("x", "dy"), d, plan["ws"], cid)
    check_out_slice(lambda o: ops.conv3x3_bf16x3_wrw(tr, x, dy, Cout, out=o), d, cid)
    check_bf16_representable(run, lambda a, b: _wrw64(tr, a, b), (x, dy), cid, scale="the scale")


def test_wrong_dtype_is_refused():
    from deepinpainting_amd import ops
    x, dy = torch.zeros(1, 16, 8, 16, device="cuda"), torch.zeros(1, 16, 8, 16, device="cuda")
    with pytest.raises(TypeError):
        ops.conv3x3_bf16x3_wrw(False, x.to(BF16), dy, 16)
    with pytest.raises(TypeError):
        ops.conv3x3_bf16x3_wrw(False, x, dy.to(BF16), 16)


@pytest.mark.parametrize("what", ["w24", "form4", "ws_short"])
def test_refusals_write_nothing(what):
    from deepinpainting_amd import _lib, ops
    L = _lib.lib()
    form, B, Cin, H, W, Cout = {"w24": (2, 1, 16, 12, 24, 16), "form4": (4, 1, 16, 8, 16, 16), "ws_short": (3, 1, 16, 8, 16, 16)}[what]
    x = torch.zeros(B, Cin, H, W, device="cuda")
    dy = torch.zeros(B, Cout, H, W, device="cuda")
    dw = torch.empty(Cout, Cin, 3, 3, device="cuda")
    _bits(dw).fill_(NAN_BITS)
    keep = dw.clone()
    ws = torch.empty(1 << 20, dtype=torch.uint8, device="cuda")
    nbytes = ws.numel()
    want, msg = {"w24": (IPSR_ERR_UNSUPPORTED, "width 24"), "form4": (IPSR_ERR_INVALID, "form code 4"), "ws_short": (IPSR_ERR_WORKSPACE, "workspace")}[what]
    if what == "w24":
        assert X.plan(0, B, Cin, H, W, Cout) is None and not ops.conv3x3_bf16x3_wrw_supported(False, B, Cin, H, W, Cout)
        assert msg in L.ipsr_last_error().decode("utf-8", "replace")
        with pytest.raises(NotImplementedError):
            ops.conv3x3_bf16x3_wrw(False, x, dy, Cout)
    if what == "ws_short":
        nbytes = L.ipsr_conv3x3_bf16x3_wrw_workspace_bytes(1, B, Cin, H, W, Cout) - 1
        assert nbytes > 0
    torch.cuda.synchronize()
    rc = L.ipsr_conv3x3_bf16_wrw(form, x.data_ptr(), dy.data_ptr(), dw.data_ptr(), B, Cin, H, W, Cout, ws.data_ptr(), nbytes, ops._stream())
    text = L.ipsr_last_error().decode("utf-8", "replace")
    torch.cuda.synchronize()
    assert rc == want and msg in text, (rc, text)
    assert _same(dw, keep), "dW was written by a refused call"


# ---- through the modules ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mk", [lambda: nn.Conv2d(64, 64, 3, padding=1), lambda: nn.ConvTranspose2d(128, 64, 3, padding=1)], ids=["conv64", "convT128_64"])
def test_modules_run_all_three_passes_when_asked(mk, direct_math):
    hipconv = direct_math
    torch.manual_seed(7)
    m = mk().cuda()
    tr = isinstance(m, nn.ConvTranspose2d)
    g = torch.Generator(device="cuda").manual_seed(11)
    x = torch.randn(2, m.in_channels, 32, 32, device="cuda", generator=g)
    dy = torch.randn(2, m.out_channels, 32, 32, device="cuda", generator=g)
    assert hipconv._MATH["fp32"] == "fp32"
    today, y0, dx0, dw0 = _module_pass(hipconv, m, x, dy)
    assert today["forward"] == "winograd" and today["input_grad"] == "winograd" and today["weight_grad"] != "bf16x3w", today
    # Today's weight gradient of these two layers is MIOpen's, whose solver may add its partial sums with atomics: bits can only be
    # compared across settings where today's engine repeats its OWN bits from one call to the next.  Where it does not, the engine
    # must be the same and the result inside today's 1e-4 band of the fp32 engines (tests/test_gpu_conv.py).
    repeats = _same(_module_pass(hipconv, m, x, dy)[3], dw0)
    print("today's weight gradient on %r repeats its bits: %s" % (today["weight_grad"], repeats))

    def as_today(dwn):
        if repeats:
            return _same(dwn, dw0)
        return float((dwn.double() - dw0.double()).abs().max() / dw0.double().abs().max()) <= 1e-4
    # "direct_bf16x3": the weight gradient's engine and bits are today's
    hipconv.set_conv_math(fp32="direct_bf16x3")
    mid, _, _, dw_mid = _module_pass(hipconv, m, x, dy)
    assert mid["forward"] == "bf16x3d" and mid["weight_grad"] == today["weight_grad"] and as_today(dw_mid), (mid, today)
    hipconv.set_conv_math(fp32="direct_bf16x3_dw")
    seen, y, dx, dw = _module_pass(hipconv, m, x, dy)
    assert seen == {"forward": "bf16x3d", "input_grad": "bf16x3d", "weight_grad": "bf16x3w"}, seen
    # fp64 autograd
    f = (lambda a, ww: F.conv_transpose2d(a, ww, None, 1, 1)) if tr else (lambda a, ww: F.conv2d(a, ww, None, 1, 1))
    xd, wd = x.double().requires_grad_(True), m.weight.detach().double().requires_grad_(True)
    y64 = f(xd, wd)
    dx64, dw64 = torch.autograd.grad(y64, (xd, wd), dy.double())
    y64 = y64.detach()
    wa = m.weight.detach().abs().double()
    g_fwd, g_bwd = (F.conv_transpose2d, F.conv2d) if tr else (F.conv2d, F.conv_transpose2d)
    _in_band("module forward", y, y64, 2.0 ** -16 * g_fwd(x.abs().double(), wa, None, 1, 1) + 1e-5 * y64.abs().max())
    _in_band("module input gradient", dx, dx64, 2.0 ** -16 * g_bwd(dy.abs().double(), wa, None, 1, 1) + 1e-5 * dx64.abs().max())
    _in_band("module weight gradient", dw, dw64, _band(tr, x, dy, dw64))
    # back on the default: the engines of today, the bits of today
    hipconv.set_conv_math(fp32="fp32")
    again, y1, dx1, dw1 = _module_pass(hipconv, m, x, dy)
    assert again == today and _same(y1, y0) and _same(dx1, dx0) and as_today(dw1)
