"""The weight gradient of the k4 s2 p1 layers on fp32 tensors with split-bf16 operands (ipsr_conv4x4s2_bf16x3_wrw,
ops.conv4x4s2_bf16x3_wrw, engine "bf16x3w", opt-in `set_conv_math(fp32="direct_bf16x3_s2_dw")`) against fp64 on the GPU.

The error band is derived, not measured (as in tests/test_gpu_bf16x3_wrw.py).  For fp32 a: hi = RNE-bf16(a) leaves |a - hi| <= 2^-9 |a|,
lo = RNE-bf16(a - hi) leaves |a - hi - lo| <= 2^-18 |a|; bf16 x bf16 is exact in fp32.  The kernel adds lo*hi + hi*lo + hi*hi, so a
product is off by lo*lo and the two residual terms: <= 3 * 2^-18 |a||b| < 2^-16 |a||b|.  Per element of dW therefore

    |dW - dW64| <= 2^-16 * wrw(|fine|, |coarse|) + 1e-5 * max|dW64|

with dW64 the fp64 weight gradient of the UNROUNDED operands, wrw(|fine|, |coarse|) the same reduction of the absolute values and the second
term the fp32-accumulation floor of the sibling tests.  Operands: normal draws times a per-channel power of two in 2^-6 .. 2^6.  Every case
reduces B * nh * nw <= 2048 coarse pixels: emulated on the CPU in fp64 on these shapes (other draws), the full three-term arithmetic lands at
<= 0.13 of the band and either cross term dropped 17-38x outside it; at 8192 pixels the margin shrinks to 6x.

The cases and the launch variant each one reaches are in tests/bf16x3_s2_wrw_plan.py (`CASES`, asserted against the restated planner).

Measured on MI355X, worst |err| / band per case: one 0.131, wrap 0.070, w32 0.083, w64 0.065, batch 0.057 (the 16 taps of `one`:
0.063 .. 0.170 of their own bands); bf16-representable operands 5.1e-08 .. 1.1e-07 of the scale; through the modules 0.046 .. 0.081.
"""
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

import bf16x3_s2_wrw_plan as X
from bf16x3_harness import NAN_BITS, _bits, _module_pass, _same, check_bf16_representable, check_guarded, check_out_slice, draw
from bf16x3_harness import _in_band as _in_band_of
from bf16x3_harness import direct_math_deterministic  # noqa: F401  (the fixture `direct_math`)

pytestmark = pytest.mark.gpu

IPSR_ERR_INVALID, IPSR_ERR_UNSUPPORTED, IPSR_ERR_WORKSPACE = -1, -2, -3
F32, BF16 = torch.float32, torch.bfloat16


def _operands(B, Kc, Cf, nh, nw, seed):
    """(fine, coarse): normal draws times a per-channel power of two in 2^-6 .. 2^6."""
    g = torch.Generator(device="cuda").manual_seed(seed)
    return draw(g, (B, Cf, 2 * nh, 2 * nw), 1), draw(g, (B, Kc, nh, nw), 1)


def _wrw64(fine, coarse):
    """fp64 autograd: the weight gradient [Kc][Cf][4][4] of Conv2d(Cf -> Kc, k4 s2 p1) on `fine` for grad_output `coarse`."""
    w = torch.zeros(coarse.shape[1], fine.shape[1], 4, 4, dtype=torch.float64, device=fine.device, requires_grad=True)
    return torch.autograd.grad(F.conv2d(fine.double(), w, None, 2, 1), w, coarse.double())[0]


def _band(fine, coarse, d64):
    return 2.0 ** -16 * _wrw64(fine.abs(), coarse.abs()) + 1e-5 * d64.abs().max()


def _in_band(tag, d, d64, band):
    _in_band_of(tag, d, d64, band, ref="dW64")


_REF = {}


def _case(cid):
    """(fine, coarse, dW64, band) of a case, computed once and never written."""
    if cid not in _REF:
        B, Kc, Cf, nh, nw = X.CASES[cid][0]
        fine, coarse = _operands(B, Kc, Cf, nh, nw, 131 + len(cid))
        d64 = _wrw64(fine, coarse)
        _REF[cid] = (fine, coarse, d64, _band(fine, coarse, d64))
    return _REF[cid]


def test_the_cases_reach_their_variants():
    X.check_cases()


@pytest.mark.parametrize("cid", list(X.CASES))
def test_split_bf16_s2_weight_gradient(cid, monkeypatch):
    from deepinpainting_amd import _lib, ops
    L = _lib.lib()
    B, Kc, Cf, nh, nw = shape = X.CASES[cid][0]
    plan = X.plan(*shape)
    assert ops.conv4x4s2_bf16x3_wrw_supported(*shape)
    assert L.ipsr_conv4x4s2_bf16x3_wrw_workspace_bytes(*shape) == plan["ws"], (cid, plan)
    fine, coarse, d64, band = _case(cid)
    d = ops.conv4x4s2_bf16x3_wrw(fine, coarse, *shape)
    torch.cuda.synchronize()
    assert d.dtype == F32 and tuple(d.shape) == (Kc, Cf, 4, 4)
    _in_band(cid, d, d64, band)
    # a second call: the same bits
    assert _same(ops.conv4x4s2_bf16x3_wrw(fine, coarse, *shape), d), "%s: two calls differ" % cid
    run = lambda f, c: ops.conv4x4s2_bf16x3_wrw(f, c, *shape)
    check_guarded(monkeypatch, run, (fine, coarse), ("fine", "coarse"), d, plan["ws"], cid)
    check_out_slice(lambda o: ops.conv4x4s2_bf16x3_wrw(fine, coarse, *shape, out=o), d, cid)
    check_bf16_representable(run, _wrw64, (fine, coarse), cid, scale="the scale")


def test_every_tap_is_inside_its_own_band():
    """A swapped row or column parity moves whole taps: each of the 16 taps against a band of its own scale."""
    from deepinpainting_amd import ops
    shape = X.CASES["one"][0]
    fine, coarse, d64, _ = _case("one")
    d = ops.conv4x4s2_bf16x3_wrw(fine, coarse, *shape)
    torch.cuda.synchronize()
    prod = 2.0 ** -16 * _wrw64(fine.abs(), coarse.abs())
    worst = []
    for r in range(4):
        for s in range(4):
            band = prod[:, :, r, s] + 1e-5 * d64[:, :, r, s].abs().max()
            worst.append(float(((d[:, :, r, s].double() - d64[:, :, r, s]).abs() / band).max()))
    print("one, per tap: max |err| / band " + " ".join("%.3f" % v for v in worst))
    assert max(worst) <= 1.0, worst


def test_wrong_dtype_is_refused():
    from deepinpainting_amd import ops
    fine, coarse = torch.zeros(1, 16, 8, 32, device="cuda"), torch.zeros(1, 16, 4, 16, device="cuda")
    with pytest.raises(TypeError):
        ops.conv4x4s2_bf16x3_wrw(fine.to(BF16), coarse, 1, 16, 16, 4, 16)
    with pytest.raises(TypeError):
        ops.conv4x4s2_bf16x3_wrw(fine, coarse.to(BF16), 1, 16, 16, 4, 16)


@pytest.mark.parametrize("what", ["w24", "nh6", "ws_short"])
def test_refusals_write_nothing(what):
    from deepinpainting_amd import _lib, ops
    L = _lib.lib()
    B, Kc, Cf, nh, nw = shape = {"w24": (1, 16, 16, 4, 24), "nh6": (1, 16, 16, 6, 16), "ws_short": (1, 16, 16, 4, 16)}[what]
    fine = torch.zeros(B, Cf, 2 * nh, 2 * nw, device="cuda")
    coarse = torch.zeros(B, Kc, nh, nw, device="cuda")
    dw = torch.empty(Kc, Cf, 4, 4, device="cuda")
    _bits(dw).fill_(NAN_BITS)
    keep = dw.clone()
    ws = torch.empty(1 << 20, dtype=torch.uint8, device="cuda")
    nbytes = ws.numel()
    want, msg = {"w24": (IPSR_ERR_UNSUPPORTED, "width 24"), "nh6": (IPSR_ERR_UNSUPPORTED, "6 coarse rows"), "ws_short": (IPSR_ERR_WORKSPACE, "workspace")}[what]
    if what == "ws_short":
        nbytes = L.ipsr_conv4x4s2_bf16x3_wrw_workspace_bytes(*shape) - 1
        assert nbytes > 0
    else:
        assert X.plan(*shape) is None and not ops.conv4x4s2_bf16x3_wrw_supported(*shape)
        assert msg in L.ipsr_last_error().decode("utf-8", "replace")
        with pytest.raises(NotImplementedError):
            ops.conv4x4s2_bf16x3_wrw(fine, coarse, *shape)
    torch.cuda.synchronize()
    rc = L.ipsr_conv4x4s2_bf16x3_wrw(fine.data_ptr(), coarse.data_ptr(), dw.data_ptr(), *shape, ws.data_ptr(), nbytes, ops._stream())
    text = L.ipsr_last_error().decode("utf-8", "replace")
    torch.cuda.synchronize()
    assert rc == want and msg in text, (rc, text)
    assert _same(dw, keep), "dW was written by a refused call"


# ---- through the modules ---------------------------------------------------------------------------------------------------------------
COARSE = 16                                                     # the coarse grid of the module test: the smallest the rule admits


@pytest.mark.parametrize("mk", [lambda: nn.Conv2d(64, 128, 4, 2, 1), lambda: nn.ConvTranspose2d(128, 64, 4, 2, 1)], ids=["conv64_128", "convT128_64"])
def test_modules_run_all_three_passes_when_asked(mk, direct_math):
    hipconv = direct_math
    torch.manual_seed(7)
    m = mk().cuda()
    tr = isinstance(m, nn.ConvTranspose2d)
    g = torch.Generator(device="cuda").manual_seed(11)
    hin, hout = (COARSE, 2 * COARSE) if tr else (2 * COARSE, COARSE)
    x = torch.randn(2, m.in_channels, hin, hin, device="cuda", generator=g)
    dy = torch.randn(2, m.out_channels, hout, hout, device="cuda", generator=g)
    assert hipconv._MATH["fp32"] == "fp32"
    today, y0, dx0, dw0 = _module_pass(hipconv, m, x, dy)
    assert today == {"forward": "wino_s2", "input_grad": "wino_s2", "weight_grad": "wino_s2"}, today
    # "direct_bf16x3_s2": the weight gradient's engine and bits are today's
    hipconv.set_conv_math(fp32="direct_bf16x3_s2")
    mid, _, _, dw_mid = _module_pass(hipconv, m, x, dy)
    assert mid == {"forward": "bf16x3d", "input_grad": "bf16x3d", "weight_grad": "wino_s2"} and _same(dw_mid, dw0), mid
    hipconv.set_conv_math(fp32="direct_bf16x3_s2_dw")
    seen, y, dx, dw = _module_pass(hipconv, m, x, dy)
    assert seen == {"forward": "bf16x3d", "input_grad": "bf16x3d", "weight_grad": "bf16x3w"}, seen
    # fp64 autograd
    f = (lambda a, ww: F.conv_transpose2d(a, ww, None, 2, 1)) if tr else (lambda a, ww: F.conv2d(a, ww, None, 2, 1))
    xd, wd = x.double().requires_grad_(True), m.weight.detach().double().requires_grad_(True)
    y64 = f(xd, wd)
    dx64, dw64 = torch.autograd.grad(y64, (xd, wd), dy.double())
    y64 = y64.detach()
    wa = m.weight.detach().abs().double()
    g_fwd, g_bwd = (F.conv_transpose2d, F.conv2d) if tr else (F.conv2d, F.conv_transpose2d)
    _in_band("module forward", y, y64, 2.0 ** -16 * g_fwd(x.abs().double(), wa, None, 2, 1) + 1e-5 * y64.abs().max())
    _in_band("module input gradient", dx, dx64, 2.0 ** -16 * g_bwd(dy.abs().double(), wa, None, 2, 1) + 1e-5 * dx64.abs().max())
    fine, coarse = (dy, x) if tr else (x, dy)
    _in_band("module weight gradient", dw, dw64, _band(fine, coarse, dw64))
    # back on the default: the engines of today, the bits of today
    hipconv.set_conv_math(fp32="fp32")
    again, y1, dx1, dw1 = _module_pass(hipconv, m, x, dy)
    assert again == today and _same(y1, y0) and _same(dx1, dx0) and _same(dw1, dw0)
