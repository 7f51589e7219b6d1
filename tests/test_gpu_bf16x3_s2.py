"""The direct split-bf16 kernel for the k4 s2 p1 layers on fp32 tensors (ipsr_conv4x4s2_bf16x3, ops.conv4x4s2_bf16x3, engine "bf16x3d"
under `set_conv_math(fp32="direct_bf16x3_s2")`) against fp64 on the GPU.

The error band is the one of tests/test_gpu_bf16x3_conv.py, derived there: a product lo*hi + hi*lo + hi*hi is off by lo*lo and the two
split residuals, <= 3 * 2^-18 |a||b| < 2^-16 |a||b|, so per output element

    |y - y64| <= 2^-16 * (|x| conv |w|) + 1e-5 * max|y64|

with y64 the fp64 convolution of the UNROUNDED operands (F.conv2d stride 2 pad 1 for fine -> coarse, F.conv_transpose2d for coarse ->
fine, the same [Kc,Cf,4,4] weight) and the second term the family's fp32-accumulation band.  Operands as there: normal draws times a
per-channel power of two in 2^-6 .. 2^6.  The cases and the plan variants they reach: tests/bf16x3_s2_plan.py.
"""
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

import bf16x3_s2_plan as S
from bf16x3_harness import NAN_BITS, _bits, _in_band, _module_pass, _same, check_bf16_representable, check_guarded, direct_math, draw  # noqa: F401

pytestmark = pytest.mark.gpu

IPSR_ERR_INVALID, IPSR_ERR_UNSUPPORTED, IPSR_ERR_WORKSPACE = -1, -2, -3
F32, BF16 = torch.float32, torch.bfloat16


def _operands(mode, B, Kc, Cf, nh, nw, seed):
    """(input of the pass, weight [Kc,Cf,4,4]): normal draws times a per-channel power of two in 2^-6 .. 2^6."""
    g = torch.Generator(device="cuda").manual_seed(seed)
    shape = (B, Cf, 2 * nh, 2 * nw) if mode == 0 else (B, Kc, nh, nw)
    return draw(g, shape, 1), draw(g, (Kc, Cf, 4, 4), 0)


def _ref64(mode, x, w):
    f = F.conv2d if mode == 0 else F.conv_transpose2d
    return f(x.double(), w.double(), None, 2, 1)


def _band(mode, x, w, y64):
    return 2.0 ** -16 * _ref64(mode, x.abs(), w.abs()) + 1e-5 * y64.abs().max()


@pytest.mark.parametrize("mode", [0, 1], ids=["fine_to_coarse", "coarse_to_fine"])
@pytest.mark.parametrize("cid", list(S.CASES))
def test_split_bf16_direct_s2(cid, mode, monkeypatch):
    from deepinpainting_amd import _lib, ops
    L = _lib.lib()
    B, Kc, Cf, nh, nw = S.CASES[cid][0]
    plan = S.plan(mode, B, Kc, Cf, nh, nw)
    assert plan is not None and L.ipsr_conv4x4s2_bf16x3_workspace_bytes(mode, B, Kc, Cf, nh, nw) == plan["ws"], (cid, mode, plan)
    if cid == "cut":
        assert plan["nsplit"] == 2, plan
    tag = "%s mode %d" % (cid, mode)
    x, w = _operands(mode, B, Kc, Cf, nh, nw, 53 + mode)
    y64 = _ref64(mode, x, w)
    band = _band(mode, x, w, y64)
    run = lambda a, ww: ops.conv4x4s2_bf16x3(mode, a, ww, a.shape[0], Kc, Cf, nh, nw)
    y = run(x, w)
    torch.cuda.synchronize()
    assert y.dtype == F32 and y.shape == y64.shape
    _in_band(tag, y, y64, band)
    # a second call: the same bits
    assert _same(run(x, w), y), "%s: two calls differ" % tag
    # every image alone: the same bits where the reduction is cut the same way, inside the band otherwise
    if B >= 2:
        one = S.plan(mode, 1, Kc, Cf, nh, nw)
        for b in range(B):
            yb = run(x[b:b + 1].contiguous(), w)
            _in_band("%s image %d" % (tag, b), yb, y64[b:b + 1], band[b:b + 1])
            if (one["nsplit"], one["sps"]) == (plan["nsplit"], plan["sps"]):
                assert _same(yb, y[b:b + 1]), "%s: image %d alone differs from the batch" % (tag, b)
    check_guarded(monkeypatch, run, (x, w), ("x", "w"), y, plan["ws"], tag)
    check_bf16_representable(run, lambda a, ww: _ref64(mode, a, ww), (x, w), tag)


def _nan_fill(t):
    _bits(t).fill_(NAN_BITS)
    return t


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("what", ["w24", "c8", "rows", "mode2", "ws_short"])
def test_refusals_write_nothing(what, mode):
    from deepinpainting_amd import _lib, ops
    L = _lib.lib()
    B, Kc, Cf, nh, nw = {"w24": (1, 16, 16, 12, 24), "c8": (1, 8, 8, 16, 16), "rows": (1, 16, 16, 12, 16), "mode2": (1, 16, 16, 16, 16),
                         "ws_short": (1, 16, 16, 16, 16)}[what]
    fine = torch.zeros(B, Cf, 2 * nh, 2 * nw, device="cuda")
    coarse = torch.zeros(B, Kc, nh, nw, device="cuda")
    inp, oshape = (fine, coarse.shape) if mode == 0 else (coarse, fine.shape)
    w = torch.zeros(Kc, Cf, 4, 4, device="cuda")
    out = _nan_fill(torch.empty(oshape, device="cuda"))
    keep = out.clone()
    ws = torch.empty(1 << 20, dtype=torch.uint8, device="cuda")
    nbytes = ws.numel()
    want, msg = {"w24": (IPSR_ERR_UNSUPPORTED, "coarse width 24"), "c8": (IPSR_ERR_UNSUPPORTED, "8 reduction channels are not a multiple of 16"),
                 "rows": (IPSR_ERR_UNSUPPORTED, "12 rows are not a multiple of the 16 rows of a tile"),
                 "mode2": (IPSR_ERR_INVALID, "mode 2"), "ws_short": (IPSR_ERR_WORKSPACE, "workspace")}[what]
    if what in ("w24", "c8", "rows"):
        assert S.plan(mode, B, Kc, Cf, nh, nw) is None and not ops.conv4x4s2_bf16x3_supported(mode, B, Kc, Cf, nh, nw)
        assert msg in L.ipsr_last_error().decode("utf-8", "replace")
        with pytest.raises(NotImplementedError):
            ops.conv4x4s2_bf16x3(mode, inp, w, B, Kc, Cf, nh, nw)
    if what == "ws_short":
        nbytes = L.ipsr_conv4x4s2_bf16x3_workspace_bytes(mode, B, Kc, Cf, nh, nw) - 1
        assert nbytes > 0
    if what == "mode2":
        assert not ops.conv4x4s2_bf16x3_supported(2, B, Kc, Cf, nh, nw)
        with pytest.raises(ValueError):
            ops.conv4x4s2_bf16x3(2, inp, w, B, Kc, Cf, nh, nw)
    torch.cuda.synchronize()
    rc = L.ipsr_conv4x4s2_bf16x3(2 if what == "mode2" else mode, inp.data_ptr(), w.data_ptr(), out.data_ptr(), B, Kc, Cf, nh, nw, ws.data_ptr(), nbytes, ops._stream())
    text = L.ipsr_last_error().decode("utf-8", "replace")
    torch.cuda.synchronize()
    assert rc == want and msg in text, (rc, text)
    assert _same(out, keep), "the output was written by a refused call"


def test_wrong_dtype_and_shape_raise():
    from deepinpainting_amd import ops
    x = torch.zeros(1, 16, 32, 32, device="cuda")
    w = torch.zeros(16, 16, 4, 4, device="cuda")
    with pytest.raises(TypeError):
        ops.conv4x4s2_bf16x3(0, x.to(BF16), w, 1, 16, 16, 16, 16)
    with pytest.raises(RuntimeError):
        ops.conv4x4s2_bf16x3(1, x, w, 1, 16, 16, 16, 16)           # mode 1 reads the coarse tensor


# ---- through the modules ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mk", [lambda: nn.Conv2d(64, 128, 4, 2, 1), lambda: nn.ConvTranspose2d(128, 64, 4, 2, 1)], ids=["conv64_128", "convT128_64"])
def test_modules_run_the_engine_when_asked(mk, direct_math):
    hipconv = direct_math
    torch.manual_seed(7)
    m = mk().cuda()
    tr = isinstance(m, nn.ConvTranspose2d)
    g = torch.Generator(device="cuda").manual_seed(11)
    hin, hout = (32, 64) if tr else (64, 32)                     # the coarse grid is 32 x 32 either way
    x = torch.randn(2, m.in_channels, hin, hin, device="cuda", generator=g)
    dy = torch.randn(2, m.out_channels, hout, hout, device="cuda", generator=g)
    assert hipconv._MATH["fp32"] == "fp32"
    today, y0, dx0, _ = _module_pass(hipconv, m, x, dy)
    assert today["forward"] == "wino_s2" and today["input_grad"] == "wino_s2", today
    hipconv.set_conv_math(fp32="direct_bf16x3_s2")
    seen, y, dx, dw = _module_pass(hipconv, m, x, dy)
    assert seen["forward"] == "bf16x3d" and seen["input_grad"] == "bf16x3d" and seen["weight_grad"] == today["weight_grad"], (seen, today)
    # fp64 autograd
    f = (lambda a, ww: F.conv_transpose2d(a, ww, None, 2, 1)) if tr else (lambda a, ww: F.conv2d(a, ww, None, 2, 1))
    xd, wd = x.double().requires_grad_(True), m.weight.detach().double().requires_grad_(True)
    y64 = f(xd, wd)
    dx64, dw64 = torch.autograd.grad(y64, (xd, wd), dy.double())
    y64 = y64.detach()
    # Conv2d [Cout,Cin] and ConvTranspose2d [Cin,Cout] are both [Kc,Cf]: the forward of one is the mode of the other's input gradient
    fmode, bmode = (1, 0) if tr else (0, 1)
    wt = m.weight.detach()
    _in_band("module forward", y, y64, _band(fmode, x, wt, y64))
    _in_band("module input gradient", dx, dx64, _band(bmode, dy, wt, dx64))
    # the weight gradient stays on today's engine and arithmetic: today's 1e-4 band of the fp32 engines (tests/test_gpu_conv.py)
    e = float((dw.double() - dw64).abs().max() / dw64.abs().max())
    print("module weight gradient on %r: %.2e of its scale" % (seen["weight_grad"], e))
    assert e <= 1e-4
    # back on the default: the engines of today, the bits of today
    hipconv.set_conv_math(fp32="fp32")
    again, y1, dx1, _ = _module_pass(hipconv, m, x, dy)
    assert again == today and _same(y1, y0) and _same(dx1, dx0)
