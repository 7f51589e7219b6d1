"""The direct 3x3 convolution on fp32 tensors with split-bf16 operands (io code 2 of ipsr_conv3x3_bf16, ops.conv3x3_bf16x3, engine
"bf16x3d") against fp64 on the GPU.

The error band is derived, not measured.  For fp32 a: hi = RNE-bf16(a) leaves |a - hi| <= 2^-9 |a|, lo = RNE-bf16(a - hi) leaves
|a - hi - lo| <= 2^-18 |a|; bf16 x bf16 is exact in fp32.  The kernel adds lo*hi + hi*lo + hi*hi, so a product is off by lo*lo and
the two residual terms: <= 3 * 2^-18 |a||b| < 2^-16 |a||b|.  Per output element therefore

    |y - y64| <= 2^-16 * (|x| * |w|) + 1e-5 * max|y64|

with y64 the fp64 convolution of the UNROUNDED operands, (|x| * |w|) the same convolution of the absolute values, and the second
term the fp32-accumulation band tests/test_gpu_bf16_conv_variants.py holds this kernel family to.  Operands: normal draws times a
per-channel power of two in 2^-6 .. 2^6 (not bf16-representable, wide range, far from subnormals).  Dropping a cross term lands
~100x outside the band, hi*hi alone ~200x.

Shapes (B, Cin, Cout, H, W), each for the four ops (Conv2d forward / input gradient, ConvTranspose2d forward / input gradient):
    one_stage    (2, 16, 48, 16, 16)   one stage, one tile, produced channels no multiple of the 64-row k tile
    wrap         (3, 48, 80, 32, 16)   three stages (the A buffers wrap), two k tiles, two pixel tiles per image (halo rows cross tiles)
    row_tiles    (2, 64, 64, 2, 256)   one image row per tile (W = 256: the largest T image)
    three_tiles  (2, 32, 64, 12, 64)   three tiles per image: the tile -> (image, row) split is a real division
    cut          (1, 128, 128, 16, 16) two workgroups, eight channel blocks: the reduction is cut into two runs + the ordered add
"""
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

import bf16_conv_plan as P
from bf16x3_harness import NAN_BITS, _bits, _in_band, _module_pass, _same, check_bf16_representable, check_guarded, direct_math, draw  # noqa: F401

pytestmark = pytest.mark.gpu

IPSR_ERR_INVALID, IPSR_ERR_UNSUPPORTED, IPSR_ERR_WORKSPACE = -1, -2, -3
F32 = torch.float32

SHAPES = {
    "one_stage": (2, 16, 48, 16, 16),
    "wrap": (3, 48, 80, 32, 16),
    "row_tiles": (2, 64, 64, 2, 256),
    "three_tiles": (2, 32, 64, 12, 64),
    "cut": (1, 128, 128, 16, 16),
}


def x3_plan(op, B, Cin, H, W, Cout):
    """The launch plan of csrc/conv_bf16.hip's data_geometry on DATA_K3_SPLIT, restated (tests/bf16_conv_plan.py): None where it refuses."""
    C, K = (Cin, Cout) if op in (0, 2) else (Cout, Cin)
    p = P.split_plan("k3_split", "S1", B, C, K, H, W)
    return p and {k: p[k] for k in ("nsplit", "sps", "ktiles", "tiles_per_img", "nstage", "ws")}


def _operands(op, B, Cin, Cout, H, W, seed):
    """(input of the op, weight in the module's layout): normal draws times a per-channel power of two in 2^-6 .. 2^6."""
    g = torch.Generator(device="cuda").manual_seed(seed)
    cin_op = Cin if op in (0, 2) else Cout
    wshape = (Cout, Cin, 3, 3) if op < 2 else (Cin, Cout, 3, 3)
    return draw(g, (B, cin_op, H, W), 1), draw(g, wshape, 0)


def _ref64(op, x, w):
    """fp64: Conv2d forward (0) and ConvTranspose2d input gradient (3) are convolutions, the other two transposed convolutions."""
    f = F.conv2d if op in (0, 3) else F.conv_transpose2d
    return f(x.double(), w.double(), None, 1, 1)


def _band(op, x, w, y64):
    return 2.0 ** -16 * _ref64(op, x.abs(), w.abs()) + 1e-5 * y64.abs().max()


@pytest.mark.parametrize("sid", list(SHAPES))
def test_split_bf16_direct_conv(sid, monkeypatch):
    from deepinpainting_amd import _lib, ops
    L = _lib.lib()
    B, Cin, Cout, H, W = SHAPES[sid]
    for op in range(4):
        plan = x3_plan(op, B, Cin, H, W, Cout)
        assert plan is not None and L.ipsr_conv3x3_bf16x3_workspace_bytes(op, B, Cin, H, W, Cout) == plan["ws"], (sid, op, plan)
        if sid == "cut":
            assert plan["nsplit"] == 2, plan
        x, w = _operands(op, B, Cin, Cout, H, W, 41 + op)
        y64 = _ref64(op, x, w)
        run = lambda a, ww: ops.conv3x3_bf16x3(op, a, ww, (a.shape[0], Cin, H, W), Cout)
        y = run(x, w)
        torch.cuda.synchronize()
        assert y.dtype == F32 and y.shape == y64.shape
        _in_band("%s op %d" % (sid, op), y, y64, _band(op, x, w, y64))
        # a second call: the same bits
        assert _same(run(x, w), y), "%s op %d: two calls differ" % (sid, op)
        # the kept packed planes (pack_valid = 1 from the second call on): the same bits, one packing launch
        n0 = ops.bf16_pack_launches
        k1 = ops.conv3x3_bf16x3(op, x, w, (B, Cin, H, W), Cout, keep_packed=True)
        k2 = ops.conv3x3_bf16x3(op, x, w, (B, Cin, H, W), Cout, keep_packed=True)
        assert ops.bf16_pack_launches == n0 + 1
        assert _same(k1, y) and _same(k2, y), "%s op %d: the kept packed weights give other bits" % (sid, op)
        # every image alone: the same bits where the reduction is cut the same way
        if B >= 2:
            one = x3_plan(op, 1, Cin, H, W, Cout)
            for b in range(B):
                yb = run(x[b:b + 1].contiguous(), w)
                _in_band("%s op %d image %d" % (sid, op, b), yb, y64[b:b + 1], _band(op, x, w, y64)[b:b + 1])
                if (one["nsplit"], one["sps"]) == (plan["nsplit"], plan["sps"]):
                    assert _same(yb, y[b:b + 1]), "%s op %d: image %d alone differs from the batch" % (sid, op, b)
        check_guarded(monkeypatch, run, (x, w), ("x", "w"), y, plan["ws"], "%s op %d" % (sid, op))
        check_bf16_representable(run, lambda a, ww: _ref64(op, a, ww), (x, w), "%s op %d" % (sid, op))


def _nan_fill(t):
    _bits(t).fill_(NAN_BITS)
    return t


@pytest.mark.parametrize("what", ["w24", "c8", "io3", "ws_short"])
def test_refusals_write_nothing(what):
    from deepinpainting_amd import _lib, ops
    L = _lib.lib()
    op, B, Cin, H, W, Cout, io = {"w24": (0, 1, 16, 12, 24, 16, 2), "c8": (0, 1, 8, 16, 16, 16, 2), "io3": (0, 1, 16, 16, 16, 16, 3),
                                  "ws_short": (0, 1, 16, 16, 16, 16, 2)}[what]
    x = torch.zeros(B, Cin, H, W, device="cuda")
    w = torch.zeros(Cout, Cin, 3, 3, device="cuda")
    out = _nan_fill(torch.empty(B, Cout, H, W, device="cuda"))
    keep = out.clone()
    ws = torch.empty(1 << 20, dtype=torch.uint8, device="cuda")
    nbytes = ws.numel()
    want, msg = {"w24": (IPSR_ERR_UNSUPPORTED, "width 24"), "c8": (IPSR_ERR_UNSUPPORTED, "8 reduction channels are not a multiple of 16"),
                 "io3": (IPSR_ERR_INVALID, "io code 3"), "ws_short": (IPSR_ERR_WORKSPACE, "workspace")}[what]
    if what in ("w24", "c8"):
        assert x3_plan(op, B, Cin, H, W, Cout) is None and not ops.conv3x3_bf16x3_supported(op, B, Cin, H, W, Cout)
        assert msg in L.ipsr_last_error().decode("utf-8", "replace")
        with pytest.raises(NotImplementedError):
            ops.conv3x3_bf16x3(op, x, w, (B, Cin, H, W), Cout)
    if what == "ws_short":
        nbytes = L.ipsr_conv3x3_bf16x3_workspace_bytes(op, B, Cin, H, W, Cout) - 1
        assert nbytes > 0
    torch.cuda.synchronize()
    for entry, extra in (("ipsr_conv3x3_bf16", ()), ("ipsr_conv3x3_bf16_packed", (0,))):
        rc = getattr(L, entry)(op, x.data_ptr(), w.data_ptr(), out.data_ptr(), B, Cin, H, W, Cout, io, *extra, ws.data_ptr(), nbytes, ops._stream())
        text = L.ipsr_last_error().decode("utf-8", "replace")
        torch.cuda.synchronize()
        assert rc == want and msg in text, (entry, rc, text)
        assert _same(out, keep), "the output was written by a refused call"


# ---- through the modules ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mk", [lambda: nn.Conv2d(64, 64, 3, padding=1), lambda: nn.ConvTranspose2d(128, 64, 3, padding=1)], ids=["conv64", "convT128_64"])
def test_modules_run_the_engine_when_asked(mk, direct_math):
    hipconv = direct_math
    torch.manual_seed(7)
    m = mk().cuda()
    tr = isinstance(m, nn.ConvTranspose2d)
    g = torch.Generator(device="cuda").manual_seed(11)
    x = torch.randn(2, m.in_channels, 32, 32, device="cuda", generator=g)
    dy = torch.randn(2, m.out_channels, 32, 32, device="cuda", generator=g)
    assert hipconv._MATH["fp32"] == "fp32"
    today, y0, dx0, _ = _module_pass(hipconv, m, x, dy)
    assert today["forward"] == "winograd" and today["input_grad"] == "winograd", today
    hipconv.set_conv_math(fp32="direct_bf16x3")
    seen, y, dx, dw = _module_pass(hipconv, m, x, dy)
    assert seen["forward"] == "bf16x3d" and seen["input_grad"] == "bf16x3d" and seen["weight_grad"] == today["weight_grad"], (seen, today)
    # fp64 autograd
    f = (lambda a, ww: F.conv_transpose2d(a, ww, None, 1, 1)) if tr else (lambda a, ww: F.conv2d(a, ww, None, 1, 1))
    xd, wd = x.double().requires_grad_(True), m.weight.detach().double().requires_grad_(True)
    y64 = f(xd, wd)
    dx64, dw64 = torch.autograd.grad(y64, (xd, wd), dy.double())
    y64 = y64.detach()
    fop, bop = (2, 3) if tr else (0, 1)
    wt = m.weight.detach()
    _in_band("module forward", y, y64, _band(fop, x, wt, y64))
    _in_band("module input gradient", dx, dx64, _band(bop, dy, wt, dx64))
    # the weight gradient stays on today's engine and arithmetic: today's 1e-4 band of the fp32 engines (tests/test_gpu_conv.py)
    e = float((dw.double() - dw64).abs().max() / dw64.abs().max())
    print("module weight gradient on %r: %.2e of its scale" % (seen["weight_grad"], e))
    assert e <= 1e-4
    # back on the default: the engines of today, the bits of today
    hipconv.set_conv_math(fp32="fp32")
    again, y1, dx1, _ = _module_pass(hipconv, m, x, dy)
    assert again == today and _same(y1, y0) and _same(dx1, dx0)
