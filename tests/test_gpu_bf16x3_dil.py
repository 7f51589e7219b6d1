"""The direct split-bf16 kernel for the dilated down convolution Conv2d(k4, stride 2, pad 3, dilation 2) on fp32 tensors (modes 4 / 5 of
ipsr_conv4x4s2_bf16x3, ops.conv4x4s2_bf16x3 with ops.S2_DILATED, engine "bf16x3d" under `hipconv.set_direct_dilated(True)`) against fp64
on the GPU.

The error band is the family's, derived in tests/test_gpu_bf16x3_conv.py: a product lo*hi + hi*lo + hi*hi is off by lo*lo and the two
split residuals, <= 3 * 2^-18 |a||b| < 2^-16 |a||b|, so per output element

    |y - y64| <= 2^-16 * (|x| conv |w|) + 1e-5 * max|y64|

with y64 the fp64 result on the UNROUNDED operands: F.conv2d(x, w, None, 2, 3, 2) for fine -> coarse and
F.conv_transpose2d(dy, w, None, 2, 3, 1, 1, 2) for coarse -> fine (output padding 1: the fine map is even; equal to the autograd gradient),
the same [Kc,Cf,4,4] weight.  The zeros of the input gradient (even rows, even columns) have band 1e-5 max|y64| and must compare equal to 0.
Operands as there: normal draws times a per-channel power of two in 2^-6 .. 2^6.  The cases and the plan variants they reach:
tests/bf16x3_dil_plan.py.
"""
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

import bf16x3_dil_plan as D
from bf16x3_harness import NAN_BITS, _bits, _in_band, _module_pass, _same, check_bf16_representable, check_guarded, direct_math, draw  # noqa: F401

pytestmark = pytest.mark.gpu

IPSR_ERR_INVALID, IPSR_ERR_UNSUPPORTED, IPSR_ERR_WORKSPACE = -1, -2, -3
F32, BF16 = torch.float32, torch.bfloat16
MODES = pytest.mark.parametrize("mode", [4, 5], ids=["fine_to_coarse", "coarse_to_fine"])


def _operands(mode, B, Kc, Cf, nh, nw, seed):
    """(input of the pass, weight [Kc,Cf,4,4]): normal draws times a per-channel power of two in 2^-6 .. 2^6."""
    g = torch.Generator(device="cuda").manual_seed(seed)
    shape = (B, Cf, 2 * nh, 2 * nw) if mode == 4 else (B, Kc, nh, nw)
    return draw(g, shape, 1), draw(g, (Kc, Cf, 4, 4), 0)


def _ref64(mode, x, w):
    if mode == 4:
        return F.conv2d(x.double(), w.double(), None, 2, 3, 2)
    return F.conv_transpose2d(x.double(), w.double(), None, 2, 3, 1, 1, 2)


def _band(mode, x, w, y64):
    return 2.0 ** -16 * _ref64(mode, x.abs(), w.abs()) + 1e-5 * y64.abs().max()


@pytest.fixture
def switch(direct_math):
    hipconv = direct_math
    assert hipconv.direct_dilated() is False
    yield hipconv
    hipconv.set_direct_dilated(False)


@pytest.fixture(scope="module")
def first_results():
    """(cid, mode) -> (x, w, y64, band, y) of the first call of every case, computed once and never written."""
    from deepinpainting_amd import ops
    out = {}

    def get(cid, mode):
        if (cid, mode) not in out:
            B, Kc, Cf, nh, nw = D.CASES[cid][0]
            x, w = _operands(mode, B, Kc, Cf, nh, nw, 71 + mode)
            y64 = _ref64(mode, x, w)
            y = ops.conv4x4s2_bf16x3(mode, x, w, B, Kc, Cf, nh, nw)
            torch.cuda.synchronize()
            out[(cid, mode)] = (x, w, y64, _band(mode, x, w, y64), y)
        return out[(cid, mode)]
    return get


@MODES
@pytest.mark.parametrize("cid", list(D.CASES))
def test_split_bf16_direct_dilated(cid, mode, monkeypatch, first_results):
    from deepinpainting_amd import _lib, ops
    L = _lib.lib()
    B, Kc, Cf, nh, nw = D.CASES[cid][0]
    plan = D.plan(mode, B, Kc, Cf, nh, nw)
    assert plan is not None and L.ipsr_conv4x4s2_bf16x3_workspace_bytes(mode, B, Kc, Cf, nh, nw) == plan["ws"], (cid, mode, plan)
    if cid == "cut":
        assert plan["nsplit"] == 2, plan
    tag = "%s mode %d" % (cid, mode)
    x, w, y64, band, y = first_results(cid, mode)
    run = lambda a, ww: ops.conv4x4s2_bf16x3(mode, a, ww, a.shape[0], Kc, Cf, nh, nw)
    assert y.dtype == F32 and y.shape == y64.shape
    _in_band(tag, y, y64, band)
    if mode == 5:
        assert (y[:, :, 0::2, :] == 0).all() and (y[:, :, :, 0::2] == 0).all(), "%s: the even rows / columns of dx are not zero" % tag
    # a second call: the same bits
    assert _same(run(x, w), y), "%s: two calls differ" % tag
    # every image alone: the same bits where the reduction is cut the same way, inside the band otherwise
    if B >= 2:
        one = D.plan(mode, 1, Kc, Cf, nh, nw)
        for b in range(B):
            yb = run(x[b:b + 1].contiguous(), w)
            _in_band("%s image %d" % (tag, b), yb, y64[b:b + 1], band[b:b + 1])
            if (one["nsplit"], one["sps"]) == (plan["nsplit"], plan["sps"]):
                assert _same(yb, y[b:b + 1]), "%s: image %d alone differs from the batch" % (tag, b)
    check_guarded(monkeypatch, run, (x, w), ("x", "w"), y, plan["ws"], tag)
    check_bf16_representable(run, lambda a, ww: _ref64(mode, a, ww), (x, w), tag)


@pytest.mark.parametrize("cid", list(D.CASES))
def test_forward_reads_only_the_odd_quarter(cid, first_results):
    """Even rows and even columns of x never reach a product: NaN / Inf there, the same bits."""
    from deepinpainting_amd import ops
    B, Kc, Cf, nh, nw = D.CASES[cid][0]
    x, w, _, _, y = first_results(cid, 4)
    xp = x.clone()
    xp[:, :, 0::2, :] = float("nan")
    xp[:, :, 1::2, 0::2] = float("inf")
    xp[:, :, 1::4, 0::4] = float("-inf")
    assert _same(xp[:, :, 1::2, 1::2], x[:, :, 1::2, 1::2])
    got = ops.conv4x4s2_bf16x3(4, xp, w, B, Kc, Cf, nh, nw)
    torch.cuda.synchronize()
    assert _same(got, y), "%s: the even rows / columns of x changed the result" % cid


def _nan_fill(t):
    _bits(t).fill_(NAN_BITS)
    return t


@pytest.mark.parametrize("cid", list(D.CASES))
def test_input_gradient_writes_every_element(cid, first_results):
    """The raw entry on a NaN-filled `out` (ops allocates with torch.empty): no NaN left, zeros on the even rows and columns, the same bits."""
    from deepinpainting_amd import _lib, ops
    L = _lib.lib()
    B, Kc, Cf, nh, nw = D.CASES[cid][0]
    dy, w, _, _, dx = first_results(cid, 5)
    out = _nan_fill(torch.empty(B, Cf, 2 * nh, 2 * nw, device="cuda"))
    nbytes = D.plan(5, B, Kc, Cf, nh, nw)["ws"]
    ws = _nan_fill(torch.empty((nbytes + 3) // 4, device="cuda")).view(torch.uint8)
    torch.cuda.synchronize()
    rc = L.ipsr_conv4x4s2_bf16x3(5, dy.data_ptr(), w.data_ptr(), out.data_ptr(), B, Kc, Cf, nh, nw, ws.data_ptr(), nbytes, ops._stream())
    torch.cuda.synchronize()
    assert rc == 0, L.ipsr_last_error()
    assert not torch.isnan(out).any(), "%s: %d elements of dx were not written" % (cid, int(torch.isnan(out).sum()))
    assert (out[:, :, 0::2, :] == 0).all() and (out[:, :, :, 0::2] == 0).all()
    assert _same(out, dx)


@MODES
@pytest.mark.parametrize("what", ["w24", "c8", "rows", "mode2", "mode6", "ws_short"])
def test_refusals_write_nothing(what, mode):
    from deepinpainting_amd import _lib, ops
    L = _lib.lib()
    B, Kc, Cf, nh, nw = {"w24": (1, 16, 16, 12, 24), "c8": (1, 8, 8, 16, 16), "rows": (1, 16, 16, 12, 16)}.get(what, (1, 16, 16, 16, 16))
    fine = torch.zeros(B, Cf, 2 * nh, 2 * nw, device="cuda")
    coarse = torch.zeros(B, Kc, nh, nw, device="cuda")
    inp, oshape = (fine, coarse.shape) if mode == 4 else (coarse, fine.shape)
    w = torch.zeros(Kc, Cf, 4, 4, device="cuda")
    out = _nan_fill(torch.empty(oshape, device="cuda"))
    keep = out.clone()
    ws = torch.empty(1 << 20, dtype=torch.uint8, device="cuda")
    nbytes = ws.numel()
    want, msg = {"w24": (IPSR_ERR_UNSUPPORTED, "coarse width 24"), "c8": (IPSR_ERR_UNSUPPORTED, "8 reduction channels are not a multiple of 16"),
                 "rows": (IPSR_ERR_UNSUPPORTED, "12 rows are not a multiple of the 16 rows of a tile"),
                 "mode2": (IPSR_ERR_INVALID, "mode 2"), "mode6": (IPSR_ERR_INVALID, "mode 6"), "ws_short": (IPSR_ERR_WORKSPACE, "workspace")}[what]
    call_mode = {"mode2": 2, "mode6": 6}.get(what, mode)
    if what in ("w24", "c8", "rows"):
        assert D.plan(mode, B, Kc, Cf, nh, nw) is None and not ops.conv4x4s2_bf16x3_supported(mode, B, Kc, Cf, nh, nw)
        assert msg in L.ipsr_last_error().decode("utf-8", "replace")
        with pytest.raises(NotImplementedError):
            ops.conv4x4s2_bf16x3(mode, inp, w, B, Kc, Cf, nh, nw)
    if what == "ws_short":
        nbytes = L.ipsr_conv4x4s2_bf16x3_workspace_bytes(mode, B, Kc, Cf, nh, nw) - 1
        assert nbytes > 0
    if what in ("mode2", "mode6"):
        assert not ops.conv4x4s2_bf16x3_supported(call_mode, B, Kc, Cf, nh, nw)
        with pytest.raises(ValueError):
            ops.conv4x4s2_bf16x3(call_mode, inp, w, B, Kc, Cf, nh, nw)
    torch.cuda.synchronize()
    rc = L.ipsr_conv4x4s2_bf16x3(call_mode, inp.data_ptr(), w.data_ptr(), out.data_ptr(), B, Kc, Cf, nh, nw, ws.data_ptr(), nbytes, ops._stream())
    text = L.ipsr_last_error().decode("utf-8", "replace")
    torch.cuda.synchronize()
    assert rc == want and msg in text, (rc, text)
    assert _same(out, keep), "the output was written by a refused call"


def test_wrong_dtype_and_shape_raise():
    from deepinpainting_amd import ops
    x = torch.zeros(1, 16, 32, 32, device="cuda")
    w = torch.zeros(16, 16, 4, 4, device="cuda")
    with pytest.raises(TypeError):
        ops.conv4x4s2_bf16x3(4, x.to(BF16), w, 1, 16, 16, 16, 16)
    with pytest.raises(RuntimeError):
        ops.conv4x4s2_bf16x3(5, x, w, 1, 16, 16, 16, 16)           # mode 5 reads the coarse tensor
    with pytest.raises(RuntimeError):
        ops.conv4x4s2_bf16x3(4, x[:, :, :16, :16].contiguous(), w, 1, 16, 16, 16, 16)       # mode 4 reads the fine tensor
    with pytest.raises(ValueError):
        ops.conv4x4s2_bf16(4, x.to(BF16), w, 1, 16, 16, 16, 16)    # the bf16-tensor kernel has no dilated form


# ---- through the modules ---------------------------------------------------------------------------------------------------------------
def test_module_runs_the_engine_when_asked(switch):
    hipconv = switch
    torch.manual_seed(7)
    m = nn.Conv2d(64, 64, 4, 2, 3, 2).cuda()
    g = torch.Generator(device="cuda").manual_seed(11)
    x = torch.randn(2, 64, 64, 64, device="cuda", generator=g)
    dy = torch.randn(2, 64, 32, 32, device="cuda", generator=g)
    assert hipconv._MATH["fp32"] == "fp32"
    today, y0, dx0, _ = _module_pass(hipconv, m, x, dy)
    assert today["forward"] == "wino_dil" and today["input_grad"] == "wino_dil", today
    hipconv.set_direct_dilated(True)
    seen, y, dx, dw = _module_pass(hipconv, m, x, dy)
    assert seen["forward"] == "bf16x3d" and seen["input_grad"] == "bf16x3d" and seen["weight_grad"] == today["weight_grad"], (seen, today)
    # fp64 autograd
    xd, wd = x.double().requires_grad_(True), m.weight.detach().double().requires_grad_(True)
    y64 = F.conv2d(xd, wd, None, 2, 3, 2)
    dx64, dw64 = torch.autograd.grad(y64, (xd, wd), dy.double())
    y64 = y64.detach()
    wt = m.weight.detach()
    _in_band("module forward", y, y64, _band(4, x, wt, y64))
    _in_band("module input gradient", dx, dx64, _band(5, dy, wt, dx64))
    # the weight gradient stays on today's engine and arithmetic: today's 1e-4 band of the fp32 engines (tests/test_gpu_conv.py)
    e = float((dw.double() - dw64).abs().max() / dw64.abs().max())
    print("module weight gradient on %r: %.2e of its scale" % (seen["weight_grad"], e))
    assert e <= 1e-4
    # off again: the engines of today, the bits of today
    hipconv.set_direct_dilated(False)
    again, y1, dx1, _ = _module_pass(hipconv, m, x, dy)
    assert again == today and _same(y1, y0) and _same(dx1, dx0)


def test_training_step_with_the_option(tmp_path, switch):
    """One training step (the second of two, on weights Adam has moved) with opt.direct_dilated=True at 2 x 256x256, dropout on — the in-situ
    check of tests/test_gpu_conv.py (`_check_hook`) at the small batch of tests/test_gpu_model.py's trainer tests: every dilated data pass on
    maps of 32 .. 256 ran on "bf16x3d" and, on its two images, is inside the band against fp64 on the tensors the step really produced; the
    losses are finite.  At this batch the 512 @32 level runs with its reduction cut."""
    import contextlib
    import io
    from deepinpainting_amd.models.models import create_model
    from deepinpainting_amd.options import Option
    hipconv = switch
    g = torch.Generator(device="cuda").manual_seed(21)
    B, S, hole = 2, 256, 128
    img = torch.rand(B, 3, S, S, device="cuda", generator=g) * 2 - 1
    ref = torch.rand(B, 3, S, S, device="cuda", generator=g) * 2 - 1
    mask = torch.zeros(1, 1, S, S, dtype=torch.bool, device="cuda")
    mask[:, :, (S - hole) // 2:(S + hole) // 2, (S - hole) // 2:(S + hole) // 2] = 1
    opt = Option(gpu_ids=[0], quiet=True, allow_random_vgg=True, checkpoints_dir=str(tmp_path), batchSize=B, use_dropout=True, direct_dilated=True)
    torch.manual_seed(5)
    with contextlib.redirect_stdout(io.StringIO()):
        m = create_model(opt)
    assert hipconv.direct_dilated() is True
    assert D.plan(4, B, 512, 512, 16, 16)["nsplit"] > 1 and D.plan(5, B, 512, 512, 16, 16)["nsplit"] > 1
    seen = {}

    def hook(kind, engine, geom, operands, result):
        transposed, k, stride, pad, dil, Cout = geom
        if transposed or (k, stride, pad, dil) != (4, 2, 3, 2) or kind == "weight_grad" or result.dtype != F32:
            return
        x = operands[0] if kind == "forward" else operands[1]
        if not 32 <= x.shape[2] <= 256:
            return
        w = operands[-1].detach()
        with torch.no_grad():
            inp, mode = (x, 4) if kind == "forward" else (operands[0], 5)
            inp = inp.detach()[:2]
            y64 = _ref64(mode, inp, w)
            err = (result.detach()[:2].double() - y64).abs()
            worst = float((err / _band(mode, inp, w, y64)).max())
        seen.setdefault((kind, tuple(x.shape)), []).append((engine, worst))

    for step in range(2):
        hipconv._check_hook = hook if step == 1 else None
        try:
            m.set_input(img, mask, ref)
            m.set_ref_latent()
            m.set_gt_latent()
            m.optimize_parameters()
        finally:
            hipconv._check_hook = None
    torch.cuda.synchronize()
    for key, calls in sorted(seen.items()):
        print("%-10s %-20s %s" % (key[0], key[1], ", ".join("%s %.3f of the band" % c for c in calls)))
    for C, H in ((64, 256), (128, 128), (256, 64), (512, 32)):
        for kind in ("forward", "input_grad"):
            assert (kind, (B, C, H, H)) in seen, "the step has no dilated %s at %d@%d" % (kind, C, H)
    assert all(eng == "bf16x3d" and worst <= 1.0 for calls in seen.values() for eng, worst in calls), seen
    losses = m.get_current_errors()
    assert losses and all(torch.isfinite(torch.as_tensor(float(v))) for v in losses.values()), losses
