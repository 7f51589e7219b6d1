"""The weight gradient of the dilated layer Conv2d(k4, stride 2, pad 3, dilation 2) on fp32 tensors with split-bf16 operands
(ipsr_conv4x4s2_bf16x3_dil_wrw, ops.conv4x4s2_bf16x3_dil_wrw, engine "bf16x3w", opt-in `hipconv.set_direct_dilated_dw(True)`) against fp64
on the GPU.

The error band is the family's, derived in tests/test_gpu_bf16x3_s2_wrw.py: a product lo*hi + hi*lo + hi*hi is off by lo*lo and the two
split residuals, <= 3 * 2^-18 |a||b| < 2^-16 |a||b|, so per element of dW

    |dW - dW64| <= 2^-16 * wrw64(|fine|, |coarse|) + 1e-5 * max|dW64|

with dW64 the fp64 autograd weight gradient of F.conv2d(x, w, None, 2, 3, 2) on the UNROUNDED operands, wrw64(|fine|, |coarse|) the same
reduction of the absolute values and the second term the fp32-accumulation floor of the sibling tests.  Operands: normal draws times a
per-channel power of two in 2^-6 .. 2^6.  Every case reduces B * nh * nw <= 2048 coarse pixels; emulated on the CPU in fp64 on the first
eight shapes (other draws), the full three-term arithmetic lands at 0.027 .. 0.155 of the band and either cross term dropped 10-42x outside it.

The cases and the launch variant each one reaches are in tests/bf16x3_dil_wrw_plan.py (`CASES`, asserted against the restated planner).

Measured on MI355X, worst |err| / band per case: one 0.121, wrap 0.069, w32 0.090, w64 0.082, batch 0.075, row1 0.072, w128 0.080, cut 0.031,
w128ring 0.042 (the 16 taps of `one`: 0.057 .. 0.151 of their own bands); bf16-representable operands 3.6e-08 .. 2.0e-07 of the scale; through
the module 0.081; in the training step 5.0e-06 .. 7.7e-06 of max|dW64| (0.020 .. 0.301 of the derived band).
"""
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

import bf16x3_dil_wrw_plan as X
from bf16x3_harness import NAN_BITS, _bits, _module_pass, _same, check_bf16_representable, check_guarded, check_out_slice, draw
from bf16x3_harness import _in_band as _in_band_of
from bf16x3_harness import direct_math  # noqa: F401  (fixture)

pytestmark = pytest.mark.gpu

IPSR_ERR_INVALID, IPSR_ERR_UNSUPPORTED, IPSR_ERR_WORKSPACE = -1, -2, -3
F32, BF16 = torch.float32, torch.bfloat16


def _operands(B, Kc, Cf, nh, nw, seed):
    """(fine, coarse): normal draws times a per-channel power of two in 2^-6 .. 2^6."""
    g = torch.Generator(device="cuda").manual_seed(seed)
    return draw(g, (B, Cf, 2 * nh, 2 * nw), 1), draw(g, (B, Kc, nh, nw), 1)


def _wrw64(fine, coarse):
    """fp64 autograd: the weight gradient [Kc][Cf][4][4] of Conv2d(Cf -> Kc, k4 s2 p3 d2) on `fine` for grad_output `coarse`."""
    w = torch.zeros(coarse.shape[1], fine.shape[1], 4, 4, dtype=torch.float64, device=fine.device, requires_grad=True)
    return torch.autograd.grad(F.conv2d(fine.double(), w, None, 2, 3, 2), w, coarse.double())[0]


def _band(fine, coarse, d64):
    return 2.0 ** -16 * _wrw64(fine.abs(), coarse.abs()) + 1e-5 * d64.abs().max()


def _in_band(tag, d, d64, band):
    _in_band_of(tag, d, d64, band, ref="dW64")


_REF = {}


def _case(cid):
    """(fine, coarse, dW64, band) of a case, computed once and never written."""
    if cid not in _REF:
        B, Kc, Cf, nh, nw = X.CASES[cid][0]
        fine, coarse = _operands(B, Kc, Cf, nh, nw, 211 + len(cid))
        d64 = _wrw64(fine, coarse)
        _REF[cid] = (fine, coarse, d64, _band(fine, coarse, d64))
    return _REF[cid]


@pytest.fixture
def switch(direct_math):
    hipconv = direct_math
    assert hipconv.direct_dilated_dw() is False and hipconv.direct_dilated() is False
    yield hipconv
    hipconv.set_direct_dilated_dw(False)
    hipconv.set_direct_dilated(False)


def test_the_cases_reach_their_variants():
    X.check_cases()


@pytest.mark.parametrize("cid", list(X.CASES))
def test_split_bf16_dilated_weight_gradient(cid, monkeypatch):
    from deepinpainting_amd import _lib, ops
    L = _lib.lib()
    B, Kc, Cf, nh, nw = shape = X.CASES[cid][0]
    plan = X.plan(*shape)
    assert ops.conv4x4s2_bf16x3_dil_wrw_supported(*shape)
    assert L.ipsr_conv4x4s2_bf16x3_dil_wrw_workspace_bytes(*shape) == plan["ws"], (cid, plan)
    fine, coarse, d64, band = _case(cid)
    d = ops.conv4x4s2_bf16x3_dil_wrw(fine, coarse, *shape)
    torch.cuda.synchronize()
    assert d.dtype == F32 and tuple(d.shape) == (Kc, Cf, 4, 4)
    _in_band(cid, d, d64, band)
    # the taps that only ever meet rows outside the image are exact zeros
    if cid == "row1":
        assert int((d64[:, :, [0, 1, 3]] == 0).sum()) == 6144 and not d[:, :, [0, 1, 3]].any()
    if cid == "w128":
        assert int((d64[:, :, 0] == 0).sum()) == 8192 and not d[:, :, 0].any()
    # a second call: the same bits
    assert _same(ops.conv4x4s2_bf16x3_dil_wrw(fine, coarse, *shape), d), "%s: two calls differ" % cid
    run = lambda f, c: ops.conv4x4s2_bf16x3_dil_wrw(f, c, *shape)
    check_guarded(monkeypatch, run, (fine, coarse), ("fine", "coarse"), d, plan["ws"], cid)
    check_out_slice(lambda o: ops.conv4x4s2_bf16x3_dil_wrw(fine, coarse, *shape, out=o), d, cid)
    check_bf16_representable(run, _wrw64, (fine, coarse), cid, scale="the scale")


def test_every_tap_is_inside_its_own_band():
    """A swapped row pair or column shift moves whole taps: each of the 16 taps against a band of its own scale."""
    from deepinpainting_amd import ops
    shape = X.CASES["one"][0]
    fine, coarse, d64, _ = _case("one")
    d = ops.conv4x4s2_bf16x3_dil_wrw(fine, coarse, *shape)
    torch.cuda.synchronize()
    prod = 2.0 ** -16 * _wrw64(fine.abs(), coarse.abs())
    worst = []
    for r in range(4):
        for s in range(4):
            band = prod[:, :, r, s] + 1e-5 * d64[:, :, r, s].abs().max()
            worst.append(float(((d[:, :, r, s].double() - d64[:, :, r, s]).abs() / band).max()))
    print("one, per tap: max |err| / band " + " ".join("%.3f" % v for v in worst))
    assert max(worst) <= 1.0, worst


@pytest.mark.parametrize("cid", ["one", "w32", "w128"])
def test_even_rows_and_columns_are_never_read(cid):
    """Only fine(odd, odd) enters the result: NaN bits in every even fine row and every even fine column change no bit of it."""
    from deepinpainting_amd import ops
    shape = X.CASES[cid][0]
    fine, coarse, _, _ = _case(cid)
    d = ops.conv4x4s2_bf16x3_dil_wrw(fine, coarse, *shape)
    dirty = fine.clone()
    _bits(dirty)[:, :, 0::2, :] = NAN_BITS
    _bits(dirty)[:, :, :, 0::2] = NAN_BITS
    assert _same(dirty[:, :, 1::2, 1::2], fine[:, :, 1::2, 1::2]) and not torch.isfinite(dirty[:, :, 0::2]).any()
    got = ops.conv4x4s2_bf16x3_dil_wrw(dirty, coarse, *shape)
    torch.cuda.synchronize()
    assert _same(got, d), "%s: an even fine row or column reached the result" % cid


def test_wrong_dtype_is_refused():
    from deepinpainting_amd import ops
    fine, coarse = torch.zeros(1, 16, 8, 32, device="cuda"), torch.zeros(1, 16, 4, 16, device="cuda")
    with pytest.raises(TypeError):
        ops.conv4x4s2_bf16x3_dil_wrw(fine.to(BF16), coarse, 1, 16, 16, 4, 16)
    with pytest.raises(TypeError):
        ops.conv4x4s2_bf16x3_dil_wrw(fine, coarse.to(BF16), 1, 16, 16, 4, 16)


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
        nbytes = L.ipsr_conv4x4s2_bf16x3_dil_wrw_workspace_bytes(*shape) - 1
        assert nbytes > 0
    else:
        assert X.plan(*shape) is None and not ops.conv4x4s2_bf16x3_dil_wrw_supported(*shape)
        assert msg in L.ipsr_last_error().decode("utf-8", "replace")
        with pytest.raises(NotImplementedError):
            ops.conv4x4s2_bf16x3_dil_wrw(fine, coarse, *shape)
    torch.cuda.synchronize()
    rc = L.ipsr_conv4x4s2_bf16x3_dil_wrw(fine.data_ptr(), coarse.data_ptr(), dw.data_ptr(), *shape, ws.data_ptr(), nbytes, ops._stream())
    text = L.ipsr_last_error().decode("utf-8", "replace")
    torch.cuda.synchronize()
    assert rc == want and msg in text, (rc, text)
    assert _same(dw, keep), "dW was written by a refused call"


# ---- through the modules ---------------------------------------------------------------------------------------------------------------
def test_module_runs_the_engine_when_asked(switch):
    hipconv = switch
    torch.manual_seed(7)
    m = nn.Conv2d(128, 128, 4, 2, 3, 2).cuda()
    g = torch.Generator(device="cuda").manual_seed(11)
    x = torch.randn(2, 128, 32, 32, device="cuda", generator=g)
    dy = torch.randn(2, 128, 16, 16, device="cuda", generator=g)
    assert hipconv._MATH["fp32"] == "fp32"
    today, y0, dx0, dw0 = _module_pass(hipconv, m, x, dy)
    assert today == {"forward": "wino_dil", "input_grad": "wino_dil", "weight_grad": "wino_dil"}, today
    xd, wd = x.double().requires_grad_(True), m.weight.detach().double().requires_grad_(True)
    dw64 = torch.autograd.grad(F.conv2d(xd, wd, None, 2, 3, 2), wd, dy.double())[0]
    # only the new switch: the data passes keep today's engine and bits, the weight gradient moves
    hipconv.set_direct_dilated_dw(True)
    seen, y, dx, dw = _module_pass(hipconv, m, x, dy)
    assert seen == {"forward": "wino_dil", "input_grad": "wino_dil", "weight_grad": "bf16x3w"}, seen
    assert _same(y, y0) and _same(dx, dx0)
    _in_band("module weight gradient", dw, dw64, _band(x, dy, dw64))
    # both switches
    hipconv.set_direct_dilated(True)
    both, _, _, dw2 = _module_pass(hipconv, m, x, dy)
    assert both == {"forward": "bf16x3d", "input_grad": "bf16x3d", "weight_grad": "bf16x3w"}, both
    assert _same(dw2, dw)
    # off again: the engines of today, the bits of today
    hipconv.set_direct_dilated(False)
    hipconv.set_direct_dilated_dw(False)
    again, y1, dx1, dw1 = _module_pass(hipconv, m, x, dy)
    assert again == today and _same(y1, y0) and _same(dx1, dx0) and _same(dw1, dw0)


def test_training_step_with_the_option(tmp_path, switch):
    """One training step (the second of two, on weights Adam has moved) with opt.direct_dilated=True and opt.direct_dilated_dw=True at
    2 x 256x256, dropout on — the in-situ check of tests/test_gpu_conv.py (`_check_hook`): every dilated weight gradient the rule moves ran
    on "bf16x3w" and is within 1e-4 of max|dW64| against fp64 on the tensors the step really produced (the project's in-situ band for fp32
    engines; the step's reductions reach 32768 pixels, beyond what the derived band was checked for — its ratio is printed); the losses are
    finite."""
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
    opt = Option(gpu_ids=[0], quiet=True, allow_random_vgg=True, checkpoints_dir=str(tmp_path), batchSize=B, use_dropout=True,
                 direct_dilated=True, direct_dilated_dw=True)
    torch.manual_seed(5)
    with contextlib.redirect_stdout(io.StringIO()):
        m = create_model(opt)
    assert hipconv.direct_dilated() is True and hipconv.direct_dilated_dw() is True
    moved = [(C, H) for C, H in ((64, 256), (128, 128), (256, 64), (512, 32)) if hipconv.select_wrw(False, B, C, H, H, C, 4, 2, 3, 2) == "bf16x3w"]
    assert (128, 128) in moved and (256, 64) in moved and (512, 32) in moved, moved
    seen = {}

    def hook(kind, engine, geom, operands, result):
        transposed, k, stride, pad, dil, Cout = geom
        if transposed or (k, stride, pad, dil) != (4, 2, 3, 2) or kind != "weight_grad" or result.dtype != F32:
            return
        dy, x = operands[0].detach(), operands[1].detach()
        if (x.shape[1], x.shape[2]) not in moved:
            return
        with torch.enable_grad():                           # the hook runs inside backward(); _wrw64 is fp64 autograd
            d64 = _wrw64(x, dy)
            band = _band(x, dy, d64)
        err = (result.detach().double() - d64).abs()
        rel = float(err.max() / d64.abs().max())
        worst = float((err / band).max())
        seen.setdefault(tuple(x.shape), []).append((engine, rel, worst))

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
        print("weight_grad %-20s %s" % (key, ", ".join("%s %.2e of max|dW64|, %.3f of the derived band" % c for c in calls)))
    for C, H in moved:
        assert (B, C, H, H) in seen, "the step has no dilated weight gradient at %d@%d" % (C, H)
    assert all(eng == "bf16x3w" and rel <= 1e-4 for calls in seen.values() for eng, rel, _ in calls), seen
    losses = m.get_current_errors()
    assert losses and all(torch.isfinite(torch.as_tensor(float(v))) for v in losses.values()), losses
