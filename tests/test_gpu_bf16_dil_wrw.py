"""The weight gradient of the dilated layer Conv2d(k4, stride 2, pad 3, dilation 2) on bf16 tensors (ipsr_conv4x4s2_bf16_dil_wrw,
ops.conv4x4s2_bf16_dil_wrw, engine "bf16d", opt-in `hipconv.set_direct_dilated_bf16_dw(True)`) against fp64 on the GPU.

Reference: the fp64 autograd weight gradient of F.conv2d(fine.double(), w, None, 2, 3, 2) on the bf16 operands as they are.  Bound, every
case: max |dW - dW64| <= 1e-5 * max |dW64| — the family's TOLW of tests/test_gpu_bf16_conv_variants.py: a product of two bf16 numbers is
exact in fp32, what is left is the fp32 accumulation of at most 2048 products per element and the ordered add of the runs' slabs.
The cases and the launch variant each one reaches are in tests/bf16_dil_wrw_plan.py (`CASES`, asserted against the restated planner).

Measured on MI355X, max |err| / max |dW64| per case: one 7.4e-08, wrap 1.3e-07, w32 1.1e-07, w64 1.1e-07, batch 1.1e-07, row1 7.6e-08,
w128 1.2e-07, cut 3.1e-07, w128ring 2.3e-07 (the 16 taps of `one`: 4.3e-08 .. 1.1e-07 of their own max); through the module 1.2e-07; in the
training step 1.3e-07 .. 2.8e-07.
"""
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

import bf16_dil_wrw_plan as X
from bf16x3_harness import NAN_BITS, _bits, _module_pass, _same, check_guarded, check_out_slice
from bf16x3_harness import direct_math  # noqa: F401  (fixture)

pytestmark = pytest.mark.gpu

IPSR_ERR_INVALID, IPSR_ERR_UNSUPPORTED, IPSR_ERR_WORKSPACE = -1, -2, -3
F32, BF16 = torch.float32, torch.bfloat16
TOLW = 1e-5
STEP_TOL = 1e-4        # in the training step: the in-situ band of the direct bf16 engines (tests/test_gpu_conv.py `_band`); reductions of up to
#                        32768 pixels, 16 times the unit cases', for which TOLW was set


def _operands(B, Kc, Cf, nh, nw, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    return torch.randn(B, Cf, 2 * nh, 2 * nw, device="cuda", generator=g).to(BF16), torch.randn(B, Kc, nh, nw, device="cuda", generator=g).to(BF16)


def _wrw64(fine, coarse):
    """fp64 autograd: the weight gradient [Kc][Cf][4][4] of Conv2d(Cf -> Kc, k4 s2 p3 d2) on `fine` for grad_output `coarse`."""
    w = torch.zeros(coarse.shape[1], fine.shape[1], 4, 4, dtype=torch.float64, device=fine.device, requires_grad=True)
    return torch.autograd.grad(F.conv2d(fine.double(), w, None, 2, 3, 2), w, coarse.double())[0]


def _err(tag, d, d64, scale_of=None):
    e = float((d.double() - d64).abs().max() / (d64 if scale_of is None else scale_of).abs().max())
    print("%s: max |err| / max |dW64| %.2e (bound %.0e)" % (tag, e, TOLW))
    return e


_REF = {}


def _case(cid):
    """(fine, coarse, dW64, dW of the first call) of a case, computed once and never written."""
    from deepinpainting_amd import ops
    if cid not in _REF:
        shape = X.CASES[cid][0]
        fine, coarse = _operands(*shape, 211 + len(cid))
        d = ops.conv4x4s2_bf16_dil_wrw(fine, coarse, *shape)
        torch.cuda.synchronize()
        _REF[cid] = (fine, coarse, _wrw64(fine, coarse), d)
    return _REF[cid]


def test_the_cases_reach_their_variants():
    X.check_cases()


@pytest.mark.parametrize("cid", list(X.CASES))
def test_bf16_dilated_weight_gradient(cid, monkeypatch):
    from deepinpainting_amd import _lib, ops
    L = _lib.lib()
    B, Kc, Cf, nh, nw = shape = X.CASES[cid][0]
    plan = X.plan(*shape)
    assert ops.conv4x4s2_bf16_dil_wrw_supported(*shape)
    assert L.ipsr_conv4x4s2_bf16_dil_wrw_workspace_bytes(*shape) == plan["ws"], (cid, plan)
    fine, coarse, d64, d = _case(cid)
    assert d.dtype == F32 and tuple(d.shape) == (Kc, Cf, 4, 4) and torch.isfinite(d).all()
    assert _err(cid, d, d64) <= TOLW
    # the taps that only ever meet rows outside the image are exact zeros
    if cid in ("row1", "w128"):
        dead = [(r, s) for r in range(4) for s in range(4) if not d64[:, :, r, s].any()]
        assert dead == [(r, s) for r in ((0, 1, 3) if cid == "row1" else (0,)) for s in range(4)], dead
        assert all(not d[:, :, r, s].any() for r, s in dead), "%s: a tap of rows outside the image is not zero" % cid
    # a second call: the same bits
    run = lambda f, c: ops.conv4x4s2_bf16_dil_wrw(f, c, *shape)
    assert _same(run(fine, coarse), d), "%s: two calls differ" % cid
    check_guarded(monkeypatch, run, (fine, coarse), ("fine", "coarse"), d, plan["ws"], cid)
    check_out_slice(lambda o: ops.conv4x4s2_bf16_dil_wrw(fine, coarse, *shape, out=o), d, cid)


def test_every_tap_is_inside_its_own_band():
    """A swapped row pair or column shift moves whole taps: each of the 16 taps within 1e-5 of its own tap's max."""
    shape = X.CASES["one"][0]
    fine, coarse, d64, d = _case("one")
    worst = [float((d[:, :, r, s].double() - d64[:, :, r, s]).abs().max() / d64[:, :, r, s].abs().max()) for r in range(4) for s in range(4)]
    print("one, per tap: max |err| / max |tap| " + " ".join("%.1e" % v for v in worst))
    assert max(worst) <= TOLW, worst


@pytest.mark.parametrize("cid", ["one", "wrap", "w64", "w128ring"])
def test_exact_on_small_integers(cid):
    """Operands of integers in -2 .. 2: every product and every partial sum is an integer of at most 4 * 2048, exact in fp32 in any order —
    dW equals the fp64 reference bit for bit after a cast."""
    from deepinpainting_amd import ops
    B, Kc, Cf, nh, nw = shape = X.CASES[cid][0]
    g = torch.Generator(device="cuda").manual_seed(5)
    fine = torch.randint(-2, 3, (B, Cf, 2 * nh, 2 * nw), device="cuda", generator=g).to(BF16)
    coarse = torch.randint(-2, 3, (B, Kc, nh, nw), device="cuda", generator=g).to(BF16)
    d = ops.conv4x4s2_bf16_dil_wrw(fine, coarse, *shape)
    d64 = _wrw64(fine, coarse)
    assert 0 < float(d64.abs().max()) <= 4 * 2048
    assert torch.equal(d.double(), d64), "%s: %d elements differ from the exact result" % (cid, int((d.double() != d64).sum()))


@pytest.mark.parametrize("cid", ["one", "w64", "w128"])
def test_only_the_odd_quarter_is_read(cid):
    """Only fine(odd, odd) enters the result: NaN / Inf in every even fine row and every even fine column change no bit of it."""
    from deepinpainting_amd import ops
    shape = X.CASES[cid][0]
    fine, coarse, _, d = _case(cid)
    dirty = fine.clone()
    dirty[:, :, 0::2, :] = float("nan")
    dirty[:, :, 1::2, 0::2] = float("inf")
    dirty[:, :, 1::4, 0::4] = float("-inf")
    assert torch.equal(dirty[:, :, 1::2, 1::2], fine[:, :, 1::2, 1::2]) and not torch.isfinite(dirty[:, :, 0::2]).any() \
        and not torch.isfinite(dirty[:, :, :, 0::2]).any()
    got = ops.conv4x4s2_bf16_dil_wrw(dirty, coarse, *shape)
    torch.cuda.synchronize()
    assert _same(got, d), "%s: an even fine row or column reached the result" % cid


def test_every_image_alone_sums_to_the_batch():
    from deepinpainting_amd import ops
    B, Kc, Cf, nh, nw = X.CASES["batch"][0]
    fine, coarse, d64, d = _case("batch")
    total = torch.zeros_like(d64)
    for b in range(B):
        total += ops.conv4x4s2_bf16_dil_wrw(fine[b:b + 1].contiguous(), coarse[b:b + 1].contiguous(), 1, Kc, Cf, nh, nw).double()
    assert _err("batch, the images alone summed in fp64", total, d64) <= TOLW
    assert float((total - d.double()).abs().max() / d64.abs().max()) <= TOLW


def test_wrong_dtype_and_shape_raise():
    from deepinpainting_amd import ops
    fine, coarse = torch.zeros(1, 16, 8, 32, device="cuda", dtype=BF16), torch.zeros(1, 16, 4, 16, device="cuda", dtype=BF16)
    with pytest.raises(TypeError):
        ops.conv4x4s2_bf16_dil_wrw(fine.float(), coarse, 1, 16, 16, 4, 16)
    with pytest.raises(TypeError):
        ops.conv4x4s2_bf16_dil_wrw(fine, coarse.float(), 1, 16, 16, 4, 16)
    with pytest.raises(RuntimeError):
        ops.conv4x4s2_bf16_dil_wrw(coarse, fine, 1, 16, 16, 4, 16)                          # (fine, coarse), in this order
    with pytest.raises(RuntimeError):
        ops.conv4x4s2_bf16_dil_wrw(fine, coarse, 1, 16, 16, 2, 32)
    with pytest.raises(RuntimeError):                                                       # `out` is fp32
        ops.conv4x4s2_bf16_dil_wrw(fine, coarse, 1, 16, 16, 4, 16, out=torch.empty(16, 16, 4, 4, device="cuda", dtype=BF16))


@pytest.mark.parametrize("what", ["w24", "w256", "nh6", "b0", "null_fine", "null_ws", "fine+8", "coarse+8", "dw+8", "ws+4", "ws_short"])
def test_refusals_write_nothing(what):
    from deepinpainting_amd import _lib, ops
    L = _lib.lib()
    B, Kc, Cf, nh, nw = shape = {"w24": (1, 16, 16, 4, 24), "w256": (1, 16, 16, 1, 256), "nh6": (1, 16, 16, 6, 16)}.get(what, (1, 16, 16, 4, 16))
    fine = torch.zeros(B, Cf, 2 * nh, 2 * nw, device="cuda", dtype=BF16)
    coarse = torch.zeros(B, Kc, nh, nw, device="cuda", dtype=BF16)
    dw = torch.empty(Kc * Cf * 16 + 4, device="cuda")
    _bits(dw).fill_(NAN_BITS)
    keep = dw.clone()
    ws = torch.empty(1 << 20, dtype=torch.uint8, device="cuda")
    nbytes = ws.numel()
    want, msg = {"w24": (IPSR_ERR_UNSUPPORTED, "width 24"), "w256": (IPSR_ERR_UNSUPPORTED, "width 256"), "nh6": (IPSR_ERR_UNSUPPORTED, "6 coarse rows"),
                 "b0": (IPSR_ERR_INVALID, "bad argument"), "null_fine": (IPSR_ERR_INVALID, "null pointer"), "null_ws": (IPSR_ERR_INVALID, "null pointer"),
                 "ws_short": (IPSR_ERR_WORKSPACE, "workspace")}.get(what, (IPSR_ERR_INVALID, "align"))
    if what == "ws_short":
        nbytes = L.ipsr_conv4x4s2_bf16_dil_wrw_workspace_bytes(*shape) - 1
        assert nbytes > 0
    if what in ("w24", "w256", "nh6"):
        assert X.plan(*shape) is None and not ops.conv4x4s2_bf16_dil_wrw_supported(*shape)
        assert msg in L.ipsr_last_error().decode("utf-8", "replace")
        with pytest.raises(NotImplementedError):
            ops.conv4x4s2_bf16_dil_wrw(fine, coarse, *shape, out=dw[:Kc * Cf * 16].view(Kc, Cf, 4, 4))
    ptr = {"fine": fine.data_ptr(), "coarse": coarse.data_ptr(), "dw": dw.data_ptr(), "ws": ws.data_ptr()}
    if "+" in what:
        ptr[what.split("+")[0]] += int(what.split("+")[1])
    if what.startswith("null_"):
        ptr[what[5:]] = None
    call_shape = (0,) + shape[1:] if what == "b0" else shape
    torch.cuda.synchronize()
    rc = L.ipsr_conv4x4s2_bf16_dil_wrw(ptr["fine"], ptr["coarse"], ptr["dw"], *call_shape, ptr["ws"], nbytes, ops._stream())
    text = L.ipsr_last_error().decode("utf-8", "replace")
    torch.cuda.synchronize()
    assert rc == want and msg in text, (rc, text)
    assert _same(dw, keep), "dW was written by a refused call"


# ---- through the modules ---------------------------------------------------------------------------------------------------------------
@pytest.fixture
def switch(direct_math):
    hipconv = direct_math
    assert hipconv.direct_dilated_bf16_dw() is False and hipconv.direct_dilated_bf16() is False
    yield hipconv
    hipconv.set_direct_dilated_bf16_dw(False)
    hipconv.set_direct_dilated_bf16(False)


def test_module_runs_the_engine_when_asked(switch):
    from deepinpainting_amd import ops
    hipconv = switch
    torch.manual_seed(7)
    m = nn.Conv2d(128, 128, 4, 2, 3, 2).cuda()
    g = torch.Generator(device="cuda").manual_seed(11)
    x = torch.randn(2, 128, 32, 32, device="cuda", generator=g).to(BF16)
    dy = torch.randn(2, 128, 16, 16, device="cuda", generator=g).to(BF16)
    amp = lambda: torch.autocast(device_type="cuda", dtype=BF16)          # as in the trainer
    with amp():
        today, y0, dx0, dw0 = _module_pass(hipconv, m, x, dy)
    assert today == {}, today                                       # 128 -> 128 @32 under bf16: all three passes are MIOpen's, the plain module call
    hipconv.set_direct_dilated_bf16_dw(True)
    with amp():
        seen, y, dx, dw = _module_pass(hipconv, m, x, dy)
    assert seen == {"forward": "miopen", "input_grad": "miopen", "weight_grad": "bf16d"}, seen
    assert dw.dtype == F32 and tuple(dw.shape) == (128, 128, 4, 4)
    d64 = _wrw64(x, dy)
    assert _err("module weight gradient", dw, d64) <= TOLW
    assert _same(dw, ops.conv4x4s2_bf16_dil_wrw(x, dy, 2, 128, 128, 16, 16))
    # weight.grad through backward(): the same bits
    m.weight.grad = None
    with amp():
        hipconv.conv_nobias(m, x.clone().requires_grad_(True)).backward(dy)
    torch.cuda.synchronize()
    assert _same(m.weight.grad, dw)
    m.weight.grad = None
    # both bf16 switches: each moves its own passes, the weight gradient keeps its bits
    hipconv.set_direct_dilated_bf16(True)
    with amp():
        both, _, _, dw2 = _module_pass(hipconv, m, x, dy)
    assert both == {"forward": "bf16d", "input_grad": "bf16d", "weight_grad": "bf16d"}, both
    assert _same(dw2, dw)
    # off again: the engines of before
    hipconv.set_direct_dilated_bf16(False)
    hipconv.set_direct_dilated_bf16_dw(False)
    with amp():
        again = _module_pass(hipconv, m, x, dy)[0]
    assert again == today


def test_training_step_with_the_option(tmp_path, switch):
    """Two training steps with opt.amp_bf16, opt.direct_dilated_bf16 and opt.direct_dilated_bf16_dw at 2 x 256x256, dropout on: the losses
    are finite, the weights of netG's dilated layers move, and every dilated weight gradient of the second step on maps of 32 .. 256 ran on
    "bf16d" and is held, on the tensors the step really produced (x cast to bf16, as the kernel reads it), to the fp64 reference within
    STEP_TOL of max |dW64|."""
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
    opt = Option(gpu_ids=[0], quiet=True, allow_random_vgg=True, checkpoints_dir=str(tmp_path), batchSize=B, use_dropout=True, amp_bf16=True,
                 direct_dilated_bf16=True, direct_dilated_bf16_dw=True)
    torch.manual_seed(5)
    with contextlib.redirect_stdout(io.StringIO()):
        m = create_model(opt)
    assert hipconv.direct_dilated_bf16() is True and hipconv.direct_dilated_bf16_dw() is True
    rows = ((64, 256), (128, 128), (256, 64), (512, 32))
    assert all(hipconv.select_wrw(False, B, C, H, H, C, 4, 2, 3, 2, True) == "bf16d" for C, H in rows)
    dilated = [mod for mod in m.netG.modules() if isinstance(mod, nn.Conv2d) and mod.kernel_size == (4, 4) and mod.dilation == (2, 2)]
    assert len(dilated) >= 4
    w0 = [mod.weight.detach().clone() for mod in dilated]
    seen = {}

    def hook(kind, engine, geom, operands, result):
        transposed, k, stride, pad, dil, Cout = geom
        if transposed or (k, stride, pad, dil) != (4, 2, 3, 2) or kind != "weight_grad":
            return
        dy, x = operands[0].detach(), operands[1].detach()
        if not 32 <= x.shape[2] <= 256:
            return
        with torch.enable_grad(), torch.autocast("cuda", enabled=False):            # the hook runs inside backward(); _wrw64 is fp64 autograd
            d64 = _wrw64(x.to(BF16), dy.to(BF16))
        worst = float((result.detach().double() - d64).abs().max() / d64.abs().max())
        seen.setdefault(tuple(x.shape), []).append((engine, str(result.dtype), worst))

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
        print("weight_grad %-20s %s" % (key, ", ".join("%s %s %.2e of max|dW64| (bound %.0e)" % (c + (STEP_TOL,)) for c in calls)))
    for C, H in rows:
        assert (B, C, H, H) in seen, "the step has no dilated weight gradient at %d@%d" % (C, H)
    assert all(eng == "bf16d" and dt == "torch.float32" and worst <= STEP_TOL for calls in seen.values() for eng, dt, worst in calls), seen
    losses = m.get_current_errors()
    assert losses and all(torch.isfinite(torch.as_tensor(float(v))) for v in losses.values()), losses
    assert all(not torch.equal(mod.weight.detach(), w) for mod, w in zip(dilated, w0)), "a dilated layer's weight did not move"
