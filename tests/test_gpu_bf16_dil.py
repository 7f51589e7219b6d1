"""The direct bf16 kernel for the dilated down convolution Conv2d(k4, stride 2, pad 3, dilation 2) on bf16 tensors (ipsr_conv4x4s2_bf16_dil,
ops.conv4x4s2_bf16_dil, engine "bf16d" under `hipconv.set_direct_dilated_bf16(True)`) against fp64 on the GPU.

Reference: F.conv2d(x, w, None, 2, 3, 2) for fine -> coarse and F.conv_transpose2d(dy, w, None, 2, 3, 1, 1, 2) for coarse -> fine (output
padding 1: the fine map is even; equal to the autograd gradient), in fp64 on the operands the kernel multiplies: the bf16 input as it is, the
fp32 weight rounded to bf16.  Bounds: the family's (tests/test_gpu_bf16_conv_variants.py) — an fp32 output within 1e-5 of max |reference| (the
products are exact in fp32, what is left is the fp32 accumulation), a bf16 output within 2^-8 (half an ulp of bf16 is 2^-9 of the value).
The cases and the plan variants they reach: tests/bf16_dil_plan.py.
"""
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

import bf16_dil_plan as D
from bf16x3_harness import _module_pass, direct_math_deterministic  # noqa: F401  (the fixture `direct_math`)
from guarded import Arena

pytestmark = pytest.mark.gpu

IPSR_ERR_INVALID, IPSR_ERR_UNSUPPORTED, IPSR_ERR_WORKSPACE = -1, -2, -3
F32, BF16 = torch.float32, torch.bfloat16
TOL = {F32: 1e-5, BF16: 2.0 ** -8}
MODES = pytest.mark.parametrize("mode", [0, 1], ids=["fine_to_coarse", "coarse_to_fine"])
DTYPES = pytest.mark.parametrize("odt", [F32, BF16], ids=["fp32_out", "bf16_out"])
CIDS = pytest.mark.parametrize("cid", list(D.CASES))


def _bits(t):
    return t.contiguous().view({4: torch.int32, 2: torch.int16}[t.element_size()])


def _same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(_bits(a), _bits(b))


def _nan_fill(t):
    _bits(t).fill_(0x7FC00DAD if t.element_size() == 4 else 0x7FC1)
    return t


def _ref64(mode, x, w):
    wd = w.to(BF16).double()
    if mode == 0:
        return F.conv2d(x.double(), wd, None, 2, 3, 2)
    return F.conv_transpose2d(x.double(), wd, None, 2, 3, 1, 1, 2)


def _err(tag, y, ref, scale_of=None):
    e = float((y.double() - ref).abs().max() / (ref if scale_of is None else scale_of).abs().max())
    print("%s: max |err| / max |ref| %.2e (bound %.2e)" % (tag, e, TOL[y.dtype]))
    return e


def _operands(mode, B, Kc, Cf, nh, nw, seed=37):
    g = torch.Generator(device="cuda").manual_seed(seed + mode)
    shape = (B, Cf, 2 * nh, 2 * nw) if mode == 0 else (B, Kc, nh, nw)
    return torch.randn(shape, device="cuda", generator=g).to(BF16), torch.randn(Kc, Cf, 4, 4, device="cuda", generator=g) * 0.1


@pytest.fixture(scope="module")
def plans():
    return D.check_cases()


@pytest.fixture(scope="module")
def first_results():
    """(cid, mode) -> (x, w, y64, {dtype: y}) of the first call of every case, computed once and never written."""
    from deepinpainting_amd import ops
    out = {}

    def get(cid, mode):
        if (cid, mode) not in out:
            shape = D.CASES[cid][0]
            x, w = _operands(mode, *shape)
            y = {dt: ops.conv4x4s2_bf16_dil(mode, x, w, *shape, out_dtype=dt) for dt in (F32, BF16)}
            torch.cuda.synchronize()
            out[cid, mode] = (x, w, _ref64(mode, x, w), y)
        return out[cid, mode]
    return get


@DTYPES
@MODES
@CIDS
def test_direct_bf16_dilated(cid, mode, odt, plans, first_results, monkeypatch):
    from deepinpainting_amd import _lib, ops
    L = _lib.lib()
    B, Kc, Cf, nh, nw = shape = D.CASES[cid][0]
    plan = plans[cid, mode]
    assert L.ipsr_conv4x4s2_bf16_dil_workspace_bytes(mode, *shape) == plan["ws"], (cid, mode, plan)
    tag = "%s mode %d %s" % (cid, mode, "bf16" if odt == BF16 else "fp32")
    print(tag, {k: plan[k] for k in ("kt", "ptile", "R", "tiles_per_img", "ktiles", "nstage", "nsplit", "sps", "raw1", "lds")})
    x, w, y64, ys = first_results(cid, mode)
    y = ys[odt]
    run = lambda a, ww: ops.conv4x4s2_bf16_dil(mode, a, ww, a.shape[0], Kc, Cf, nh, nw, out_dtype=odt)
    assert y.dtype == odt and y.shape == y64.shape and torch.isfinite(y).all()
    assert _err(tag, y, y64) <= TOL[odt]
    if mode == 1:
        # every even row and every even column of dx is +0 (all bits clear), with and without a reduction cut
        assert not _bits(y[:, :, 0::2, :]).any() and not _bits(y[:, :, :, 0::2]).any(), "%s: an even row / column of dx is not +0" % tag
    # a second call: the same bits
    assert _same(run(x, w), y), "%s: two calls differ" % tag
    # every image alone: the same bits where the reduction is cut the same way, inside the bound otherwise
    if B >= 2:
        one = D.plan(mode, 1, Kc, Cf, nh, nw)
        for b in range(B):
            yb = run(x[b:b + 1].contiguous(), w)
            assert _err("%s image %d" % (tag, b), yb, y64[b:b + 1], y64) <= TOL[odt]
            if D.same_cut(plan, one):
                assert _same(yb, y[b:b + 1]), "%s: image %d alone differs from the batch" % (tag, b)
    # guard bands: a NaN-filled workspace of exactly the queried size, guard bands round every operand and the result
    keep = (x.clone(), w.clone())
    arena = Arena(ws_fill="nan")
    gx, gw = arena.guarded_copy(x, "x"), arena.guarded_copy(w, "w")
    with arena.installed(monkeypatch):
        got = run(gx, gw)
    torch.cuda.synchronize()
    arena.check_guards()
    assert _same(gx, keep[0]) and _same(gw, keep[1]) and _same(x, keep[0]) and _same(w, keep[1]), "%s: an input was modified" % tag
    assert _same(got, y), "%s: the guarded run differs" % tag
    assert arena.guard_bytes() > 0 and arena.workspaces and arena.workspaces[0][0] == plan["ws"]


@MODES
@CIDS
def test_exact_on_small_integers(cid, mode):
    """Operands of small integers times powers of two: every product and every partial sum is a multiple of 2^-3 below 2^21, exact in fp32 in
    any order — the fp32 output equals the fp64 reference bit for bit."""
    from deepinpainting_amd import ops
    B, Kc, Cf, nh, nw = shape = D.CASES[cid][0]
    g = torch.Generator(device="cuda").manual_seed(5 + mode)
    ishape = (B, Cf, 2 * nh, 2 * nw) if mode == 0 else (B, Kc, nh, nw)
    x = torch.randint(-3, 4, ishape, device="cuda", generator=g).float() * torch.exp2(torch.randint(-1, 2, (1, ishape[1], 1, 1), device="cuda", generator=g).float())
    w = torch.randint(-3, 4, (Kc, Cf, 4, 4), device="cuda", generator=g).float() * torch.exp2(torch.randint(-2, 1, (Kc, 1, 1, 1), device="cuda", generator=g).float())
    assert torch.equal(x.to(BF16).float(), x) and torch.equal(w.to(BF16).float(), w)
    y = ops.conv4x4s2_bf16_dil(mode, x.to(BF16), w, *shape, out_dtype=F32)
    r64 = _ref64(mode, x.to(BF16), w)
    assert float(r64.abs().max()) < 2.0 ** 21 and float(r64.abs().max()) > 0
    assert torch.equal(y.double(), r64), "%s mode %d: %d elements differ from the exact result" % (cid, mode, int((y.double() != r64).sum()))


@DTYPES
@CIDS
def test_forward_reads_only_the_odd_quarter(cid, odt, first_results):
    """Even rows and even columns of x never reach a product (the raw tile carries the even columns into the LDS; the transposition must drop
    them): NaN / Inf there, the same bits."""
    from deepinpainting_amd import ops
    shape = D.CASES[cid][0]
    x, w, _, ys = first_results(cid, 0)
    xp = x.clone()
    xp[:, :, 0::2, :] = float("nan")
    xp[:, :, 1::2, 0::2] = float("inf")
    xp[:, :, 1::4, 0::4] = float("-inf")
    assert _same(xp[:, :, 1::2, 1::2], x[:, :, 1::2, 1::2])
    got = ops.conv4x4s2_bf16_dil(0, xp, w, *shape, out_dtype=odt)
    torch.cuda.synchronize()
    assert _same(got, ys[odt]), "%s: the even rows / columns of x changed the result" % cid


@DTYPES
@CIDS
def test_input_gradient_writes_every_element(cid, odt, first_results):
    """The raw entry on a NaN-filled `out` and workspace: no NaN left, +0 on the even rows and columns, the bits of the ops call."""
    from deepinpainting_amd import _lib, ops
    L = _lib.lib()
    B, Kc, Cf, nh, nw = shape = D.CASES[cid][0]
    dy, w, _, ys = first_results(cid, 1)
    out = _nan_fill(torch.empty(B, Cf, 2 * nh, 2 * nw, device="cuda", dtype=odt))
    nbytes = D.plan(1, *shape)["ws"]
    ws = _nan_fill(torch.empty((nbytes + 3) // 4, device="cuda")).view(torch.uint8)
    torch.cuda.synchronize()
    rc = L.ipsr_conv4x4s2_bf16_dil(1, dy.data_ptr(), w.data_ptr(), out.data_ptr(), *shape, int(odt == BF16), ws.data_ptr(), nbytes, ops._stream())
    torch.cuda.synchronize()
    assert rc == 0, L.ipsr_last_error()
    assert not torch.isnan(out).any(), "%s: %d elements of dx were not written" % (cid, int(torch.isnan(out).sum()))
    assert not _bits(out[:, :, 0::2, :]).any() and not _bits(out[:, :, :, 0::2]).any()
    assert _same(out, ys[odt])


@DTYPES
@MODES
@pytest.mark.parametrize("what", ["w24", "w256", "c8", "rows", "mode2", "mode4", "mode5", "b0", "ws_short"])
def test_refusals_write_nothing(what, mode, odt):
    from deepinpainting_amd import _lib, ops
    L = _lib.lib()
    B, Kc, Cf, nh, nw = {"w24": (1, 16, 16, 12, 24), "w256": (1, 16, 16, 1, 256), "c8": (1, 8, 8, 16, 16), "rows": (1, 16, 16, 12, 16)}.get(what, (1, 16, 16, 16, 16))
    fine = torch.zeros(B, Cf, 2 * nh, 2 * nw, device="cuda", dtype=BF16)
    coarse = torch.zeros(B, Kc, nh, nw, device="cuda", dtype=BF16)
    inp, oshape = (fine, coarse.shape) if mode == 0 else (coarse, fine.shape)
    w = torch.zeros(Kc, Cf, 4, 4, device="cuda")
    out = _nan_fill(torch.empty(oshape, device="cuda", dtype=odt))
    keep = out.clone()
    ws = torch.empty(1 << 20, dtype=torch.uint8, device="cuda")
    nbytes = ws.numel()
    want, msg = {"w24": (IPSR_ERR_UNSUPPORTED, "coarse width 24"), "w256": (IPSR_ERR_UNSUPPORTED, "coarse width 256"),
                 "c8": (IPSR_ERR_UNSUPPORTED, "8 reduction channels are not a multiple of 16"),
                 "rows": (IPSR_ERR_UNSUPPORTED, "12 rows are not a multiple of the 16 rows of a tile"),
                 "mode2": (IPSR_ERR_INVALID, "bad argument"), "mode4": (IPSR_ERR_INVALID, "bad argument"), "mode5": (IPSR_ERR_INVALID, "bad argument"),
                 "b0": (IPSR_ERR_INVALID, "bad argument"), "ws_short": (IPSR_ERR_WORKSPACE, "workspace")}[what]
    call_mode = {"mode2": 2, "mode4": 4, "mode5": 5}.get(what, mode)
    call_B = 0 if what == "b0" else B
    if what in ("w24", "w256", "c8", "rows"):
        assert D.plan(mode, B, Kc, Cf, nh, nw) is None and not ops.conv4x4s2_bf16_dil_supported(mode, B, Kc, Cf, nh, nw)
        assert msg in L.ipsr_last_error().decode("utf-8", "replace")
        with pytest.raises(NotImplementedError):
            ops.conv4x4s2_bf16_dil(mode, inp, w, B, Kc, Cf, nh, nw, out_dtype=odt)
    if what == "ws_short":
        nbytes = L.ipsr_conv4x4s2_bf16_dil_workspace_bytes(mode, B, Kc, Cf, nh, nw) - 1
        assert nbytes > 0
    if what in ("mode2", "mode4", "mode5"):
        assert not ops.conv4x4s2_bf16_dil_supported(call_mode, B, Kc, Cf, nh, nw)
        with pytest.raises(ValueError):
            ops.conv4x4s2_bf16_dil(call_mode, inp, w, B, Kc, Cf, nh, nw, out_dtype=odt)
    torch.cuda.synchronize()
    rc = L.ipsr_conv4x4s2_bf16_dil(call_mode, inp.data_ptr(), w.data_ptr(), out.data_ptr(), call_B, Kc, Cf, nh, nw, int(odt == BF16), ws.data_ptr(), nbytes,
                                   ops._stream())
    text = L.ipsr_last_error().decode("utf-8", "replace")
    torch.cuda.synchronize()
    assert rc == want and msg in text, (rc, text)
    assert _same(out, keep), "the output was written by a refused call"


def test_wrong_dtype_and_shape_raise():
    from deepinpainting_amd import ops
    x = torch.zeros(1, 16, 32, 32, device="cuda", dtype=BF16)
    w = torch.zeros(16, 16, 4, 4, device="cuda")
    with pytest.raises(TypeError):
        ops.conv4x4s2_bf16_dil(0, x.float(), w, 1, 16, 16, 16, 16)                          # reads bf16 activations
    with pytest.raises(TypeError):
        ops.conv4x4s2_bf16_dil(0, x, w.to(BF16), 1, 16, 16, 16, 16)                         # fp32 weights
    with pytest.raises(RuntimeError):
        ops.conv4x4s2_bf16_dil(1, x, w, 1, 16, 16, 16, 16)                                  # mode 1 reads the coarse tensor
    with pytest.raises(RuntimeError):
        ops.conv4x4s2_bf16_dil(0, x[:, :, :16, :16].contiguous(), w, 1, 16, 16, 16, 16)     # mode 0 reads the fine tensor
    with pytest.raises(TypeError):
        ops.conv4x4s2_bf16_dil(0, x, w, 1, 16, 16, 16, 16, out_dtype=torch.float16)         # writes bf16 or fp32


# ---- through the modules ---------------------------------------------------------------------------------------------------------------
@pytest.fixture
def switch(direct_math):
    hipconv = direct_math
    assert hipconv.direct_dilated_bf16() is False
    yield hipconv
    hipconv.set_direct_dilated_bf16(False)


def test_module_runs_the_engine_when_asked(switch):
    from deepinpainting_amd import ops
    hipconv = switch
    torch.manual_seed(7)
    m = nn.Conv2d(32, 48, 4, 2, 3, 2).cuda()
    g = torch.Generator(device="cuda").manual_seed(11)
    x = torch.randn(2, 32, 32, 32, device="cuda", generator=g).to(BF16)
    dy = torch.randn(2, 48, 16, 16, device="cuda", generator=g).to(BF16)
    # under bf16 autocast, as in the trainer (a bare bf16 tensor meets the fp32 weight in torch's own convolution while no engine takes the layer)
    amp = lambda: torch.autocast(device_type="cuda", dtype=BF16)
    with amp():
        today, y0, dx0, dw0 = _module_pass(hipconv, m, x, dy)
    assert today == {}, today                                       # 32 -> 48 channels: all three passes are MIOpen's, the plain module call
    hipconv.set_direct_dilated_bf16(True)
    with amp():
        seen, y, dx, dw = _module_pass(hipconv, m, x, dy)
    assert seen == {"forward": "bf16d", "input_grad": "bf16d", "weight_grad": "miopen"}, seen
    w = m.weight.detach()
    assert y.dtype == BF16 and dx.dtype == BF16 and dw.dtype == F32
    assert _same(y, ops.conv4x4s2_bf16_dil(ops.S2_FINE_TO_COARSE, x, w, 2, 48, 32, 16, 16))
    assert _same(dx, ops.conv4x4s2_bf16_dil(ops.S2_COARSE_TO_FINE, dy, w, 2, 48, 32, 16, 16))
    assert _err("module forward", y, _ref64(0, x, w)) <= TOL[BF16] and _err("module input gradient", dx, _ref64(1, dy, w)) <= TOL[BF16]
    assert _same(dw, dw0), "the weight gradient changed with the switch"
    # the no-grad path
    with torch.no_grad(), amp():
        assert _same(hipconv.conv_nobias(m, x), y)
    # off again: the engines and the bits of before
    hipconv.set_direct_dilated_bf16(False)
    with amp():
        again, y1, dx1, dw1 = _module_pass(hipconv, m, x, dy)
    assert again == today and _same(y1, y0) and _same(dx1, dx0) and _same(dw1, dw0)


def test_training_step_with_the_option(tmp_path, switch):
    """Two training steps with opt.amp_bf16 and opt.direct_dilated_bf16 at 2 x 256x256, dropout on: the losses are finite, the weights of
    netG's dilated layers move, and every dilated forward / input-gradient call of the second step on maps of 32 .. 256 ran on "bf16d" and
    is held, on the tensors the step really produced, to the fp64 reference of its own operands (the input and the weight rounded to bf16, as
    the kernel reads them) at the bound of its output type.  No step-level tolerance against the switch-off step is set."""
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
                 direct_dilated_bf16=True)
    torch.manual_seed(5)
    with contextlib.redirect_stdout(io.StringIO()):
        m = create_model(opt)
    assert hipconv.direct_dilated_bf16() is True
    dilated = [mod for mod in m.netG.modules() if isinstance(mod, nn.Conv2d) and mod.kernel_size == (4, 4) and mod.dilation == (2, 2)]
    assert len(dilated) >= 4
    w0 = [mod.weight.detach().clone() for mod in dilated]
    seen = {}

    def hook(kind, engine, geom, operands, result):
        transposed, k, stride, pad, dil, Cout = geom
        if transposed or (k, stride, pad, dil) != (4, 2, 3, 2) or kind == "weight_grad":
            return
        x = operands[0] if kind == "forward" else operands[1]
        if not 32 <= x.shape[2] <= 256:
            return
        with torch.no_grad():
            inp, mode = (x, 0) if kind == "forward" else (operands[0], 1)
            y64 = _ref64(mode, inp.detach().to(BF16), operands[-1].detach())
            worst = float((result.detach().double() - y64).abs().max() / y64.abs().max())
        seen.setdefault((kind, tuple(x.shape)), []).append((engine, worst, TOL[result.dtype]))

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
        print("%-10s %-20s %s" % (key[0], key[1], ", ".join("%s %.2e (bound %.2e)" % c for c in calls)))
    for C, H in ((64, 256), (128, 128), (256, 64), (512, 32)):
        for kind in ("forward", "input_grad"):
            assert (kind, (B, C, H, H)) in seen, "the step has no dilated %s at %d@%d" % (kind, C, H)
    assert all(eng == "bf16d" and worst <= bound for calls in seen.values() for eng, worst, bound in calls), seen
    losses = m.get_current_errors()
    assert losses and all(torch.isfinite(torch.as_tensor(float(v))) for v in losses.values()), losses
    assert all(not torch.equal(mod.weight.detach(), w) for mod, w in zip(dilated, w0)), "a dilated layer's weight did not move"
