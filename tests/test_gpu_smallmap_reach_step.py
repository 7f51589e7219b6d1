"""One training step with the trainer's reach of the small-map engine's tiled regime (`opt.smallmap_reach`, default 1024), batch 2 at
256x256: every call that reaches "smallmap" through the reach — the dispatcher without a reach answers something else for it — is compared
with MIOpen's result on the very operands the step produced, within twice the bound of tests/test_gpu_smallmap_tiled.py (either result may
be off the exact value by that bound): n * 2^-24 * (|w| (*) |x|), n = the reduction length + 32 slab adds (the most the plan chooses) + k*k
col2im taps, |w| (*) |x| in float64 on the CPU.  Each such call must have reached `ops.conv_smallmap` with `tiled` as `_reach_regime` says for
it, and at least one of them tiled.  The losses are finite, and with `smallmap_reach=0` no such call occurs.
"""
import contextlib
import io

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
U = 2.0 ** -24


def _step(tmp_path, reach, hook):
    from deepinpainting_amd.models import hipconv
    from deepinpainting_amd.models.models import create_model
    from deepinpainting_amd.options import Option
    g = torch.Generator(device="cuda").manual_seed(21)
    B, S, hole = 2, 256, 128
    img = torch.rand(B, 3, S, S, device="cuda", generator=g) * 2 - 1
    ref = torch.rand(B, 3, S, S, device="cuda", generator=g) * 2 - 1
    mask = torch.zeros(1, 1, S, S, dtype=torch.bool, device="cuda")
    mask[:, :, (S - hole) // 2:(S + hole) // 2, (S - hole) // 2:(S + hole) // 2] = 1
    opt = Option(gpu_ids=[0], quiet=True, allow_random_vgg=True, checkpoints_dir=str(tmp_path), batchSize=B, use_dropout=True, smallmap_reach=reach)
    torch.manual_seed(5)
    with contextlib.redirect_stdout(io.StringIO()):
        m = create_model(opt)
    was = hipconv._check_hook
    hipconv._check_hook = hook
    try:
        m.set_input(img, mask, ref)
        m.set_ref_latent()
        m.set_gt_latent()
        m.optimize_parameters()
    finally:
        hipconv._check_hook = was
    torch.cuda.synchronize()
    losses = m.get_current_errors()
    assert losses and all(torch.isfinite(torch.as_tensor(float(v))) for v in losses.values()), losses


def _through_reach(hipconv, ops, kind, engine, geom, operands):
    """-> (op, lay) when this call ran on "smallmap" though the dispatcher without a reach answers otherwise, else None."""
    transposed, k, stride, pad, dil, Cout = geom
    if engine != "smallmap":
        return None
    x = operands[0] if kind == "forward" else operands[1]
    lay = (transposed,) + tuple(x.shape) + (Cout, k, stride, pad, dil)
    if kind == "weight_grad":
        return (None, lay) if hipconv.select_wrw(*lay) != "smallmap" else None
    op = {("forward", False): ops.CONV_FWD, ("input_grad", False): ops.CONV_BWD_DATA,
          ("forward", True): ops.CONVT_FWD, ("input_grad", True): ops.CONVT_BWD_DATA}[kind, transposed]
    return (op, lay) if hipconv.select(op, *lay[1:]) != "smallmap" else None


def test_step_with_the_reach(tmp_path):
    from deepinpainting_amd import ops
    from deepinpainting_amd.models import hipconv
    seen, flags, regimes = [], [], []
    real = ops.conv_smallmap

    def spy(*a, tiled=False, **kw):                 # the engine's call as `_run_data` / `_run_wrw` made it; the hook runs right after it
        flags.append(bool(tiled))
        return real(*a, tiled=tiled, **kw)

    def hook(kind, engine, geom, operands, result):
        if engine == "smallmap":
            last = flags[-1]                        # (calls outside autograd come without a hook: only the latest is this pass's)
            del flags[:]
        hit = _through_reach(hipconv, ops, kind, engine, geom, operands)
        if hit is None:
            assert engine != "smallmap" or last is False, "a pass of the chain's own rules ran tiled"
            return
        assert kind != "weight_grad", "the reach moves no weight gradient"
        want = hipconv._reach_regime("data", *hit)
        assert want in ("stream", "tiled") and last == (want == "tiled"), (kind, hit, want, last)
        regimes.append(want)
        transposed, k, stride, pad, dil, Cout = geom
        with torch.no_grad():
            if kind == "forward":
                x, w = (t.detach() for t in operands)
                theirs = hipconv._miopen_forward(x, w, transposed, stride, pad, dil)
                conv = (lambda a, b: F.conv_transpose2d(a, b, None, stride, pad, 0, 1, dil)) if transposed else (lambda a, b: F.conv2d(a, b, None, stride, pad, dil))
                mag = conv(x.double().abs().cpu(), w.double().abs().cpu())
                n = x.shape[1] * (k * k if not transposed else 1) + 32 + k * k
            else:
                dy, x, w = (t.detach() for t in operands)
                theirs = hipconv._miopen_backward(dy, x, w, transposed, stride, pad, dil, [True, False, False])[0]
                xa = x.double().abs().cpu().requires_grad_()
                with torch.enable_grad():
                    ya = F.conv_transpose2d(xa, w.double().abs().cpu(), None, stride, pad, 0, 1, dil) if transposed else \
                        F.conv2d(xa, w.double().abs().cpu(), None, stride, pad, dil)
                    mag = torch.autograd.grad(ya, xa, dy.double().abs().cpu())[0]
                n = Cout * (k * k if transposed else 1) + 32 + k * k
            err = (result.detach().double() - theirs.double()).abs().cpu()
            worst = float((err / (2 * n * U * mag).clamp_min(1e-300)).max())
        seen.append((kind, hit[1], worst))

    ops.conv_smallmap = spy
    try:
        _step(tmp_path, 1024, hook)
    finally:
        ops.conv_smallmap = real
    assert "tiled" in regimes and "stream" in regimes, regimes
    for kind, lay, worst in seen:
        print("%-10s %-48s %.3f of twice the bound" % (kind, lay, worst))
    assert len(seen) >= 4, "the step made %d calls through the reach" % len(seen)
    assert {s[0] for s in seen} == {"forward", "input_grad"}
    assert all(worst <= 1.0 for _, _, worst in seen), [s for s in seen if s[2] > 1.0]


def test_step_without_the_reach(tmp_path):
    from deepinpainting_amd import ops
    from deepinpainting_amd.models import hipconv
    seen = []
    _step(tmp_path, 0, lambda kind, engine, geom, operands, result: seen.append(_through_reach(hipconv, ops, kind, engine, geom, operands)))
    assert seen and all(s is None for s in seen)
