"""Every convolution engine at the edges of what the dispatcher admits (tests/dispatch_envelope.py `ROWS`: elongated, one-row and one-column
maps, batches 1 and 3, minimum channel counts), through the modules: forward, input gradient and weight gradient of nn.Conv2d /
nn.ConvTranspose2d by `hipconv.conv_nobias` and autograd, each pass on the engine the row names.

Per row: the call runs between guard bands (tests/guarded.py: guarded copies of x, the weight and dy; every result, cache and workspace the
front-ends allocate guarded too, workspaces NaN-filled and exactly the size asked for) — a kernel that writes past an elongated map breaks a
band instead of corrupting a neighbour; then once more on plain tensors (bf16x3_harness._module_pass), and every pass on a HIP engine must
repeat its bits.  Each HIP pass is compared with fp64 autograd of the same operands (of exactly what the kernel multiplies where a side is
bf16: the table above `_ROUNDS_WEIGHTS` in tests/test_gpu_conv.py), error / max |reference| within `_band` of tests/test_gpu_conv.py.  Passes
that land on MIOpen are run and checked for shape and finiteness only.  tests/test_dispatch_envelope.py keeps the rows on their engines
without a GPU; here the engines recorded through `hipconv._check_hook` must equal the row's triple.

Each case prints one line per pass — engine, worst error, band (profiles/dispatch_envelope_errors.txt is that output).
"""
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

import dispatch_envelope as de
from bf16x3_harness import _module_pass
from guarded import Arena, _bits
from test_gpu_conv import _ROUNDS_INPUT, _ROUNDS_WEIGHTS, _WRW_KEEPS_X, _band, _f64

pytestmark = pytest.mark.gpu

KINDS = ("forward", "input_grad", "weight_grad")


@pytest.fixture
def hipconv(monkeypatch):
    """The dispatcher with no engine forced and no A/B switch set; the hook and the switches restored afterwards."""
    from deepinpainting_amd.models import hipconv as hc
    monkeypatch.setattr(hc, "_FORCE", None)
    monkeypatch.setattr(hc, "_check_hook", None)
    for var in ("IPSR_CONV_ENGINE", "IPSR_NO_SMALLMAP", "IPSR_NO_THIN", "IPSR_SMALLMAP_MAX_POS", "IPSR_BF16_ENGINES"):
        monkeypatch.delenv(var, raising=False)
    hc.reload_env()
    yield hc
    monkeypatch.undo()
    hc.reload_env()


def _module(row, w):
    k, stride, pad, dil = row.geom
    m = (nn.ConvTranspose2d if row.mod == "convT" else nn.Conv2d)(row.cin, row.cout, k, stride, pad, dilation=dil, bias=False)
    m.weight = nn.Parameter(w)
    return m


def _same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(_bits(a.contiguous()), _bits(b.contiguous()))


def _rounded(t):
    return t.to(torch.bfloat16).float()


def _reference_operands(kind, engine, bf16, x, w, dy):
    """fp32 copies of what the engine multiplies in this pass (tests/test_gpu_conv.py, the table above `_ROUNDS_WEIGHTS`): all-fp32 calls
    round nothing; with a bf16 side dy is bf16, the weights are rounded by the engines of `_ROUNDS_WEIGHTS`, an fp32 x by those of
    `_ROUNDS_INPUT` (forward) / by every engine outside `_WRW_KEEPS_X` (weight gradient)."""
    x, w, dy = x.float(), w.float(), dy.float()
    if bf16:
        dy = _rounded(dy)
        if kind == "forward":
            x = _rounded(x) if engine in _ROUNDS_INPUT else x
        if kind in ("forward", "input_grad"):
            w = _rounded(w) if engine in _ROUNDS_WEIGHTS else w
        elif engine not in _WRW_KEEPS_X:
            x = _rounded(x)
    return x, w, dy


@pytest.mark.parametrize("row", de.ROWS, ids=[r.id for r in de.ROWS])
def test_every_engine_at_the_edges_of_its_rule(row, hipconv, monkeypatch):
    torch.cuda.set_device(0)
    k, stride, pad, dil = row.geom
    transposed = row.mod == "convT"
    g = torch.Generator(device="cuda").manual_seed(29)
    act = torch.bfloat16 if row.bf16 else torch.float32
    Ho, Wo = de.out_extents(row.lay)
    x0 = torch.randn(row.B, row.cin, row.H, row.W, device="cuda", generator=g).to(act)
    dy0 = torch.randn(row.B, row.cout, Ho, Wo, device="cuda", generator=g).to(act)
    w0 = torch.randn((row.cin, row.cout, k, k) if transposed else (row.cout, row.cin, k, k), device="cuda", generator=g) * 0.1

    # A bf16 tensor into a layer whose three passes are all MIOpen's is the plain torch call, which refuses a bf16 input with fp32 weights: such
    # a row runs under bf16 autocast, the form in which the trainer's bf16 activations reach MIOpen.  The dispatcher answers the same under
    # either form (`hipconv._layer_of`), and the row's point is that no pass reaches a HIP engine.
    amp = torch.autocast("cuda", dtype=torch.bfloat16, enabled=row.bf16 and all(e == "miopen" for e in row.engines))
    with de.switches(hipconv, row.switches), amp:
        math = hipconv.conv_math(row.bf16)
        # between guard bands, on NaN-filled workspaces
        arena = Arena(ws_fill="nan")
        xg, wg, dyg = arena.guarded_copy(x0, "x"), arena.guarded_copy(w0, "w"), arena.guarded_copy(dy0, "dy")
        mg = _module(row, wg)
        seen = {}
        hipconv._check_hook = lambda kind, eng, geom, operands, result: seen.__setitem__(kind, eng)
        with arena.installed(monkeypatch):
            xr = xg.requires_grad_(True)
            y = hipconv.conv_nobias(mg, xr)
            dx, dw = torch.autograd.grad(y, (xr, mg.weight), dyg)
        torch.cuda.synchronize()
        arena.check_guards()
        assert _same(xg.detach(), x0) and _same(wg, w0) and _same(dyg, dy0), "%s: an operand was modified" % row.id
        got = dict(zip(KINDS, (y.detach(), dx, dw)))
        if any(e != "miopen" for e in row.engines):
            assert tuple(seen.get(kd) for kd in KINDS) == row.engines, (row.id, seen)
        else:
            assert not seen                          # all three on MIOpen: the plain torch call, which has no hook
        # once more, on plain tensors
        seen2, y2, dx2, dw2 = _module_pass(hipconv, _module(row, w0.clone()), x0, dy0)
        again = dict(zip(KINDS, (y2, dx2, dw2)))
        assert seen2 == seen, (row.id, seen, seen2)

    shapes = {"forward": dy0.shape, "input_grad": x0.shape, "weight_grad": w0.shape}
    refs, over = {}, []
    f = (lambda a, ww: F.conv_transpose2d(a, ww, None, stride, pad, 0, 1, dil)) if transposed else (lambda a, ww: F.conv2d(a, ww, None, stride, pad, dil))
    for kind, engine in zip(KINDS, row.engines):
        res = got[kind]
        assert res.shape == shapes[kind] and res.dtype == (torch.float32 if kind == "weight_grad" else act), (row.id, kind, res.shape, res.dtype)
        assert bool(torch.isfinite(res).all()) and bool(torch.isfinite(again[kind]).all()), "%s %s on %s is not finite" % (row.id, kind, engine)
        if engine == "miopen":
            print("envelope: %-58s %-11s %-9s (not judged)" % (row.id, kind, engine))
            continue
        assert _same(res, again[kind]), "%s: %s on %s does not repeat its bits" % (row.id, kind, engine)
        xo, wo, dyo = _reference_operands(kind, engine, row.bf16, x0, w0, dy0)
        key = (torch.equal(xo, x0.float()), torch.equal(wo, w0), torch.equal(dyo, dy0.float()))      # one fp64 reference per distinct set of operands
        if key not in refs:
            refs[key] = dict(zip(KINDS, _f64(f, xo, wo, dyo)))
        want = refs[key][kind]
        err = float((res.double() - want).abs().max() / want.abs().max())
        band = _band(engine, math, res)
        print("envelope: %-58s %-11s %-9s err %.2e  band %.2e" % (row.id, kind, engine, err, band))
        if not err <= band:
            over.append((kind, engine, err, band))
    assert not over, (row.id, over)
