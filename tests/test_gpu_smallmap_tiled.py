"""The tiled regime of the small-map engine (csrc/smallmap.hip, `ops.conv_smallmap(..., tiled=True)`): forward-type (SM_FWD) and
data-type (SM_DATA) passes as LDS-tiled split-K GEMMs, the weight gradient (SM_WRW, which has no tiled form and must run as without the
flag), against the same convolution in float64 on the CPU.

Bound, fixed before any run: per output element |y - y64| <= n * 2^-24 * (|w| (*) |x|), the bound of an fp32 fma chain followed by
ordered adds, with n = the reduction length + the slab adds + the col2im taps: SM_FWD Cq*k*k + nslab, SM_DATA R + nslab + k*k, SM_WRW the
number of positions.  nslab is the call's own number of splits, read off the workspace the library asks for (nslab partial tiles of
rows x Tp floats and 768 spare bytes).  |w| (*) |x| is computed in float64.

The shapes are the smallest that reach each path of the plan and the kernel (tiles are 128 rows x 128 positions, stages 16 deep):
  rows        R = 32 (a quarter of a row tile: three of a workgroup's four 32-row bands are outside) and R = 160 (a tile + 32);
              Cq = 8 (k4) and 128 (k3), the least with Cq*k*k % 128 == 0
  positions   33 (the first the regime takes: B = 11 on 1x3), 128, 129 (a second position tile with one position), 160 (B = 10 on 4x4: image
              borders inside a tile), 1024 (B = 16 on 8x8), and the refusal at 1025
  reduction   one split of two stages, the least the plan chooses (SM_DATA with R = 32); a ragged last split (SM_FWD 328 stages in 30 splits
              of 11, the last has 9; SM_DATA 26 stages in 3 splits of 9, the last has 8); 32 splits, the most the plan chooses; and one stage
              only per split — a prologue and no further stage — which the plan never chooses and `ipsr_debug_set_option(6, n)` forces
  taps        1x3 maps (k3: every tap but one row outside, on every side), 4x4 maps under k4 s2 p3 d2 (taps outside on every side)
"""
import functools

import pytest
import torch
import torch.nn.functional as F

K3, K4, K4D = (3, 1, 1, 1), (4, 2, 1, 1), (4, 2, 3, 2)
# (role, R, Cq, coarse H, coarse W, (k, stride, pad, dil), B)
CASES = (
    ("conv", 32, 128, 1, 3, K3, 11),        # P = 33
    ("conv", 160, 128, 4, 4, K3, 8),        # P = 128
    ("convT", 160, 128, 1, 3, K3, 43),      # P = 129
    ("conv", 160, 128, 8, 8, K3, 16),       # P = 1024
    ("conv", 160, 8, 4, 4, K4, 10),         # P = 160
    ("convT", 32, 8, 8, 8, K4, 16),         # P = 1024
    ("conv", 32, 8, 4, 4, K4D, 8),          # P = 128, dilated
    ("convT", 160, 8, 4, 4, K4D, 10),       # P = 160, dilated, odd fine grid (7x7)
    ("conv", 32, 328, 4, 4, K4, 10),        # SM_FWD: ragged last split
    ("convT", 416, 8, 4, 4, K4, 8),         # SM_DATA: ragged last split
    ("conv", 32, 512, 4, 4, K4, 8),         # SM_FWD: 32 splits
)
IDS = ["%s_R%d_Cq%d_%dx%d_k%dd%d_B%d" % (c[0], c[1], c[2], c[3], c[4], c[5][0], c[5][3], c[6]) for c in CASES]
U = 2.0 ** -24


def _fine(role, H, W, geom):
    k, st, pad, dil = geom
    if geom == K3:
        return H, W
    if geom == K4:
        return 2 * H, 2 * W
    return (2 * H, 2 * W) if role == "conv" else (2 * H - 1, 2 * W - 1)


@functools.lru_cache(maxsize=None)
def _reference(case):
    """fp32 operands and, in float64 on the CPU, the three results with their |w| (*) |x| companions.  Computed once per case, never modified."""
    role, R, Cq, H, W, geom, B = case
    k, st, pad, dil = geom
    Hf, Wf = _fine(role, H, W, geom)
    g = torch.Generator().manual_seed(1000 + CASES.index(case))
    coarse = torch.randn(B, R, H, W, generator=g)
    fine = torch.randn(B, Cq, Hf, Wf, generator=g)
    w = torch.randn(R, Cq, k, k, generator=g) * 0.05
    out = {}
    for tag, fn in (("val", lambda t: t.double()), ("abs", lambda t: t.double().abs())):
        c, f, wt = fn(coarse).requires_grad_(), fn(fine).requires_grad_(), fn(w).requires_grad_()
        if role == "conv":          # Conv2d [Cout = R][Cin = Cq]: fine -> coarse
            y = F.conv2d(f, wt, None, st, pad, dil)
            assert y.shape == c.shape
            data, dw = torch.autograd.grad(y, (f, wt), c.detach())
            out[tag] = dict(fwd=y.detach(), data=data, wrw=dw)
        else:                       # ConvTranspose2d [Cin = R][Cout = Cq]: coarse -> fine
            y = F.conv_transpose2d(c, wt, None, st, pad, 0, 1, dil)
            assert y.shape == f.shape
            fwd, dw = torch.autograd.grad(y, (c, wt), f.detach())
            out[tag] = dict(fwd=fwd, data=y.detach(), wrw=dw)
    n = dict(fwd=Cq * k * k, data=R + k * k, wrw=B * H * W)          # without the slab adds: `_nslab`
    geo = (B, R, Cq, H, W, Hf, Wf, k, st, pad, dil)
    return coarse, fine, w, out["val"], out["abs"], n, geo


def _nslab(ops, name, geo):
    """The splits of the tiled call as the library plans it now: its workspace is nslab partial tiles [rows][Tp] + 768 bytes."""
    if name == "wrw":
        return 0
    from deepinpainting_amd import _lib
    B, R, Cq, H, W = geo[:5]
    k = geo[7]
    rows, Tp = (R if name == "fwd" else Cq * k * k), (B * H * W + 127) // 128 * 128
    nbytes = _lib.lib().ipsr_conv_smallmap_workspace_bytes((ops.SM_FWD if name == "fwd" else ops.SM_DATA) | ops.SM_TILED, *geo)
    ns, rest = divmod(nbytes - 768, rows * Tp * 4)
    assert rest == 0 and ns >= 1, (nbytes, rows, Tp)
    return ns


def _check(ops, name, case, want_nslab=None):
    _, _, _, val, mag, n, geo = _reference(case)
    ns = _nslab(ops, name, geo)
    assert want_nslab is None or ns == want_nslab, (ns, want_nslab)
    got = _run(ops, name, case)
    again = _run(ops, name, case)
    torch.cuda.synchronize()
    assert got.shape == val[name].shape and got.dtype == torch.float32
    assert torch.equal(got.view(torch.int32), again.view(torch.int32)), "two identical calls differ"
    err = (got.cpu().double() - val[name]).abs()
    bound = (n[name] + ns) * U * mag[name]
    worst = float((err / bound.clamp_min(1e-300)).max())
    print("%s %s nslab %d: worst error / bound %.3f, max |err| %.3g" % (name, geo, ns, worst, float(err.max())))
    assert torch.isfinite(got).all() and bool((err <= bound).all()), "error %.3g x the bound" % worst


def _run(ops, name, case, tiled=True):
    coarse, fine, w, _, _, _, geo = _reference(case)
    c, f, wt = coarse.cuda(), fine.cuda(), w.cuda()
    if name == "fwd":
        return ops.conv_smallmap(ops.SM_FWD, f, wt, *geo, tiled=tiled)
    if name == "data":
        return ops.conv_smallmap(ops.SM_DATA, c, wt, *geo, tiled=tiled)
    return ops.conv_smallmap(ops.SM_WRW, c, f, *geo, tiled=tiled)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ("fwd", "data", "wrw"))
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_tiled_against_float64(case, name):
    from deepinpainting_amd import ops
    _check(ops, name, case, {(IDS[8], "fwd"): 30, (IDS[9], "data"): 3, (IDS[10], "fwd"): 32, (IDS[0], "data"): 1}.get((IDS[CASES.index(case)], name)))


@pytest.mark.gpu
@pytest.mark.parametrize("name", ("fwd", "data"))
@pytest.mark.parametrize("case", (CASES[6], CASES[2]), ids=(IDS[6], IDS[2]))
def test_one_stage_per_split(case, name):
    """Debug option 6 with a count beyond the stages: every split is one stage (the kernel's prologue and nothing else), and the sum over
    as many partial tiles as there are stages — 8 / 72 (SM_FWD) and 2 / 10 (SM_DATA) here — stays inside the same bound."""
    from deepinpainting_amd import _lib, ops
    role, R, Cq, H, W, geom, B = case
    stages = (Cq * geom[0] * geom[0] if name == "fwd" else R) // 16
    L = _lib.lib()
    _lib.check(L.ipsr_debug_set_option(6, 1 << 20), "ipsr_debug_set_option")
    try:
        _check(ops, name, case, stages)
    finally:
        L.ipsr_debug_set_option(6, 0)


@pytest.mark.gpu
@pytest.mark.parametrize("case", (CASES[0], CASES[4], CASES[7], CASES[8]), ids=(IDS[0], IDS[4], IDS[7], IDS[8]))
def test_debug_option_5_runs_the_streaming_kernels(case):
    """A/B: under ipsr_debug_set_option(5, 1) a call with the flag gives the bits of the same call without it."""
    from deepinpainting_amd import _lib, ops
    L = _lib.lib()
    for name in ("fwd", "data", "wrw"):
        stream = _run(ops, name, case, tiled=False)
        _lib.check(L.ipsr_debug_set_option(5, 1), "ipsr_debug_set_option")
        try:
            ab = _run(ops, name, case, tiled=True)
        finally:
            L.ipsr_debug_set_option(5, 0)
        assert torch.equal(ab.view(torch.int32), stream.view(torch.int32)), name
        if name == "wrw":           # no tiled form: the flag changes nothing
            assert torch.equal(_run(ops, name, case, tiled=True).view(torch.int32), stream.view(torch.int32))


def test_position_limit_and_flag_range():
    """No kernel launched: 1024 positions are taken with the flag, 1025 refused, as without it; unknown flag bits are refused."""
    from deepinpainting_amd import _lib, ops
    geo = lambda B: (B, 32, 128, 1, 1, 1, 1, 3, 1, 1, 1)
    for op in (ops.SM_FWD, ops.SM_DATA, ops.SM_WRW):
        assert ops.smallmap_supported(op, *geo(1024), tiled=True) and ops.smallmap_supported(op, *geo(1024))
        assert not ops.smallmap_supported(op, *geo(1025), tiled=True) and not ops.smallmap_supported(op, *geo(1025))
        assert _lib.lib().ipsr_conv_smallmap_workspace_bytes(op | 32, *geo(64)) == 0
        assert _lib.lib().ipsr_conv_smallmap_workspace_bytes(op | 4, *geo(64)) == 0
