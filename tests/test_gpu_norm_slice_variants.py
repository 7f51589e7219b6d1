"""The slice / y2 / dy2 forms of the fused instance norm (csrc/instnorm.hip:87-295) in every launch variant.

These are the forms that carry the U-Net skip connections without a concatenation pass: the forward writes y into a channel slice of
a wider tensor and relu(normalised value) into a slice of a second one (y2); the backward reads dy and y from slices of wider tensors
and adds the gradient of the second output (dy2, a slice again) inside the kernel.  The launcher picks the workgroup shape from the
plane size alone, exactly as for the dense entry points (the table of tests/test_gpu_norm_variants.py, whose PLANES and variant() are
imported here), so every plane size of that table is run again with the slice arguments:

  variant (T threads x E elements, form)   selected at            case ids (each in fp32 and bf16; each runs slice, y2 and dy2)
  ---------------------------------------  ---------------------  -------------------------------------------------------------
  <64, 4>   scalar                         in_dispatch            hw3, hw255
  <64, 4>   vector                         in_dispatch            hw4, hw256
  <64, 16>  scalar                         in_dispatch            hw257, hw1023
  <64, 16>  vector                         in_dispatch            hw260, hw1024
  <256, 16> scalar                         in_dispatch            hw1025, hw4095
  <256, 16> vector                         in_dispatch            hw1028, hw4096
  <256, 64> scalar                         in_dispatch            hw4097, hw16383
  <256, 64> vector                         in_dispatch            hw4100, hw16384
  <512, 128> vector (REX)                  in_dispatch                                       hw16388, hw65536
  slice addresses                          instnorm.hip:99 (y), :101 (y2), :194-198 (dy, y, dy2)
  refused: strides, alignment, tickets     api.hip:489-492, :515-520, launch_instnorm_act_bwd  refuse_* (INVALID)
  refused: plane sizes                     launch_instnorm_act_fwd / _bwd                     refuse_hw16385, refuse_hw65540

Placement (an off-by-one in an offset or a stride lands in a NaN channel or moves a plane): y at channel 2 of C + 5 channels, y2 at
channel 1 of C + 3; the backward reads dy and y from channel 2 of C + 5 and dy2 from channel 1 of C + 3.  Everything outside the
slices holds the NaN pattern of _nan_like.  With odd HW the slice pointers are not 4-element aligned: the scalar cases.

Each case runs the three configurations of CONFIGS and asserts
  1. slice form == dense form, bit for bit (y, mean, rstd; dx, the three partial arrays, the batch sums): the same kernel with other
     strides, so the fp64 check of tests/test_gpu_norm_variants.py carries over to the slice arguments;
  2. y2 slice == relu(y slice) (torch.equal) for every activation, in fp32 and after the one bf16 rounding;
  3. with dy2: dx, dgamma, dbeta, dbias against torch fp64 autograd of sum(act(n) * dy) + sum(relu(n) * dy2), in the bands of
     test_gpu_norm_variants._run (5e-5 of the scale, + 2^-8 for bf16 dx; 2e-6 of max(scale, per-channel sum |dx|) for dbias).  The
     data is drawn by the rule of _draw (same generator order, dy2 last); every pre-activation is >= 2e-6 from 0 in fp64 for EVERY
     activation, since relu' of the second output is always taken;
  4. batch sums == partials added in order b = 0..B-1, bitwise; tickets zero after the backward;
  5. nothing outside the slices is written, the read-only wide tensors are unchanged, every result is finite.
"""
import pytest
import torch

from test_gpu_norm_variants import ACT, CONFIGS, IPSR_ERR_INVALID, IPSR_ERR_UNSUPPORTED, PLANES, _act64, _err, _nan_like, variant

gpu = pytest.mark.gpu

Y_AT, Y_EXTRA = 2, 5          # y, and the backward's dy and y: channels [2, 2 + C) of C + 5
Y2_AT, Y2_EXTRA = 1, 3        # y2 and dy2: channels [1, 1 + C) of C + 3
FORMS = ("slice", "y2", "dy2")  # what _run passes through every case
DTYPES = [torch.float32, torch.bfloat16]


def _shape(HW):
    return (2, 3) if HW > 4096 else (3, 8)


def _draw2(HW, dtype, cfg):
    """_draw's operands (same generator order) plus dy2; EVERY pre-activation >= 2e-6 from 0 in fp64, whatever the activation."""
    act, affine, with_bias = CONFIGS[cfg]
    (H, W), (B, C) = PLANES[HW], _shape(HW)
    seed = HW * 8 + cfg
    for s in range(seed, seed + 64):
        g = torch.Generator().manual_seed(s)
        x = (torch.randn(B, C, H, W, generator=g) * 2 + 0.5).to(dtype)
        dy = torch.randn(B, C, H, W, generator=g).to(dtype)
        bias = torch.randn(C, generator=g) if with_bias else None
        gamma = torch.rand(C, generator=g) + 0.5 if affine else None
        beta = torch.randn(C, generator=g) if affine else None
        dy2 = torch.randn(B, C, H, W, generator=g).to(dtype)
        u = torch.nn.functional.instance_norm(x.double() + (bias.double().view(1, -1, 1, 1) if with_bias else 0), None, None,
                                              gamma.double() if affine else None, beta.double() if affine else None, True, 0.1, 1e-5)
        if float(u.abs().min()) >= 2e-6:
            return x, dy, dy2, bias, gamma, beta
    raise AssertionError("no seed keeps the data away from the ReLU kink")


def _ref64(x, dy, dy2, bias, gamma, beta, act):
    C = x.shape[1]
    x64 = x.double().requires_grad_(True)
    b64 = (bias.double() if bias is not None else torch.zeros(C, dtype=torch.float64)).requires_grad_(True)
    g64 = (gamma.double() if gamma is not None else torch.ones(C, dtype=torch.float64)).requires_grad_(True)
    be64 = (beta.double() if beta is not None else torch.zeros(C, dtype=torch.float64)).requires_grad_(True)
    n = torch.nn.functional.instance_norm(x64 + b64.view(1, -1, 1, 1), None, None, g64, be64, True, 0.1, 1e-5)
    loss = (_act64(n, act) * dy.double()).sum() + (torch.relu(n) * dy2.double()).sum()
    return torch.autograd.grad(loss, (x64, g64, be64, b64))


def _bits(t):
    return t.contiguous().view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32)


def _same(a, b):
    return torch.equal(_bits(a), _bits(b))


def _wide(t, at, extra):
    """t in channels [at, at + C) of a NaN-filled tensor with `extra` more channels -> (wide, pointer to the slice, batch stride)."""
    B, C, H, W = t.shape
    w = _nan_like((B, C + extra, H, W), t.dtype)
    w[:, at:at + C] = t
    return w, w.data_ptr() + at * H * W * w.element_size(), (C + extra) * H * W


def _outside_untouched(wide, at, C, what):
    pat = _nan_like((1,), wide.dtype)
    for part in (wide[:, :at], wide[:, at + C:]):
        assert bool((_bits(part) == _bits(pat)).all()), "%s: channels outside the slice were written" % what


def _bwd(L, ops, dyp, dybs, d2p, d2bs, yp, ybs, x, bias, gamma, mean, rstd, act, tickets, dense=False):
    B, C = x.shape[:2]
    HW = x.numel() // (B * C)
    bf = int(x.dtype == torch.bfloat16)
    dx = _nan_like(tuple(x.shape), x.dtype)
    part = _nan_like((3, B, C), torch.float32)
    sums = _nan_like((3, C), torch.float32)
    tail = (bias, gamma, mean.data_ptr(), rstd.data_ptr(), ACT[act], 0.2, B, C, HW, bf, dx.data_ptr(), part[0].data_ptr(),
            part[1].data_ptr(), part[2].data_ptr(), sums.data_ptr(), tickets.data_ptr(), ops._stream())
    if dense:
        rc = L.ipsr_instnorm_act_backward(dyp, yp, x.data_ptr(), *tail)
    else:
        rc = L.ipsr_instnorm_act_backward_slice(dyp, dybs, d2p, d2bs, yp, ybs, x.data_ptr(), *tail)
    assert rc == 0, (rc, L.ipsr_last_error())
    torch.cuda.synchronize()
    # 4. the batch sums of the ticketed launch == the partials added in order b = 0..B-1 (fp32), bit for bit; tickets back at zero
    ordered = torch.zeros_like(part[:, 0, :])
    for b in range(B):
        ordered = ordered + part[:, b, :]
    assert _same(sums, ordered), "sums are not the ordered sum of the partials"
    assert int(tickets.abs().max()) == 0
    return dx, part, sums


def _run(HW, dtype, cfg):
    from deepinpainting_amd import _lib, ops
    L = _lib.lib()
    act, affine, with_bias = CONFIGS[cfg]
    (H, W), (B, C) = PLANES[HW], _shape(HW)
    bf = dtype == torch.bfloat16
    where = (HW, dtype, act, affine, with_bias)
    x, dy, dy2, bias, gamma, beta = _draw2(HW, dtype, cfg)
    dx64, dg64, db64, dbias64 = _ref64(x, dy, dy2, bias, gamma, beta, act)
    xd, dyd, dy2d = x.cuda(), dy.cuda(), dy2.cuda()
    bd, gd, bed = (t.cuda() if t is not None else None for t in (bias, gamma, beta))
    bp, gp = ops._ptr(bd), ops._ptr(gd)

    # dense forward, slice forward without y2, slice forward with y2
    y_d, mean_d, rstd_d, tick_d = ops.instnorm_act_forward(xd, bd, gd, bed, 1e-5, act, 0.2, return_tickets=True)
    wide_a = _nan_like((B, C + Y_EXTRA, H, W), dtype)
    _, mean_a, rstd_a, tick_a = ops.instnorm_act_forward(xd, bd, gd, bed, 1e-5, act, 0.2, into=wide_a, into_at=Y_AT, return_tickets=True)
    wide_y = _nan_like((B, C + Y_EXTRA, H, W), dtype)
    wide_y2 = _nan_like((B, C + Y2_EXTRA, H, W), dtype)
    _, mean_b, rstd_b, tick_b = ops.instnorm_act_forward(xd, bd, gd, bed, 1e-5, act, 0.2, into=wide_y, into_at=Y_AT, relu_into=wide_y2,
                                                        relu_at=Y2_AT, return_tickets=True)
    torch.cuda.synchronize()
    # 1. forward: the slice holds the dense form's bytes, with and without the second output
    for tag, wide, mean, rstd in (("slice", wide_a, mean_a, rstd_a), ("slice+y2", wide_y, mean_b, rstd_b)):
        assert _same(wide[:, Y_AT:Y_AT + C], y_d), ("y", tag) + where
        assert _same(mean, mean_d) and _same(rstd, rstd_d), ("mean/rstd", tag) + where
        _outside_untouched(wide, Y_AT, C, "y (%s)" % tag)                              # 5.
    # 2. y2 == relu(y), the ReLU of the same normalised value, exact in fp32 and after the one bf16 rounding
    y2 = wide_y2[:, Y2_AT:Y2_AT + C]
    assert torch.equal(y2, torch.relu(wide_y[:, Y_AT:Y_AT + C])), ("y2",) + where
    _outside_untouched(wide_y2, Y2_AT, C, "y2")                                        # 5.
    assert bool(torch.isfinite(y_d.float()).all()) and bool(torch.isfinite(y2.float()).all())

    # backward: dense, slice without dy2, slice with dy2
    wide_dy, dyp, dybs = _wide(dyd, Y_AT, Y_EXTRA)
    wide_dy2, d2p, d2bs = _wide(dy2d, Y2_AT, Y2_EXTRA)
    yp, ybs = wide_y.data_ptr() + Y_AT * H * W * wide_y.element_size(), (C + Y_EXTRA) * H * W
    if HW % 4 == 0:   # the vector form's precondition (api.hip:518-519); with odd HW no slice pointer is 4-element aligned
        assert all(p % (8 if bf else 16) == 0 for p in (dyp, d2p, yp)) and (dybs | d2bs | ybs) % 4 == 0
    else:
        assert HW % 2 == 1 and (Y_AT * HW) % 4 and (Y2_AT * HW) % 4
    keep = [t.clone() for t in (wide_dy, wide_dy2, wide_y)]
    dx_d, part_d, sums_d = _bwd(L, ops, dyd.data_ptr(), 0, None, 0, y_d.data_ptr(), 0, xd, bp, gp, mean_d, rstd_d, act, tick_d, dense=True)
    dx_s, part_s, sums_s = _bwd(L, ops, dyp, dybs, None, 0, yp, ybs, xd, bp, gp, mean_b, rstd_b, act, tick_b)
    # 1. backward: dx, the three partial arrays and the sums equal the dense backward's, byte for byte
    assert _same(dx_s, dx_d), ("dx slice vs dense",) + where
    assert _same(part_s, part_d) and _same(sums_s, sums_d), ("partials / sums slice vs dense",) + where
    dx, part, sums = _bwd(L, ops, dyp, dybs, d2p, d2bs, yp, ybs, xd, bp, gp, mean_b, rstd_b, act, tick_b)
    # 5. read-only operands unchanged, nothing read from the NaN channels
    for name, a, b in zip(("dy", "dy2", "y"), (wide_dy, wide_dy2, wide_y), keep):
        assert _same(a, b), "the backward wrote its operand %s" % name
    for t in (dx_d, dx, part, sums):
        assert bool(torch.isfinite(t.float()).all()), ("not finite",) + where
    # 3. dy2 against fp64
    extra = 2.0 ** -8 if bf else 0.0
    e, s = _err(dx, dx64)
    assert e <= (5e-5 + extra) * s, ("dx", e / s) + where
    for name, got, want in (("dgamma", sums[0], dg64), ("dbeta", sums[1], db64)):
        e, s = _err(got, want)
        assert e <= 5e-5 * s, (name, e / s) + where
    e, s = _err(sums[2], dbias64)
    s = max(s, float(dx64.abs().sum(dim=(0, 2, 3)).max()))
    assert e <= 2e-6 * s, ("dbias", e / s) + where


@gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16"])
@pytest.mark.parametrize("HW", sorted(PLANES), ids=["hw%d" % k for k in sorted(PLANES)])
def test_slice_forms_in_every_launch_variant(HW, dtype):
    v = variant(HW)
    assert v is not None and v[2] == (HW % 4 == 0)
    T, E, _ = v
    assert (T * E) // 4 < HW <= T * E or (T, E) == (64, 4), (HW, v)
    for cfg in range(len(CONFIGS)):
        _run(HW, dtype, cfg)


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16"])
def test_a_seed_is_found_for_every_case(dtype):
    """No GPU: the draw of every (plane, configuration) finds, within its 64 seeds, data whose pre-activations keep 2e-6 from 0."""
    for HW in sorted(PLANES):
        for cfg in range(len(CONFIGS)):
            x, dy, dy2 = _draw2(HW, dtype, cfg)[:3]
            assert x.dtype == dtype and x.shape == dy.shape == dy2.shape == _shape(HW) + PLANES[HW]


# ---- refusals ----

def _refusal_operands(H, W, dtype):
    B, C = 2, 3
    t = {"B": B, "C": C, "HW": H * W, "bf": int(dtype == torch.bfloat16), "es": 2 if dtype == torch.bfloat16 else 4}
    t["x"] = torch.randn(B, C, H, W, device="cuda").to(dtype)
    t["bias"], t["gamma"], t["beta"] = (torch.randn(C, device="cuda") for _ in range(3))
    # one spare plane behind each wide tensor: an "off by one element" pointer still lies inside the allocation
    t["wy"] = _nan_like((B * (C + Y_EXTRA) + 1, H, W), dtype)
    t["wy2"] = _nan_like((B * (C + Y2_EXTRA) + 1, H, W), dtype)
    t["wdy"] = torch.randn(B * (C + Y_EXTRA) + 1, H, W, device="cuda").to(dtype)
    t["wyin"] = torch.randn(B * (C + Y_EXTRA) + 1, H, W, device="cuda").to(dtype)
    t["wdy2"] = torch.randn(B * (C + Y2_EXTRA) + 1, H, W, device="cuda").to(dtype)
    t["stats"] = _nan_like((2 * B * C + C,), torch.float32)
    t["dx"] = _nan_like((B, C, H, W), dtype)
    t["part"] = _nan_like((3, B, C), torch.float32)
    t["sums"] = _nan_like((3, C), torch.float32)
    t["outputs"] = ("wy", "wy2", "stats", "dx", "part", "sums")
    t["keep"] = [t[k].clone() for k in t["outputs"]]
    torch.cuda.synchronize()
    return t


def _refused_fwd(t, code, y_off=0, y2_off=0, ybs=None, y2bs=None, with_y2=True):
    from deepinpainting_amd import _lib, ops
    L = _lib.lib()
    B, C, HW, es = t["B"], t["C"], t["HW"], t["es"]
    s = t["stats"]
    rc = L.ipsr_instnorm_act_forward_slice(
        t["x"].data_ptr(), t["bias"].data_ptr(), t["gamma"].data_ptr(), t["beta"].data_ptr(), 1e-5, 2, 0.2, B, C, HW, t["bf"],
        t["wy"].data_ptr() + (Y_AT * HW + y_off) * es, (C + Y_EXTRA) * HW if ybs is None else ybs,
        t["wy2"].data_ptr() + (Y2_AT * HW + y2_off) * es if with_y2 else None, ((C + Y2_EXTRA) * HW if y2bs is None else y2bs) if with_y2 else 0,
        s[:B * C].data_ptr(), s[B * C:2 * B * C].data_ptr(), s[2 * B * C:].data_ptr(), ops._stream())
    assert rc == code, (rc, L.ipsr_last_error())


def _refused_bwd(t, code, dy_off=0, y_off=0, dy2_off=0, dybs=None, ybs=None, dy2bs=None, with_dy2=True, tickets=True):
    from deepinpainting_amd import _lib, ops
    L = _lib.lib()
    B, C, HW, es = t["B"], t["C"], t["HW"], t["es"]
    s, p = t["stats"], t["part"]
    mean = torch.zeros(B * C, device="cuda")
    rstd = torch.ones(B * C, device="cuda")
    rc = L.ipsr_instnorm_act_backward_slice(
        t["wdy"].data_ptr() + (Y_AT * HW + dy_off) * es, (C + Y_EXTRA) * HW if dybs is None else dybs,
        t["wdy2"].data_ptr() + (Y2_AT * HW + dy2_off) * es if with_dy2 else None, ((C + Y2_EXTRA) * HW if dy2bs is None else dy2bs) if with_dy2 else 0,
        t["wyin"].data_ptr() + (Y_AT * HW + y_off) * es, (C + Y_EXTRA) * HW if ybs is None else ybs,
        t["x"].data_ptr(), t["bias"].data_ptr(), t["gamma"].data_ptr(), mean.data_ptr(), rstd.data_ptr(), 2, 0.2, B, C, HW, t["bf"],
        t["dx"].data_ptr(), p[0].data_ptr(), p[1].data_ptr(), p[2].data_ptr(), t["sums"].data_ptr(),
        s[2 * B * C:].data_ptr() if tickets else None, ops._stream())
    assert rc == code, (rc, L.ipsr_last_error())


def _nothing_written(t):
    torch.cuda.synchronize()
    for name, b in zip(t["outputs"], t["keep"]):
        assert torch.equal(t[name].view(torch.uint8), b.view(torch.uint8)), "%s was written by a refused call" % name


@gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16"])
def test_refused_slice_arguments_write_nothing(dtype):
    """IPSR_ERR_INVALID for a batch stride below C*HW (y, y2, dy, y, dy2), for a vector-sized plane (HW % 4 == 0) with a batch stride
    that is no multiple of 4 or a slice pointer one element off, and for batch sums without ticket words; a scalar-sized plane takes
    the same odd strides and pointers (they are the scalar cases above).  Outputs hold a NaN pattern and stay bitwise unchanged."""
    t = _refusal_operands(4, 6, dtype)          # HW = 24: vector form
    C, HW = t["C"], t["HW"]
    _refused_fwd(t, 0)                          # the arguments every refusal below departs from are accepted ...
    _refused_bwd(t, 0)
    t = _refusal_operands(4, 6, dtype)          # ... (fresh NaN-filled outputs)
    _refused_fwd(t, IPSR_ERR_INVALID, ybs=C * HW - 1)
    _refused_fwd(t, IPSR_ERR_INVALID, ybs=C * HW - 4)
    _refused_fwd(t, IPSR_ERR_INVALID, y2bs=C * HW - 1)
    _refused_fwd(t, IPSR_ERR_INVALID, y2bs=C * HW - 4)
    _refused_fwd(t, IPSR_ERR_INVALID, ybs=(C + Y_EXTRA) * HW + 1)
    _refused_fwd(t, IPSR_ERR_INVALID, ybs=(C + Y_EXTRA) * HW + 2, with_y2=False)
    _refused_fwd(t, IPSR_ERR_INVALID, y2bs=(C + Y2_EXTRA) * HW + 1)
    _refused_fwd(t, IPSR_ERR_INVALID, y_off=1)
    _refused_fwd(t, IPSR_ERR_INVALID, y_off=1, with_y2=False)
    _refused_fwd(t, IPSR_ERR_INVALID, y2_off=1)
    _refused_bwd(t, IPSR_ERR_INVALID, dybs=C * HW - 4)
    _refused_bwd(t, IPSR_ERR_INVALID, ybs=C * HW - 4)
    _refused_bwd(t, IPSR_ERR_INVALID, dy2bs=C * HW - 4)
    for k in ("dybs", "ybs"):
        _refused_bwd(t, IPSR_ERR_INVALID, **{k: (C + Y_EXTRA) * HW + 1})
        _refused_bwd(t, IPSR_ERR_INVALID, with_dy2=False, **{k: (C + Y_EXTRA) * HW + 2})
    _refused_bwd(t, IPSR_ERR_INVALID, dy2bs=(C + Y2_EXTRA) * HW + 1)
    for k in ("dy_off", "y_off", "dy2_off"):
        _refused_bwd(t, IPSR_ERR_INVALID, **{k: 1})
    _refused_bwd(t, IPSR_ERR_INVALID, tickets=False)
    _refused_bwd(t, IPSR_ERR_INVALID, tickets=False, with_dy2=False)
    _nothing_written(t)
    t = _refusal_operands(3, 7, dtype)          # HW = 21: scalar form, strides below C*HW are refused all the same
    C, HW = t["C"], t["HW"]
    _refused_fwd(t, IPSR_ERR_INVALID, ybs=C * HW - 1)
    _refused_fwd(t, IPSR_ERR_INVALID, y2bs=C * HW - 1)
    _refused_bwd(t, IPSR_ERR_INVALID, dybs=C * HW - 1)
    _refused_bwd(t, IPSR_ERR_INVALID, ybs=C * HW - 1)
    _refused_bwd(t, IPSR_ERR_INVALID, dy2bs=C * HW - 1)
    _refused_bwd(t, IPSR_ERR_INVALID, tickets=False)
    _nothing_written(t)


@gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16"])
@pytest.mark.parametrize("H,W", [(5, 3277), (5, 13108)], ids=["refuse_hw16385", "refuse_hw65540"])
def test_refused_planes_write_nothing_in_slice_form(H, W, dtype):
    """HW = 16385 (scalar above the register limit) and 65540 (above the largest plane): IPSR_ERR_UNSUPPORTED from the slice forms,
    with and without y2 / dy2, and no output written."""
    assert variant(H * W) is None
    t = _refusal_operands(H, W, dtype)
    for second in (True, False):
        _refused_fwd(t, IPSR_ERR_UNSUPPORTED, with_y2=second)
        _refused_bwd(t, IPSR_ERR_UNSUPPORTED, with_dy2=second)
    _nothing_written(t)


def test_every_variant_is_reached_in_every_slice_form():
    """No GPU: the cases reach all nine launch shapes at their capacity edges, each with the slice, the y2 and the dy2 argument, in
    fp32 and bf16, and every scalar case has slice pointers that are not 4-element aligned."""
    cases = [(variant(hw), form, dtype) for hw in PLANES for form in FORMS for dtype in DTYPES]
    shapes = {(64, 4, False), (64, 4, True), (64, 16, False), (64, 16, True), (256, 16, False), (256, 16, True), (256, 64, False),
              (256, 64, True), (512, 128, True)}
    assert set(cases) == {(v, form, dtype) for v in shapes for form in ("slice", "y2", "dy2") for dtype in DTYPES}
    for T, E in ((64, 4), (64, 16), (256, 16), (256, 64), (512, 128)):
        assert T * E in PLANES and (T * E == 65536 or T * E + 1 in PLANES or T * E + 4 in PLANES)
    for hw in PLANES:
        B, C = _shape(hw)
        if hw % 4:
            assert hw % 2 == 1 and (Y_AT * hw) % 4 and (Y2_AT * hw) % 4, hw
        assert B * (C + Y_EXTRA) * hw <= 2 * 8 * 65536          # the largest tensor of the module
