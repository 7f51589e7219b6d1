"""The fused instance norm + activation (csrc/instnorm.hip) in every launch variant, against torch in fp64.

The launcher picks a workgroup shape from the plane size HW alone (`in_dispatch` of instnorm.hip, which also holds the streaming "REX"
shape above 16384 elements): a thread holds E elements, T threads a plane, so T*E is the regime's
capacity.  Each regime comes in a vector (HW % 4 == 0) and a scalar form; all come with fp32 and bf16 activations.  A case sits at
a capacity edge (HW == T*E), one element past it (the next regime with a ragged last pass) or just below it, on non-square planes.

  variant (T threads x E elements, form)   HW range            selected at            case ids (each in fp32 and bf16)
  ---------------------------------------  ------------------  ---------------------  -----------------------------------------
  <64, 4>   scalar                         2 .. 256            in_dispatch            hw3, hw255
  <64, 4>   vector                         4 .. 256            in_dispatch            hw4, hw256
  <64, 16>  scalar                         257 .. 1024         in_dispatch            hw257, hw1023
  <64, 16>  vector                         260 .. 1024         in_dispatch            hw260, hw1024
  <256, 16> scalar                         1025 .. 4096        in_dispatch            hw1025, hw4095
  <256, 16> vector                         1028 .. 4096        in_dispatch            hw1028, hw4096
  <256, 64> scalar                         4097 .. 16384       in_dispatch            hw4097, hw16383
  <256, 64> vector                         4100 .. 16384       in_dispatch            hw4100, hw16384
  <512, 128> vector (REX)                  16388 .. 65536      in_dispatch            hw16388, hw65536
  refused: HW = 1 (IPSR_ERR_INVALID)       < 2                 api.hip:470            refuse_hw1
  refused: scalar above the register limit 16385 (HW % 4 != 0) the two launchers      refuse_hw16385
  refused: above the largest plane         65540               the two launchers      refuse_hw65540

Every case runs three configurations, so each variant meets every activation, affine and not, bias and not:
(none, affine, bias), (relu, no affine, bias), (leaky, affine, no bias).

Reference: torch fp64 on the same operands (bf16 inputs upcast exactly; a missing gamma / beta / bias is 1 / 0 / 0, the identity the
kernel applies).  Bands are those of test_fused_instnorm_act_vs_torch against torch fp32: 2e-5 of the scale for y, 5e-5 for dx,
dgamma, dbeta, and 2e-6 of the larger of the scale and the per-channel sum of |dx| for dbias (true value 0); bf16 outputs (y, dx)
add 2^-8.  The data keeps every pre-activation value at least 2e-6 from the activation's kink (where the derivative jumps; fp32 and
fp64 may fall on different sides), by drawing a new seed.

In every variant the batch sums (dgamma, dbeta, dbias) written by the ticketed launch equal the per-plane partials added in order
b = 0..B-1, bit for bit (the property test_fused_backward_batch_sums_come_from_the_same_launch checks on six shapes).
"""
import pytest
import torch

pytestmark = pytest.mark.gpu

IPSR_ERR_INVALID, IPSR_ERR_UNSUPPORTED = -1, -2
ACT = {"none": 0, "relu": 1, "leaky": 2}
CONFIGS = [("none", True, True), ("relu", False, True), ("leaky", True, False)]

# (H, W): non-square planes at and around every capacity edge
PLANES = {3: (1, 3), 4: (2, 2), 255: (15, 17), 256: (8, 32), 257: (1, 257), 260: (10, 26), 1023: (31, 33), 1024: (16, 64),
          1025: (25, 41), 1028: (4, 257), 4095: (63, 65), 4096: (32, 128), 4097: (17, 241), 4100: (41, 100), 16383: (127, 129),
          16384: (64, 256), 16388: (4, 4097), 65536: (128, 512)}


def variant(HW):
    """(T, E, vector) the launcher picks: `in_dispatch` of instnorm.hip (the 512 x 128 form above IN_MAX_HW_REG = 16384)."""
    if HW > 65536 or HW < 2:
        return None
    if HW > 16384:
        return (512, 128, True) if HW % 4 == 0 else None
    vec = HW % 4 == 0
    for cap, T, E in ((256, 64, 4), (1024, 64, 16), (4096, 256, 16), (16384, 256, 64)):
        if HW <= cap:
            return T, E, vec


def _act64(t, act):
    if act == "relu":
        return torch.relu(t)
    if act == "leaky":
        return torch.nn.functional.leaky_relu(t, 0.2)
    return t


def _draw(B, C, H, W, dtype, act, affine, with_bias, seed):
    """Operands whose pre-activation stays >= 2e-6 from the kink (any value for act = none)."""
    for s in range(seed, seed + 64):
        g = torch.Generator().manual_seed(s)
        x = (torch.randn(B, C, H, W, generator=g) * 2 + 0.5).to(dtype)
        dy = torch.randn(B, C, H, W, generator=g).to(dtype)
        bias = torch.randn(C, generator=g) if with_bias else None
        gamma = torch.rand(C, generator=g) + 0.5 if affine else None
        beta = torch.randn(C, generator=g) if affine else None
        u = torch.nn.functional.instance_norm(x.double() + (bias.double().view(1, -1, 1, 1) if with_bias else 0), None, None,
                                              gamma.double() if affine else None, beta.double() if affine else None, True, 0.1, 1e-5)
        if act == "none" or float(u.abs().min()) >= 2e-6:
            return x, dy, bias, gamma, beta
    raise AssertionError("no seed keeps the data away from the activation's kink")


def _ref64(x, dy, bias, gamma, beta, act):
    C = x.shape[1]
    x64 = x.double().requires_grad_(True)
    b64 = (bias.double() if bias is not None else torch.zeros(C, dtype=torch.float64)).requires_grad_(True)
    g64 = (gamma.double() if gamma is not None else torch.ones(C, dtype=torch.float64)).requires_grad_(True)
    be64 = (beta.double() if beta is not None else torch.zeros(C, dtype=torch.float64)).requires_grad_(True)
    y = _act64(torch.nn.functional.instance_norm(x64 + b64.view(1, -1, 1, 1), None, None, g64, be64, True, 0.1, 1e-5), act)
    dx, dg, db, dbias = torch.autograd.grad(y, (x64, g64, be64, b64), dy.double())
    return y.detach(), dx, dg, db, dbias


def _err(a, b):
    return float((a.double().cpu() - b).abs().max()), max(1.0, float(b.abs().max()))


def _run(HW_case, dtype, act, affine, with_bias, seed):
    from deepinpainting_amd import _lib, ops
    L = _lib.lib()
    H, W = PLANES[HW_case]
    B, C = (2, 3) if HW_case > 4096 else (3, 8)
    bf = dtype == torch.bfloat16
    x, dy, bias, gamma, beta = _draw(B, C, H, W, dtype, act, affine, with_bias, seed)
    y64, dx64, dg64, db64, dbias64 = _ref64(x, dy, bias, gamma, beta, act)
    xd, dyd = x.cuda(), dy.cuda()
    bd, gd, bed = (t.cuda() if t is not None else None for t in (bias, gamma, beta))
    y, mean, rstd, tickets = ops.instnorm_act_forward(xd, bd, gd, bed, 1e-5, act, 0.2, return_tickets=True)
    dx = torch.empty_like(xd)
    part = torch.full((3, B, C), float("nan"), device="cuda")
    sums = torch.full((3, C), float("nan"), device="cuda")
    _lib.check(L.ipsr_instnorm_act_backward(dyd.data_ptr(), y.data_ptr(), xd.data_ptr(), ops._ptr(bd), ops._ptr(gd), mean.data_ptr(),
                                            rstd.data_ptr(), ACT[act], 0.2, B, C, H * W, int(bf), dx.data_ptr(), part[0].data_ptr(),
                                            part[1].data_ptr(), part[2].data_ptr(), sums.data_ptr(), tickets.data_ptr(), ops._stream()),
               "ipsr_instnorm_act_backward")
    torch.cuda.synchronize()
    assert y.dtype == dtype and dx.dtype == dtype
    # the batch sums of the ticketed launch == the partials added in order b = 0..B-1 (fp32), bit for bit
    ordered = torch.zeros_like(part[:, 0, :])
    for b in range(B):
        ordered = ordered + part[:, b, :]
    assert torch.equal(sums, ordered), (HW_case, dtype, act)
    assert int(tickets.abs().max()) == 0
    extra = 2.0 ** -8 if bf else 0.0
    e, s = _err(y, y64)
    assert e <= (2e-5 + extra) * s, ("y", HW_case, dtype, act, affine, with_bias, e / s)
    e, s = _err(dx, dx64)
    assert e <= (5e-5 + extra) * s, ("dx", HW_case, dtype, act, affine, with_bias, e / s)
    for name, got, want in (("dgamma", sums[0], dg64), ("dbeta", sums[1], db64)):
        e, s = _err(got, want)
        assert e <= 5e-5 * s, (name, HW_case, dtype, act, affine, with_bias, e / s)
    e, s = _err(sums[2], dbias64)
    s = max(s, float(dx64.abs().sum(dim=(0, 2, 3)).max()))
    assert e <= 2e-6 * s, ("dbias", HW_case, dtype, act, affine, with_bias, e / s)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("HW", sorted(PLANES), ids=["hw%d" % k for k in sorted(PLANES)])
def test_every_launch_variant_vs_fp64(HW, dtype):
    v = variant(HW)
    assert v is not None and v[2] == (HW % 4 == 0)
    T, E, _ = v
    # at a capacity edge, one past it (a ragged last pass of the next regime), or just below: never silently in a neighbour
    assert (T * E) // 4 < HW <= T * E or (T, E) == (64, 4), (HW, v)
    for i, (act, affine, with_bias) in enumerate(CONFIGS):
        _run(HW, dtype, act, affine, with_bias, seed=HW * 8 + i)


def test_every_variant_is_reached():
    """The cases above reach all nine launch shapes, in both forms where both exist, at their capacity edge."""
    got = {variant(hw) for hw in PLANES}
    assert got == {(64, 4, False), (64, 4, True), (64, 16, False), (64, 16, True), (256, 16, False), (256, 16, True),
                   (256, 64, False), (256, 64, True), (512, 128, True)}
    for T, E in ((64, 4), (64, 16), (256, 16), (256, 64), (512, 128)):
        assert T * E in PLANES                                              # the capacity edge itself
        assert T * E == 65536 or (T * E + 1 in PLANES or T * E + 4 in PLANES)   # one past it (16385 is refused: 16388)


def _nan_like(shape, dtype):
    t = torch.empty(shape, dtype=dtype, device="cuda")
    t.view(torch.int16 if dtype == torch.bfloat16 else torch.int32).fill_(0x7FC1 if dtype == torch.bfloat16 else 0x7FC00DAD)
    return t


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("H,W,code", [(1, 1, IPSR_ERR_INVALID), (5, 3277, IPSR_ERR_UNSUPPORTED), (5, 13108, IPSR_ERR_UNSUPPORTED)],
                         ids=["refuse_hw1", "refuse_hw16385", "refuse_hw65540"])
def test_refused_planes_write_nothing(H, W, code, dtype):
    """HW = 1 (no variance), 16385 (scalar above the register limit) and 65540 (above the largest plane): the forward and the backward
    return the error and leave every output, pre-filled with a NaN pattern, bitwise unchanged."""
    from deepinpainting_amd import _lib, ops
    L = _lib.lib()
    HW = H * W
    assert variant(HW) is None
    B, C = 2, 3
    bf = int(dtype == torch.bfloat16)
    x = torch.randn(B, C, H, W, device="cuda").to(dtype)
    dy = torch.randn(B, C, H, W, device="cuda").to(dtype)
    bias, gamma, beta = (torch.randn(C, device="cuda") for _ in range(3))
    y = _nan_like((B, C, H, W), dtype)
    stats = _nan_like((2 * B * C + C,), torch.float32)
    mean, rstd, tickets = stats[:B * C], stats[B * C:2 * B * C], stats[2 * B * C:]
    dx = _nan_like((B, C, H, W), dtype)
    part = _nan_like((3, B, C), torch.float32)
    sums = _nan_like((3, C), torch.float32)
    keep = [t.clone() for t in (y, stats, dx, part, sums)]
    torch.cuda.synchronize()
    rc = L.ipsr_instnorm_act_forward(x.data_ptr(), bias.data_ptr(), gamma.data_ptr(), beta.data_ptr(), 1e-5, 2, 0.2, B, C, HW, bf,
                                     y.data_ptr(), mean.data_ptr(), rstd.data_ptr(), tickets.data_ptr(), ops._stream())
    assert rc == code, (rc, L.ipsr_last_error())
    rc = L.ipsr_instnorm_act_backward(dy.data_ptr(), y.data_ptr(), x.data_ptr(), bias.data_ptr(), gamma.data_ptr(), mean.data_ptr(),
                                      rstd.data_ptr(), 2, 0.2, B, C, HW, bf, dx.data_ptr(), part[0].data_ptr(), part[1].data_ptr(),
                                      part[2].data_ptr(), sums.data_ptr(), tickets.data_ptr(), ops._stream())
    torch.cuda.synchronize()
    assert rc == code, (rc, L.ipsr_last_error())
    for name, a, b in zip(("y", "mean/rstd/tickets", "dx", "partials", "sums"), (y, stats, dx, part, sums), keep):
        assert torch.equal(a.view(torch.uint8), b.view(torch.uint8)), "%s was written by a refused call" % name
