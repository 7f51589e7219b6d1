"""The pointwise glue kernels (csrc/pointwise.hip, bias_act_bwd_kernel of csrc/instnorm.hip) in every launch form, bit for bit.

Each kernel has a vector form (16-byte accesses: HW % 4 == 0, for the pool W % 4 == 0) and a scalar form, each on fp32 and bf16
tensors, and walks its plane in a grid-stride loop: a workgroup has 256 threads and the grid is sized for about 4 trips per thread
(2 for the pool); bias_act_bwd_kernel gives one 256-thread workgroup a whole plane.

  kernel / form                     selected at                                 case ids (each in fp32 and bf16)
  --------------------------------  ------------------------------------------  -------------------------------------------------------------
  bias_act_kernel vector            pointwise.hip:39, launch_bias_act           hw4, hw1024, hw4096 (one workgroup, four full trips), hw4100
  bias_act_kernel scalar            pointwise.hip:49, launch_bias_act           hw1, hw3, hw1023, hw1025, hw4097
    second output y2 (slice)        pointwise.hip:38                            the same, through ipsr_bias_act_skip
  bias_act_bwd_kernel vector        instnorm.hip:311                            hw4, hw256, hw1020, hw1024, hw1028, hw4100
  bias_act_bwd_kernel scalar        instnorm.hip:327                            hw1, hw3, hw255, hw1023 (four trips)
    dy2 (slice)                     instnorm.hip:309                            the same, through ipsr_bias_act_backward_skip
  cat_relu_{fwd,bwd}_kernel vector  pointwise.hip:106 / :129, cat_relu_gx       c5+3 and c2+7 at hw4 .. hw4100
  cat_relu_{fwd,bwd}_kernel scalar  pointwise.hip:113 / :138, cat_relu_gx       c5+3 and c2+7 at hw1 .. hw4097
    y == NULL / dy == NULL          pointwise.hip:108, :114 / :131, :139        the same cases
  bias_relu_pool2_kernel vector     pointwise.hip:68, launch_bias_relu_pool2    2x4, 5x8, 64x32, 66x64 (second workgroup)
  bias_relu_pool2_kernel scalar     pointwise.hip:81, launch_bias_relu_pool2    2x2, 3x5, 7x9, 6x6 (even W, W % 4 == 2), 35x66 (second workgroup)
  refused: > 65535 planes / batch   the four launchers of pointwise.hip         refuse_* (UNSUPPORTED)
  refused: act, alignment, strides  api.hip:431-473, :525-543, launch_bias_act  refuse_* (INVALID)

Reference: these kernels do one add, one compare and one rounding per element, so the reference is the same expression evaluated by
torch on the CPU in fp32 (bf16 inputs upcast, fp32 arithmetic, one rounding to bf16) and the comparison is bit for bit.  The backward
is dx = dy * act'(y) + dy2 * relu'(y) with masks 0 / 1 / slope taken from y > 0, so the sum rounds once.  The one tolerance is the
bias-gradient partial, an fp32 sum: against the fp64 sum of the plane's fp32 dx it keeps within L * 2^-24 * sum |dx| with
L = ceil(HW / 256) + 12, an upper bound on the longest chain of additions (a thread's strided terms, six shuffle steps, four wave
partials, and the grouping inside a vector); every case prints its ratio to that bound (pytest -s; worst seen on an MI355X over the
120 bias-gradient cases: 0.097).  The batch sums equal the partials added in order b = 0..B-1, bitwise.

NaN and infinity (pointwise.hip:15-17, instnorm.hip:73): relu, leaky relu and the pooling maximum propagate NaN as torch does; the
backward's mask is `y > 0` (a NaN output selects 0 / slope).  One case per kernel holds NaN, +inf, -inf and -0.0 and is compared with
torch on the CPU on the NaN mask and on the remaining values.
"""
import math
import zlib

import pytest
import torch

from test_gpu_norm_variants import IPSR_ERR_INVALID, IPSR_ERR_UNSUPPORTED, _nan_like

gpu = pytest.mark.gpu

ACTS = {"none": 0, "relu": 1, "leaky": 2}
SLOPE = 0.2
DTYPES = [torch.float32, torch.bfloat16]
DTYPE_IDS = ["fp32", "bf16"]
HW_VECTOR, HW_SCALAR = (4, 1024, 4096, 4100), (1, 3, 1023, 1025, 4097)
HW_FWD = sorted(HW_VECTOR + HW_SCALAR)
HW_BWD = (1, 3, 4, 255, 256, 1020, 1023, 1024, 1028, 4100)     # 1023: the scalar form with several trips
CAT_CHANNELS = ((5, 3), (2, 7))
POOL_PLANES = ((2, 2), (2, 4), (3, 5), (7, 9), (6, 6), (5, 8), (64, 32), (66, 64), (35, 66))
B_C = (3, 5)                  # planes of the bias kernels: C is no multiple of anything convenient
Y2_AT, Y2_EXTRA = 1, 3        # y2 / dy2: channels [1, 1 + C) of C + 3
TICKET_WORD = 0x5A5A5A5A


def _cdiv(a, b):
    return (a + b - 1) // b


def _loop(per, per_wg_trips):
    """(workgroups, most trips of a thread, ragged last trip) of a grid-stride loop over `per` items, 256 threads a workgroup."""
    gx = max(1, _cdiv(per, 256 * per_wg_trips))
    return gx, _cdiv(per, gx * 256), per % (gx * 256) != 0


def bias_act_variant(HW):
    """(vector, workgroups, trips, ragged): pointwise.hip:39 and launch_bias_act."""
    vec = HW % 4 == 0
    return (vec,) + _loop(HW // 4 if vec else HW, 4)


def cat_relu_variant(C1, C2, HW):
    """pointwise.hip:106 / :129 and launch_cat_relu_{fwd,bwd} (cat_relu_gx): one grid row walks a sample's C1 + C2 planes."""
    vec = HW % 4 == 0
    n = (C1 + C2) * HW
    return (vec,) + _loop(n // 4 if vec else n, 4)


def pool_variant(H, W):
    """pointwise.hip:68 and launch_bias_relu_pool2: a thread of the vector form writes two adjacent outputs."""
    vec = W % 4 == 0
    Ho, Wo = H // 2, W // 2
    return (vec,) + _loop(Ho * (Wo // 2) if vec else Ho * Wo, 2)


def bias_act_bwd_variant(HW):
    """instnorm.hip:311-334: one 256-thread workgroup per plane."""
    vec = HW % 4 == 0
    per = HW // 4 if vec else HW
    return vec, 1, _cdiv(per, 256), per % 256 != 0


def _bits(t):
    return t.contiguous().view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32)


def _same(gpu_t, cpu_t):
    return gpu_t.dtype == cpu_t.dtype and gpu_t.shape == cpu_t.shape and torch.equal(_bits(gpu_t).cpu(), _bits(cpu_t))


def _same_nan(gpu_t, cpu_t):
    """Equal NaN masks, equal values elsewhere (torch on the CPU is the reference of both)."""
    a, b = gpu_t.cpu().float(), cpu_t.float()
    return a.shape == b.shape and torch.equal(torch.isnan(a), torch.isnan(b)) and torch.equal(torch.nan_to_num(a, nan=7.0), torch.nan_to_num(b, nan=7.0))


def _act32(v, act):
    if act == "relu":
        return torch.relu(v)
    if act == "leaky":
        return torch.where(v < 0, v * SLOPE, v)
    return v


def _mask32(y, act):
    """act'(y) from the output, as fp32 0 / 1 / slope."""
    one = torch.ones_like(y)
    if act == "relu":
        return torch.where(y > 0, one, torch.zeros_like(y))
    if act == "leaky":
        return torch.where(y > 0, one, torch.full_like(y, SLOPE))
    return one


def _gen(*key):
    return torch.Generator().manual_seed(zlib.crc32(repr(key).encode()))


def _rand(g, shape, dtype):
    return torch.randn(shape, generator=g).to(dtype)


def _wide_nan(t, at, extra):
    """t [B,C,HW] in channels [at, at + C) of a NaN-filled tensor with `extra` more channels -> (wide, slice pointer, batch stride)."""
    B, C, HW = t.shape
    w = _nan_like((B, C + extra, HW), t.dtype)
    w[:, at:at + C] = t
    return w, w.data_ptr() + at * HW * w.element_size(), (C + extra) * HW


def _outside_untouched(wide, at, C, what):
    pat = _nan_like((1,), wide.dtype)
    for part in (wide[:, :at], wide[:, at + C:]):
        assert bool((_bits(part) == _bits(pat)).all()), "%s: channels outside the slice were written" % what


def _tickets(C):
    return torch.full((C,), TICKET_WORD, dtype=torch.int32, device="cuda")


def _api():
    from deepinpainting_amd import _lib, ops
    return _lib.lib(), ops._stream()


def _ok(L, rc):
    assert rc == 0, (rc, L.ipsr_last_error())


# ---- ipsr_bias_act / ipsr_bias_act_skip ----

def _bias_act_case(x, bias, act, check):
    """x [B,C,HW] on the CPU: the plain entry (tickets given, tickets NULL) and the skip entry against act(x + bias) in fp32."""
    L, st = _api()
    B, C, HW = x.shape
    bf = int(x.dtype == torch.bfloat16)
    v = x.float() + (bias.view(1, -1, 1) if bias is not None else 0)
    want, want2 = _act32(v, act).to(x.dtype), torch.relu(v).to(x.dtype)
    bd = bias.cuda() if bias is not None else None
    bp = bd.data_ptr() if bd is not None else None
    for with_tickets in (True, False):
        xd, tk = x.cuda(), _tickets(C) if with_tickets else None
        _ok(L, L.ipsr_bias_act(xd.data_ptr(), bp, B, C, HW, ACTS[act], SLOPE, bf, tk.data_ptr() if with_tickets else None, st))
        torch.cuda.synchronize()
        assert check(xd, want), ("bias_act", act, HW, x.dtype)
        assert tk is None or int(tk.abs().max()) == 0, "the forward leaves the ticket words zero"
    xd, tk = x.cuda(), _tickets(C)
    wide, y2p, y2bs = _wide_nan(torch.zeros_like(xd), Y2_AT, Y2_EXTRA)
    _ok(L, L.ipsr_bias_act_skip(xd.data_ptr(), bp, B, C, HW, ACTS[act], SLOPE, bf, y2p, y2bs, tk.data_ptr(), st))
    torch.cuda.synchronize()
    assert check(xd, want), ("bias_act_skip x", act, HW, x.dtype)
    assert check(wide[:, Y2_AT:Y2_AT + C], want2), ("bias_act_skip y2", act, HW, x.dtype)
    _outside_untouched(wide, Y2_AT, C, "bias_act_skip y2")
    assert int(tk.abs().max()) == 0


@gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=DTYPE_IDS)
@pytest.mark.parametrize("HW", HW_FWD, ids=["hw%d" % k for k in HW_FWD])
def test_bias_act_and_skip_bit_exact(HW, dtype):
    vec, gx, trips, ragged = bias_act_variant(HW)
    assert vec == (HW in HW_VECTOR) and (gx > 1) == (HW in (1025, 4097, 4100)) and trips <= 4
    B, C = B_C
    g = _gen("bias_act", HW)
    x, bias = _rand(g, (B, C, HW), dtype), torch.randn(C, generator=g)
    for act in ACTS:
        _bias_act_case(x, bias, act, _same)
    _bias_act_case(x, None, "leaky", _same)          # bias = NULL


# ---- ipsr_bias_act_backward / ipsr_bias_act_backward_skip ----

_worst_ratio = {"value": 0.0}


def _bias_act_bwd_case(dy, dy2, y, act, need_bias, check):
    L, st = _api()
    B, C, HW = y.shape
    bf = int(y.dtype == torch.bfloat16)
    r32 = dy.float() * _mask32(y.float(), act)
    if dy2 is not None:
        r32 = r32 + dy2.float() * _mask32(y.float(), "relu")
    dyd, yd = dy.cuda(), y.cuda()
    dx = _nan_like((B, C, HW), y.dtype)
    part, sums = _nan_like((B, C), torch.float32), _nan_like((C,), torch.float32)
    tk = torch.zeros(C, dtype=torch.int32, device="cuda")          # as the matching forward leaves them (checked above)
    tail = (ACTS[act], SLOPE, B, C, HW, bf, dx.data_ptr()) + ((part.data_ptr(), sums.data_ptr(), tk.data_ptr()) if need_bias else (None, None, None)) + (st,)
    if dy2 is None:
        _ok(L, L.ipsr_bias_act_backward(dyd.data_ptr(), yd.data_ptr(), *tail))
    else:
        wide, d2p, d2bs = _wide_nan(dy2.cuda(), Y2_AT, Y2_EXTRA)
        keep = wide.clone()
        _ok(L, L.ipsr_bias_act_backward_skip(dyd.data_ptr(), d2p, d2bs, yd.data_ptr(), *tail))
    torch.cuda.synchronize()
    where = (act, HW, y.dtype, dy2 is not None, need_bias)
    assert check(dx, r32.to(y.dtype)), ("dx",) + where
    if dy2 is not None:
        assert torch.equal(_bits(wide), _bits(keep)), "dy2 was written"
    if not need_bias:
        return
    ordered = torch.zeros_like(sums)
    for b in range(B):
        ordered = ordered + part[b]
    assert torch.equal(_bits(sums), _bits(ordered)), ("sums != ordered partials",) + where
    assert int(tk.abs().max()) == 0
    if check is _same:
        want = r32.double().sum(dim=2)
        bound = (_cdiv(HW, 256) + 12) * 2.0 ** -24 * r32.double().abs().sum(dim=2)
        err = (part.cpu().double() - want).abs()
        ratio = float((err / bound.clamp_min(1e-300)).max())
        _worst_ratio["value"] = max(_worst_ratio["value"], ratio)
        print("bias_act_backward dbias partial: error / bound = %.3f (%s hw%d %s dy2=%s), worst so far %.3f"
              % (ratio, act, HW, str(y.dtype).split(".")[-1], dy2 is not None, _worst_ratio["value"]))
        assert bool((err <= bound).all()), ("dbias partial", ratio) + where


@gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=DTYPE_IDS)
@pytest.mark.parametrize("HW", HW_BWD, ids=["hw%d" % k for k in HW_BWD])
def test_bias_act_backward_and_skip_bit_exact(HW, dtype):
    vec, gx, trips, ragged = bias_act_bwd_variant(HW)
    assert vec == (HW % 4 == 0) and gx == 1 and trips == _cdiv(HW // 4 if vec else HW, 256)
    B, C = B_C
    g = _gen("bias_act_bwd", HW)
    dy, dy2, pre = (_rand(g, (B, C, HW), dtype) for _ in range(3))
    for act in ACTS:
        y = _act32(pre.float(), act).to(dtype)        # an output of the forward: zeros where relu cut
        for with_dy2 in (False, True):
            for need_bias in (True, False):
                _bias_act_bwd_case(dy, dy2 if with_dy2 else None, y, act, need_bias, _same)


# ---- ipsr_cat_relu_forward / ipsr_cat_relu_backward ----

def _cat_relu_case(y, x, g, check):
    """y [B,C1,HW], x [B,C2,HW], g [B,C1+C2,HW] on the CPU: the full and the half-only forms of both directions."""
    L, st = _api()
    (B, C1, HW), C2 = y.shape, x.shape[1]
    dtype, bf = y.dtype, int(y.dtype == torch.bfloat16)
    want = torch.relu(torch.cat([y.float(), x.float()], 1)).to(dtype)
    yd, xd, gd = y.cuda(), x.cuda(), g.cuda()
    where = (C1, C2, HW, dtype)
    out = _nan_like((B, C1 + C2, HW), dtype)
    _ok(L, L.ipsr_cat_relu_forward(yd.data_ptr(), xd.data_ptr(), B, C1, C2, HW, bf, out.data_ptr(), st))
    torch.cuda.synchronize()
    assert check(out, want), ("cat_relu forward",) + where
    # y == NULL: the first C1 channels (a known pattern) stay, the skip half is exact
    half = _nan_like((B, C1 + C2, HW), dtype)
    _ok(L, L.ipsr_cat_relu_forward(None, xd.data_ptr(), B, C1, C2, HW, bf, half.data_ptr(), st))
    torch.cuda.synchronize()
    assert check(half[:, C1:], want[:, C1:]), ("cat_relu forward, y == NULL",) + where
    assert bool((_bits(half[:, :C1]) == _bits(_nan_like((1,), dtype))).all()), ("y == NULL wrote the first half",) + where
    # backward: the mask from `out` (bit-identical to `want` unless NaN is about), the two channel slices
    od = want.cuda()
    r = torch.where(want.float() > 0, g.float(), torch.zeros_like(g.float())).to(dtype)
    dy, dx = _nan_like((B, C1, HW), dtype), _nan_like((B, C2, HW), dtype)
    _ok(L, L.ipsr_cat_relu_backward(gd.data_ptr(), od.data_ptr(), B, C1, C2, HW, bf, dy.data_ptr(), dx.data_ptr(), st))
    torch.cuda.synchronize()
    assert check(dy, r[:, :C1].contiguous()) and check(dx, r[:, C1:].contiguous()), ("cat_relu backward",) + where
    dx2 = _nan_like((B, C2, HW), dtype)
    _ok(L, L.ipsr_cat_relu_backward(gd.data_ptr(), od.data_ptr(), B, C1, C2, HW, bf, None, dx2.data_ptr(), st))
    torch.cuda.synchronize()
    assert check(dx2, r[:, C1:].contiguous()), ("cat_relu backward, dy == NULL",) + where
    assert torch.equal(_bits(gd).cpu(), _bits(g)) and torch.equal(_bits(od).cpu(), _bits(want)), "the backward wrote an operand"


@gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=DTYPE_IDS)
@pytest.mark.parametrize("C1,C2", CAT_CHANNELS, ids=["c%d+%d" % c for c in CAT_CHANNELS])
@pytest.mark.parametrize("HW", HW_FWD, ids=["hw%d" % k for k in HW_FWD])
def test_cat_relu_full_and_half_forms_bit_exact(HW, C1, C2, dtype):
    vec, gx, trips, ragged = cat_relu_variant(C1, C2, HW)
    assert vec == (HW in HW_VECTOR) and gx == max(1, _cdiv((C1 + C2) * HW // (4 if vec else 1), 1024)) and trips <= 4
    B = 3
    g = _gen("cat_relu", HW, C1)
    _cat_relu_case(_rand(g, (B, C1, HW), dtype), _rand(g, (B, C2, HW), dtype), _rand(g, (B, C1 + C2, HW), dtype), _same)


# ---- ipsr_bias_relu_pool2 ----

def _pool_case(x, bias, check):
    L, st = _api()
    B, C, H, W = x.shape
    bf = int(x.dtype == torch.bfloat16)
    v = x.float() + (bias.view(1, -1, 1, 1) if bias is not None else 0)
    want = torch.nn.functional.max_pool2d(torch.relu(v), 2, 2).to(x.dtype)
    n = want.numel()
    xd, bd = x.cuda(), bias.cuda() if bias is not None else None
    buf = _nan_like((n + 64,), x.dtype)               # 64 elements behind the result: an extra row or column would land there
    _ok(L, L.ipsr_bias_relu_pool2(xd.data_ptr(), bd.data_ptr() if bd is not None else None, B, C, H, W, bf, buf.data_ptr(), st))
    torch.cuda.synchronize()
    assert check(buf[:n].view(want.shape), want), ("bias_relu_pool2", H, W, x.dtype, bias is not None)
    assert bool((_bits(buf[n:]) == _bits(_nan_like((1,), x.dtype))).all()), "bias_relu_pool2 wrote behind its result"
    assert torch.equal(_bits(xd).cpu(), _bits(x)), "bias_relu_pool2 wrote its input"


@gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=DTYPE_IDS)
@pytest.mark.parametrize("H,W", POOL_PLANES, ids=["%dx%d" % p for p in POOL_PLANES])
def test_bias_relu_pool2_bit_exact(H, W, dtype):
    vec, gx, trips, ragged = pool_variant(H, W)
    assert vec == (W % 4 == 0) and (gx > 1) == ((H, W) in ((66, 64), (35, 66))) and trips <= 2
    B, C = 2, 3
    g = _gen("pool", H, W)
    x, bias = _rand(g, (B, C, H, W), dtype), torch.randn(C, generator=g)
    _pool_case(x, bias, _same)
    _pool_case(x, None, _same)                        # bias = NULL


# ---- NaN, infinity, -0.0 ----

def _specials(t, g):
    """A quarter of t's elements replaced by NaN, +inf, -inf and -0.0 in turn."""
    flat = t.clone().view(-1)
    idx = torch.randperm(flat.numel(), generator=g)[:max(4, flat.numel() // 4)]
    vals = torch.tensor([float("nan"), float("inf"), float("-inf"), -0.0]).to(t.dtype)
    flat[idx] = vals[torch.arange(idx.numel()) % 4]
    return flat.view(t.shape)


@gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=DTYPE_IDS)
@pytest.mark.parametrize("HW", [36, 35], ids=["vector", "scalar"])
def test_nan_and_infinity_propagate_as_in_torch(HW, dtype):
    """Every kernel on operands that hold NaN, +inf, -inf and -0.0, against the same expression by torch on the CPU: the same NaN
    mask, the same values elsewhere."""
    B, C = B_C
    g = _gen("nan", HW)
    x = _specials(_rand(g, (B, C, HW), dtype), g)
    bias = torch.randn(C, generator=g)
    for act in ACTS:
        _bias_act_case(x, bias, act, _same_nan)
        _bias_act_case(x, None, act, _same_nan)       # -0.0 survives a missing bias
    dy, dy2, y = (_specials(_rand(g, (B, C, HW), dtype), g) for _ in range(3))
    for act in ACTS:
        for d2 in (None, dy2):
            _bias_act_bwd_case(dy, d2, y, act, False, _same_nan)
    C1, C2 = CAT_CHANNELS[0]
    _cat_relu_case(_specials(_rand(g, (B, C1, HW), dtype), g), _specials(_rand(g, (B, C2, HW), dtype), g),
                   _specials(_rand(g, (B, C1 + C2, HW), dtype), g), _same_nan)
    # the pool: NaN at each of the four window positions in turn (and one window with +inf, one with -inf only, one with -0.0)
    for H, W in ((4, 8), (5, 6)):
        xp = _rand(g, (2, 2, H, W), dtype)
        for k, (di, dj) in enumerate(((0, 0), (0, 1), (1, 0), (1, 1))):
            xp[k // 2, k % 2, di, dj] = float("nan")          # window (0, 0) of plane k
            xp[k // 2, k % 2, 2 + di, 2 + dj] = float("nan")  # window (1, 1)
        xp[0, 0, 0, 2] = float("inf")
        xp[0, 1, 0:2, 2:4] = float("-inf")
        xp[1, 0, 0:2, 2:4] = -0.0
        _pool_case(xp, None, _same_nan)
        _pool_case(xp, torch.randn(2, generator=g), _same_nan)


# ---- refusals ----

def _unchanged(pairs):
    torch.cuda.synchronize()
    for name, t, keep in pairs:
        assert torch.equal(t.view(torch.uint8), keep.view(torch.uint8)), "%s was written by a refused call" % name


@gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=DTYPE_IDS)
def test_refused_plane_and_batch_counts_write_nothing(dtype):
    """More than 65535 planes (the grid's second dimension) or samples: IPSR_ERR_UNSUPPORTED, nothing written.  HW = 1 keeps the
    tensors tiny."""
    L, st = _api()
    bf = int(dtype == torch.bfloat16)
    N = 65536
    x, x4, y, out, half, dx, dy = (_nan_like((n,), dtype) for n in (N, 4 * N, N, 2 * N, N, N, N))
    bias = torch.zeros(N, device="cuda")
    keep = [(name, t, t.clone()) for name, t in (("x", x), ("x4", x4), ("y", y), ("out", out), ("half", half), ("dx", dx), ("dy", dy))]
    for B, C in ((1, N), (N, 1), (256, 256)):
        assert L.ipsr_bias_act(x.data_ptr(), bias.data_ptr(), B, C, 1, 1, SLOPE, bf, None, st) == IPSR_ERR_UNSUPPORTED, L.ipsr_last_error()
        assert L.ipsr_bias_act_skip(x.data_ptr(), bias.data_ptr(), B, C, 1, 1, SLOPE, bf, y.data_ptr(), C, None, st) == IPSR_ERR_UNSUPPORTED
        assert L.ipsr_bias_relu_pool2(x4.data_ptr(), bias.data_ptr(), B, C, 2, 2, bf, y.data_ptr(), st) == IPSR_ERR_UNSUPPORTED, L.ipsr_last_error()
    assert L.ipsr_cat_relu_forward(half.data_ptr(), x.data_ptr(), N, 1, 1, 1, bf, out.data_ptr(), st) == IPSR_ERR_UNSUPPORTED, L.ipsr_last_error()
    assert L.ipsr_cat_relu_forward(None, x.data_ptr(), N, 1, 1, 1, bf, out.data_ptr(), st) == IPSR_ERR_UNSUPPORTED
    assert L.ipsr_cat_relu_backward(out.data_ptr(), out.data_ptr(), N, 1, 1, 1, bf, dy.data_ptr(), dx.data_ptr(), st) == IPSR_ERR_UNSUPPORTED, L.ipsr_last_error()
    assert L.ipsr_cat_relu_backward(out.data_ptr(), out.data_ptr(), N, 1, 1, 1, bf, None, dx.data_ptr(), st) == IPSR_ERR_UNSUPPORTED
    _unchanged(keep)


@gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=DTYPE_IDS)
def test_refused_arguments_write_nothing(dtype):
    """IPSR_ERR_INVALID for an unknown activation, for a vector-sized plane behind a pointer one element off, for a y2 / dy2 batch
    stride below C*HW or (vector-sized plane) no multiple of 4, and for a one-row pool; nothing written."""
    L, st = _api()
    bf, es = int(dtype == torch.bfloat16), 2 if dtype == torch.bfloat16 else 4
    B, C, HW = 2, 3, 8
    n = B * C * HW
    # every tensor has HW spare elements, so "one element off" stays inside its allocation
    x, y2, dx, dyo, out = (_nan_like((m + HW,), dtype) for m in (n, B * (C + Y2_EXTRA) * HW, n, n, 2 * n))
    src = torch.randn(2 * n + HW, device="cuda").to(dtype)             # read-only operands
    bias = torch.zeros(C, device="cuda")
    part, sums, tk = _nan_like((B, C), torch.float32), _nan_like((C,), torch.float32), _nan_like((C,), torch.float32)
    outs = (("x", x), ("y2", y2), ("dx", dx), ("dy", dyo), ("out", out), ("partials", part), ("sums", sums), ("tickets", tk))
    keep = [(name, t, t.clone()) for name, t in outs]
    torch.cuda.synchronize()
    X, Y2, DX, DY, OUT, S = (t.data_ptr() for t in (x, y2, dx, dyo, out, src))
    y2bs = (C + Y2_EXTRA) * HW
    INV = IPSR_ERR_INVALID

    def red(rc):
        assert rc == INV, (rc, L.ipsr_last_error())
    for act in (3, -1):
        red(L.ipsr_bias_act(X, bias.data_ptr(), B, C, HW, act, SLOPE, bf, tk.data_ptr(), st))
        red(L.ipsr_bias_act_skip(X, bias.data_ptr(), B, C, HW, act, SLOPE, bf, Y2 + Y2_AT * HW * es, y2bs, tk.data_ptr(), st))
        red(L.ipsr_bias_act_backward(S, S, act, SLOPE, B, C, HW, bf, DX, part.data_ptr(), sums.data_ptr(), tk.data_ptr(), st))
        red(L.ipsr_bias_act_backward_skip(S, S, y2bs, S, act, SLOPE, B, C, HW, bf, DX, part.data_ptr(), sums.data_ptr(), tk.data_ptr(), st))
    # one element off
    red(L.ipsr_bias_act(X + es, bias.data_ptr(), B, C, HW, 1, SLOPE, bf, tk.data_ptr(), st))
    red(L.ipsr_bias_act_skip(X + es, bias.data_ptr(), B, C, HW, 1, SLOPE, bf, Y2 + Y2_AT * HW * es, y2bs, tk.data_ptr(), st))
    red(L.ipsr_bias_act_skip(X, bias.data_ptr(), B, C, HW, 1, SLOPE, bf, Y2 + (Y2_AT * HW + 1) * es, y2bs, tk.data_ptr(), st))
    for a, b, d in ((S + es, S, DX), (S, S + es, DX), (S, S, DX + es)):
        red(L.ipsr_bias_act_backward(a, b, 1, SLOPE, B, C, HW, bf, d, part.data_ptr(), sums.data_ptr(), tk.data_ptr(), st))
        red(L.ipsr_bias_act_backward_skip(a, S, y2bs, b, 1, SLOPE, B, C, HW, bf, d, part.data_ptr(), sums.data_ptr(), tk.data_ptr(), st))
    red(L.ipsr_bias_act_backward_skip(S, S + es, y2bs, S, 1, SLOPE, B, C, HW, bf, DX, part.data_ptr(), sums.data_ptr(), tk.data_ptr(), st))
    for a, b, o in ((S + es, S, OUT), (S, S + es, OUT), (S, S, OUT + es), (None, S + es, OUT), (None, S, OUT + es)):
        red(L.ipsr_cat_relu_forward(a, b, B, C, C, HW, bf, o, st))
    for a, b, p, q in ((S + es, S, DY, DX), (S, S + es, DY, DX), (S, S, DY + es, DX), (S, S, DY, DX + es), (S, S, None, DX + es)):
        red(L.ipsr_cat_relu_backward(a, b, B, C, C, HW, bf, p, q, st))
    red(L.ipsr_bias_relu_pool2(S + es, bias.data_ptr(), B, C, 2, 4, bf, OUT, st))
    # strides of the second output / second gradient
    for bad in (C * HW - 1, C * HW - 4, y2bs + 1, y2bs + 2):
        red(L.ipsr_bias_act_skip(X, bias.data_ptr(), B, C, HW, 1, SLOPE, bf, Y2 + Y2_AT * HW * es, bad, tk.data_ptr(), st))
        red(L.ipsr_bias_act_backward_skip(S, S, bad, S, 1, SLOPE, B, C, HW, bf, DX, part.data_ptr(), sums.data_ptr(), tk.data_ptr(), st))
    red(L.ipsr_bias_act_skip(X, bias.data_ptr(), B, C, HW - 1, 1, SLOPE, bf, Y2, C * (HW - 1) - 1, tk.data_ptr(), st))     # scalar-sized plane
    # batch sums without the partials or without the ticket words
    red(L.ipsr_bias_act_backward(S, S, 1, SLOPE, B, C, HW, bf, DX, part.data_ptr(), sums.data_ptr(), None, st))
    red(L.ipsr_bias_act_backward(S, S, 1, SLOPE, B, C, HW, bf, DX, None, sums.data_ptr(), tk.data_ptr(), st))
    # the pool needs two rows and two columns
    red(L.ipsr_bias_relu_pool2(S, bias.data_ptr(), B, C, 1, 8, bf, OUT, st))
    red(L.ipsr_bias_relu_pool2(S, bias.data_ptr(), B, C, 8, 1, bf, OUT, st))
    _unchanged(keep)


# ---- reach ----

def test_every_form_is_reached():
    """No GPU: from the restated launcher formulas, every kernel meets both forms, in fp32 and bf16, at one workgroup and at more than
    one (bias_act_bwd_kernel: one trip and several), each with a ragged last trip and with a full one."""
    both = {(vec, many) for vec in (False, True) for many in (False, True)}
    assert DTYPES == [torch.float32, torch.bfloat16]                     # every case list below is run in both

    def reach(variants):
        got = {(v[0], v[1] > 1) for v in variants}
        ragged = {(v[0], v[1] > 1) for v in variants if v[3]}
        return got, ragged
    got, ragged = reach([bias_act_variant(hw) for hw in HW_FWD])
    assert got == both and ragged == both
    assert bias_act_variant(4096) == (True, 1, 4, False)                 # exactly one workgroup with exactly four trips
    assert bias_act_variant(4100) == (True, 2, 3, True)                  # the first ragged size that needs a second workgroup
    assert bias_act_variant(1025)[1] == 2 and bias_act_variant(1023) == (False, 1, 4, True)
    for C1, C2 in CAT_CHANNELS:
        assert C1 != C2
        got, ragged = reach([cat_relu_variant(C1, C2, hw) for hw in HW_FWD])
        assert got == both and ragged == both, (C1, C2)
    got, ragged = reach([pool_variant(H, W) for H, W in POOL_PLANES])
    assert got == both and ragged == both
    assert pool_variant(64, 32) == (True, 1, 1, False) and pool_variant(66, 64)[1] == 2 and pool_variant(35, 66)[:2] == (False, 2)
    assert pool_variant(6, 6)[0] is False                                 # even W with W % 4 == 2 runs the scalar form
    assert {(H % 2, W % 2) for H, W in POOL_PLANES} >= {(0, 0), (1, 0), (1, 1)}             # odd H, odd H and W: last row / column dropped
    bwd = [bias_act_bwd_variant(hw) for hw in HW_BWD]
    assert all(v[1] == 1 for v in bwd)
    assert {(v[0], v[2] > 1) for v in bwd} == both                        # one trip and several, in both forms
    assert {(v[0], v[3]) for v in bwd} == {(True, True), (True, False), (False, True)}      # ragged and full last trips (scalar: always ragged)
    assert math.gcd(B_C[1], 4) == 1 and math.gcd(B_C[0] * B_C[1], 4) == 1
