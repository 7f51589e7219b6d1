"""The thin-layer and one-channel kernels of csrc/thin_conv.hip in every launch variant, against torch in fp64 on the GPU.

Every case goes through the `ops` wrappers (ops.py:812-974).  tests/thin_conv_plan.py restates the launchers and holds the case
tables; tests/test_thin_conv_plan.py proves without a GPU that the tables reach every row below, and each test here asserts its
own row again (`P.check_case`) before it compares numbers.

  variant                                                                            selected at                                        case ids
  ---------------------------------------------------------------------------------  -------------------------------------------------  ----------------------------------------
  thin_f2m_mfma_kernel<4,2>                                                          thin_f2m_mfma_plan (KS, MT)                        convT136_3_k3_b1_5x32
  thin_f2m_mfma_kernel<4,3>                                                          thin_f2m_mfma_plan (KS, MT)                        convT128_3_k4s2_b2_5x32
  thin_f2m_mfma_kernel<4,4>                                                          thin_f2m_mfma_plan (KS, MT)                        conv6_136_k3_b1_6x32
  thin_f2m_mfma_kernel<2,2>                                                          thin_f2m_mfma_plan (KS, MT)                        conv3_8_k3_b1_7x64, conv3_8_k3_b33_250x32
  thin_f2m_mfma_kernel<2,3>                                                          thin_f2m_mfma_plan (KS, MT)                        conv3_40_k4s2_b2_6x64
  thin_f2m_mfma_kernel<2,4>                                                          thin_f2m_mfma_plan (KS, MT)                        conv6_72_k3_b1_9x32
  thin_f2m_mfma_kernel<2,6>                                                          thin_f2m_mfma_plan (KS, MT)                        convT24_6_k4s2_b2_5x32
  thin_f2m_mfma_kernel: a second o tile with 8 live rows                             thin_f2m_mfma_plan (otiles), thin_f2m_mfma_kernel  conv6_136_k3_b1_6x32, conv6_72_k3_b1_9x32
                                                                                                                                        convT136_3_k3_b1_5x32
  thin_f2m_mfma_kernel: ragged last row group, a wave idle                           thin_f2m_mfma_kernel                               convT128_3_k4s2_b2_5x32, conv6_136_k3_b1_6x32
                                                                                                                                        conv3_8_k3_b1_7x64, conv3_40_k4s2_b2_6x64
  thin_f2m_mfma_kernel: two x segments per row                                       thin_f2m_mfma_kernel                               conv3_8_k3_b1_7x64
  thin_f2m_mfma_kernel: rows_per_wg 8, last group of 2 rows                          thin_f2m_mfma_plan (rows)                          conv3_8_k3_b33_250x32
  thin_wrw_mfma_kernel<4,1>                                                          thin_wrw_mfma_plan (RT, MT)                        kb136_cs3_k3_b2_5x16
  thin_wrw_mfma_kernel<4,2>                                                          thin_wrw_mfma_plan (RT, MT)                        kb128_cs3_k4_b1_6x48
  thin_wrw_mfma_kernel<2,1>                                                          thin_wrw_mfma_plan (RT, MT)                        kb8_cs3_k3_b2_7x80, kb8_cs3_k3_b17_242x16
  thin_wrw_mfma_kernel<2,2>                                                          thin_wrw_mfma_plan (RT, MT)                        kb72_cs6_k3_b1_5x16, kb8_cs6_k3_b9_230x16
  thin_wrw_mfma_kernel<2,3>                                                          thin_wrw_mfma_plan (RT, MT)                        kb24_cs6_k4_b2_6x16
  thin_wrw_mfma_kernel: ragged last row group at rows 4                              thin_wrw_mfma_kernel                               kb136_cs3_k3_b2_5x16, kb128_cs3_k4_b1_6x48
                                                                                                                                        kb8_cs3_k3_b2_7x80, kb72_cs6_k3_b1_5x16
                                                                                                                                        kb24_cs6_k4_b2_6x16
  thin_wrw_mfma_kernel: limit 1024 -> rows 8, last group of 2 rows                   thin_wrw_mfma_plan (rows)                          kb8_cs3_k3_b17_242x16
  thin_wrw_mfma_kernel: limit 512 -> rows 8, last group of 6 rows                    thin_wrw_mfma_plan (rows)                          kb8_cs6_k3_b9_230x16
  thin_wrw_mfma_kernel: two k tiles                                                  thin_wrw_mfma_plan (ktiles)                        kb136_cs3_k3_b2_5x16, kb72_cs6_k3_b1_5x16
  thin_f2m_kernel<3>, flip 0 and 1                                                   thin_f2m_plan (I), ops.conv3x3_thin                f2m_b2_3_16_1x2, f2m_b1_3_48_2x1026
  thin_f2m_kernel<6>, flip 0 and 1                                                   thin_f2m_plan (I), ops.conv3x3_thin                f2m_b1_6_32_3x514
  thin_f2m_kernel: more than one block on x, y and z                                 thin_f2m_plan (grid)                               f2m_b1_6_32_3x514, f2m_b1_3_48_2x1026
  thin_m2f_kernel<3>, flip 0 and 1                                                   thin_m2f_plan (O), ops.conv3x3_thin                m2f_b2_16_3_1x4, m2f_b1_455_3_2x8
  thin_m2f_kernel<6>, flip 0 and 1                                                   thin_m2f_plan (O), ops.conv3x3_thin                m2f_b1_18_6_5x260, m2f_b1_227_6_3x4
  thin_m2f_kernel: two blocks on x and y                                             thin_m2f_plan (grid)                               m2f_b1_18_6_5x260
  thin_m2f_kernel: two blocks on z                                                   thin_m2f_plan (grid)                               m2f_b2_16_3_1x4
  thin_m2f_kernel: the last I that fits the 48 KB of LDS                             thin_m2f_plan (lds_bytes)                          m2f_b1_455_3_2x8, m2f_b1_227_6_3x4
  thin_wrw_kernel<3>                                                                 thin_wrw_plan (Cs)                                 wrw_b1_2_3_1x4, wrw_b1_2_3_3x260
  thin_wrw_kernel<6>                                                                 thin_wrw_plan (Cs)                                 wrw_b2_4_6_65x8, wrw_b2_6_6_130x516
  thin_wrw_kernel: a second row block (H > 64)                                       thin_wrw_plan (grid)                               wrw_b2_4_6_65x8, wrw_b2_6_6_130x516
  thin_wrw_kernel: a second x block (W > 256)                                        thin_wrw_plan (grid)                               wrw_b1_2_3_3x260, wrw_b2_6_6_130x516
  thin_wrw_kernel: more than one block on x, y and z                                 thin_wrw_plan (grid)                               wrw_b2_6_6_130x516
  one_fwd_kernel<4> / one_wrw_kernel<4>: a 1 x 1 output                              to_one_plan (K)                                    one_b1_c1_4x4_k4p0
  one_fwd_kernel<4>: exactly 256 groups, a second chunk of one channel, two samples  to_one_plan, one_fwd_kernel                        one_b2_c9_33x33_k4p1
  one_fwd_kernel<3> / one_wrw_kernel<3>: pad 0, 224 groups                           to_one_plan (K)                                    one_b1_c8_34x30_k3p0
  one_fwd_kernel<3>: Wo % 4 != 0                                                     one_fwd_kernel                                     one_b2_c7_6x9_k3p1, one_b1_c5_5x5_k3p2
  one_fwd_kernel<3>: pad 2                                                           one_fwd_kernel                                     one_b1_c5_5x5_k3p2
  refused: few -> many at an odd width                          thin_f2m_plan            f2m_odd_w
  refused: many -> few one channel past the 48 KB of LDS        thin_m2f_plan            m2f_i456_o3, m2f_i228_o6
  refused: conv_to_one at 264 pixel groups                      to_one_plan              one_b1_c8_34x33_k4p1

Two data regimes per case, both against fp64:

(a) exact.  Activations are integers in [-3, 3], weights and bias in [-2, 2]: all bf16-representable.  The test first asserts that
the fp64 convolution of the absolute values (+ |bias|) stays below 2^24 — a condition on the data, held by orders of magnitude at
these shapes.  Then every product and every partial sum is an integer that fp32 holds exactly, in any order and on either
matrix-core path, so an fp32 result must equal the fp64 reference bit for bit and a bf16 result its round-to-nearest-even (`f2bf`
of ipsr_common.h).  A dropped, doubled or misplaced tap, row, channel or block changes an integer.

(b) real-valued.  Normal draws times a per-channel power of two in 2^-3 .. 2^3.  The reference is fp64 of exactly what the kernel
multiplies: an operand the kernel rounds to bf16 is rounded, one it keeps in fp32 is kept (each test's docstring names the rule
and its lines).  The band is elementwise: 2e-5 (conv_to_one: 5e-6; the constants tests/test_gpu_conv.py holds these kernels to)
times the fp64 convolution of the ABSOLUTE values (+ |bias|), plus 2^-8 |y64| for a bf16 result.  Each check prints its worst
|err| / band.

Weight gradients and conv_to_one give the same bits on a second call.  The most ragged cases of each entry point run once more
inside tests/guarded.py's Arena (guard bands around every tensor, NaN-filled scratch of exactly the size asked for): guards intact,
inputs unmodified, the same bits.  Refused calls leave a NaN-patterned output bitwise unchanged.
"""
import pytest
import torch
import torch.nn.functional as F

import thin_conv_plan as P
from guarded import Arena

pytestmark = pytest.mark.gpu

IPSR_ERR_UNSUPPORTED = -2
F32, BF16 = torch.float32, torch.bfloat16
BAND, BAND_ONE = 2e-5, 5e-6                               # tests/test_gpu_conv.py: the thin family, conv_to_one


def _bits(t):
    return t.contiguous().view(torch.int32 if t.element_size() == 4 else torch.int16)


def _same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(_bits(a), _bits(b))


def _gen(seed):
    return torch.Generator(device="cuda").manual_seed(seed)


def _draw(shape, g, exact, weight=False):
    """Regime (a): integers in [-3, 3] (activations) or [-2, 2] (weights, bias).  Regime (b): normal draws times a power of two in
    2^-3 .. 2^3 per channel (dimension 1 of an activation tensor, dimension 0 of a weight, each entry of a bias)."""
    if exact:
        r = 2 if weight else 3
        return torch.randint(-r, r + 1, shape, device="cuda", generator=g).float()
    t = torch.randn(shape, device="cuda", generator=g)
    if len(shape) == 1:
        sshape = shape
    else:
        sshape = [1] * len(shape)
        sshape[0 if weight else 1] = shape[0 if weight else 1]
    return t * torch.exp2(torch.randint(-3, 4, tuple(sshape), device="cuda", generator=g).float())


def _rb(t):
    """What the kernels' `thin_rb` / `f2bf` do to an fp32 operand: round to nearest even bf16."""
    return t.to(BF16).float()


def _data64(op, a, w, stride):
    """fp64 of a data pass (pad 1): Conv2d forward (0) and ConvTranspose2d input gradient (3) are convolutions with the module's
    weight as it lies, Conv2d input gradient (1) and ConvTranspose2d forward (2) transposed convolutions."""
    f = F.conv2d if op in (0, 3) else F.conv_transpose2d
    return f(a.double(), w.double(), None, stride, 1)


def _wrw64(transposed, x, dy, wshape, stride, pad=1):
    """fp64 weight gradient of the module (Conv2d [Cout,Cin,k,k] / ConvTranspose2d [Cin,Cout,k,k]) by torch's own backward."""
    w = torch.zeros(wshape, dtype=torch.float64, device="cuda")
    return torch.ops.aten.convolution_backward(dy.double(), x.double(), w, None, [stride, stride], [pad, pad], [1, 1], bool(transposed), [0, 0], 1,
                                               [False, True, False])[1]


WORST = {}


def _exact(tag, y, y64, abs64):
    """Regime (a).  Below 2^24 every product and every partial sum is an integer fp32 holds exactly, in any order: an fp32 result IS
    the fp64 one, a bf16 result its round-to-nearest-even.  (`+ 0` gives a zero its positive sign on both sides.)"""
    assert float(abs64.max()) < 2.0 ** 24, (tag, float(abs64.max()))
    want = y64.float().to(y.dtype)
    if not _same(y + 0, want + 0):
        bad = (y.double() != want.double()).nonzero()
        raise AssertionError("%s: %d of %d elements differ from the exact result, first at %s: %r != %r" % (
            tag, bad.shape[0], y.numel(), bad[0].tolist(), float(y[tuple(bad[0])]), float(want[tuple(bad[0])])))


def _in_band(entry, tag, y, y64, abs64, const):
    """Regime (b), elementwise: |y - y64| <= const * (fp64 convolution of the absolute values, + |bias|) + 2^-8 |y64| for a bf16 y."""
    band = const * abs64 + (2.0 ** -8 * y64.abs() if y.dtype == BF16 else 0.0)
    err = (y.double() - y64).abs()
    worst = float((err / band.clamp_min(1e-300)).max())
    WORST[entry] = max(WORST.get(entry, 0.0), worst)
    print("%s %s: max |err| / band %.3f (worst of %s so far %.3f)" % (entry, tag, worst, entry, WORST[entry]))
    assert bool(torch.isfinite(y).all()) and worst <= 1.0, (entry, tag, worst)


def _check(entry, tag, exact, y, y64, abs64, const=BAND):
    assert y.shape == y64.shape, (tag, y.shape, y64.shape)
    if exact:
        _exact(tag, y, y64, abs64)
    else:
        _in_band(entry, tag, y, y64, abs64, const)


def _nan_fill(t):
    _bits(t).fill_(0x7FC00DAD if t.element_size() == 4 else 0x7FC1)
    return t


def _guarded(monkeypatch, run, tensors, want, ws_bytes=None):
    """`run(*tensors)` once more inside an Arena: guarded copies of the inputs, NaN-filled scratch of exactly the size asked for."""
    arena = Arena(ws_fill="nan")
    copies = [arena.guarded_copy(t, "in%d" % i) for i, t in enumerate(tensors)]
    with arena.installed(monkeypatch):
        yg = run(*copies)
    torch.cuda.synchronize()
    arena.check_guards()
    assert all(_same(c, t) for c, t in zip(copies, tensors)), "an input was modified"
    assert _same(yg, want), "the guarded run differs"
    if ws_bytes is not None:
        assert arena.workspaces and arena.workspaces[0][0] == ws_bytes, (arena.workspaces and arena.workspaces[0][0], ws_bytes)


REGIMES = [pytest.param(True, id="exact"), pytest.param(False, id="real")]


# ---- ops.conv_thin_f2m_mfma ------------------------------------------------------------------------------------------------------------
F2M_MFMA_GUARDED = ("conv6_136_k3_b1_6x32", "conv3_8_k3_b33_250x32")


@pytest.mark.parametrize("exact", REGIMES)
@pytest.mark.parametrize("cid", list(P.F2M_MFMA_CASES))
def test_few_to_many_on_the_matrix_cores(cid, exact, monkeypatch):
    """ipsr_conv_thin_f2m_mfma: input and weights are rounded to bf16 whatever the tensors' types (thin_conv.hip:470, :553), bias
    and ReLU are fp32, one rounding on the way out."""
    from deepinpainting_amd import ops
    P.check_case(cid)
    tr, Cin, Cout, k, st, B, H, W = P.F2M_MFMA_CASES[cid][0]
    _, Cs, O, Ho, Wo, _, _ = P.f2m_mfma_geometry(P.F2M_MFMA_CASES[cid][0])
    op = ops.CONVT_BWD_DATA if tr else ops.CONV_FWD
    g = _gen(len(cid) * 131 + Ho + exact)
    a = _draw((B, Cs, Ho * st, Wo * st), g, exact)
    w = _draw((Cin, Cout, k, k) if tr else (Cout, Cin, k, k), g, exact, weight=True)
    bias = _draw((O,), g, exact, weight=True)
    assert ops.thin_f2m_mfma_supported(op, B, Cin, H, W, Cout, k, st)
    ar, wr = _rb(a), _rb(w)
    y64 = _data64(op, ar, wr, st)
    abs64 = _data64(op, ar.abs(), wr.abs(), st)
    b64 = bias.double().view(1, -1, 1, 1)
    for in_dt, out_dt in ((F32, BF16), (BF16, BF16), (BF16, F32)):
        inp = a.to(in_dt)
        for epi in (False, True):
            run = lambda aa, ww, bb: ops.conv_thin_f2m_mfma(op, aa, ww, (B, Cin, H, W), Cout, k, st, bias=bb if epi else None, relu=epi, out_dtype=out_dt)
            y = run(inp, w, bias)
            assert y.dtype == out_dt
            tag = "%s %s->%s%s" % (cid, in_dt, out_dt, " bias relu" if epi else "")
            _check("conv_thin_f2m_mfma", tag, exact, y, torch.relu(y64 + b64) if epi else y64, abs64 + b64.abs() if epi else abs64)
            if cid in F2M_MFMA_GUARDED and exact and (in_dt, out_dt, epi) == (F32, BF16, True):
                _guarded(monkeypatch, run, (inp, w, bias), y)


# ---- ops.conv_thin_wrw_mfma ------------------------------------------------------------------------------------------------------------
WRW_MFMA_GUARDED = ("kb136_cs3_k3_b2_5x16", "kb8_cs3_k3_b17_242x16")


@pytest.mark.parametrize("exact", REGIMES)
@pytest.mark.parametrize("cid", list(P.WRW_MFMA_CASES))
def test_weight_gradient_on_the_matrix_cores(cid, exact, monkeypatch):
    """ipsr_conv_thin_wrw_mfma: a bf16 wide tensor multiplies on the bf16 matrix cores, an fp32 narrow one is rounded to bf16 inside
    (thin_conv.hip:355); fp32 / fp32 multiplies unrounded on the fp32 matrix cores (:347).  The result is fp32."""
    from deepinpainting_amd import ops
    plan = P.check_case(cid)
    Kb, Cs, k, B, Hb, Wb = P.WRW_MFMA_CASES[cid][0]
    st = 1 if k == 3 else 2
    g = _gen(len(cid) * 137 + Hb + exact)
    big = _draw((B, Kb, Hb, Wb), g, exact)
    small = _draw((B, Cs, Hb * st, Wb * st), g, exact)
    for tr in (False, True):                              # Conv2d(Cs, Kb): big = dy, small = x;  ConvTranspose2d(Kb, Cs): big = x, small = dy
        pair = (lambda bg, sm: (bg, sm)) if tr else (lambda bg, sm: (sm, bg))
        Cin, Cout, H, W = (Kb, Cs, Hb, Wb) if tr else (Cs, Kb, Hb * st, Wb * st)
        assert ops.thin_wrw_mfma_supported(tr, B, Cin, H, W, Cout, k, st)
        ref = {}
        for big_dt, small_dt in ((F32, F32), (BF16, BF16), (BF16, F32)):
            rounded = big_dt == BF16
            if rounded not in ref:
                bg, sm = (_rb(big), _rb(small)) if rounded else (big, small)
                x, dy = pair(bg, sm)
                xa, dya = pair(bg.abs(), sm.abs())
                ref[rounded] = (_wrw64(tr, x, dy, (Kb, Cs, k, k), st), _wrw64(tr, xa, dya, (Kb, Cs, k, k), st))
            x, dy = pair(big.to(big_dt), small.to(small_dt))
            run = lambda xx, dd: ops.conv_thin_wrw_mfma(tr, xx, dd, k, st)
            dw = run(x, dy)
            assert dw.dtype == F32
            tag = "%s %s big %s small %s" % (cid, "convT" if tr else "conv", big_dt, small_dt)
            _check("conv_thin_wrw_mfma", tag, exact, dw, *ref[rounded])
            assert _same(run(x, dy), dw), "%s: two calls differ" % tag
            if cid in WRW_MFMA_GUARDED and exact and small_dt == F32 and tr == (big_dt == BF16):
                _guarded(monkeypatch, run, (x, dy), dw, plan["ws"])


# ---- ops.conv3x3_thin --------------------------------------------------------------------------------------------------------------------
THIN_GUARDED = ("f2m_b1_3_48_2x1026", "m2f_b1_18_6_5x260")


def _thin_data_case(cid, exact, monkeypatch, src, dst, B, H, W, few2many):
    """All four module passes that read `src` channels and write `dst`: Conv2d(src, dst) forward, Conv2d(dst, src) input gradient,
    ConvTranspose2d(src, dst) forward, ConvTranspose2d(dst, src) input gradient — flip 0, 1, 1, 0 (ops.py:874) — in the four io
    combinations.  With a bf16 tensor on either side the weights and an fp32 input are rounded to bf16 (thin_conv.hip:40-47, :64,
    :93-98, :124); fp32 / fp32 rounds nothing."""
    from deepinpainting_amd import ops
    g = _gen(len(cid) * 139 + W + exact)
    a = _draw((B, src, H, W), g, exact)
    bias = _draw((dst,), g, exact, weight=True)
    b64 = bias.double().view(1, -1, 1, 1)
    for op in range(4):
        Cin, Cout = (src, dst) if op in (0, 2) else (dst, src)
        kop, I, O, flip = P.thin_module_pass(op, Cin, Cout)
        assert (kop, I, O) == (0 if few2many else 1, src, dst) and ops.thin_supported(op, Cin, H, W, Cout)
        w = _draw((Cout, Cin, 3, 3) if op < 2 else (Cin, Cout, 3, 3), g, exact, weight=True)
        ref = {}
        for in_dt, out_dt in ((F32, F32), (F32, BF16), (BF16, F32), (BF16, BF16)):
            rounded = BF16 in (in_dt, out_dt)
            if rounded not in ref:
                ae, we = (_rb(a), _rb(w)) if rounded else (a, w)
                ref[rounded] = (_data64(op, ae, we, 1), _data64(op, ae.abs(), we.abs(), 1))
            y64, abs64 = ref[rounded]
            inp = a.to(in_dt)
            for epi in ((False, True) if few2many else (False,)):
                run = lambda aa, ww, bb: ops.conv3x3_thin(op, aa, ww, (B, Cin, H, W), Cout, bias=bb if epi else None, relu=epi, out_dtype=out_dt)
                y = run(inp, w, bias)
                assert y.dtype == out_dt
                tag = "%s op %d flip %d %s->%s%s" % (cid, op, flip, in_dt, out_dt, " bias relu" if epi else "")
                _check("conv3x3_thin " + ("few->many" if few2many else "many->few"), tag, exact, y,
                       torch.relu(y64 + b64) if epi else y64, abs64 + b64.abs() if epi else abs64)
                if cid in THIN_GUARDED and exact and (in_dt, out_dt) == (F32, BF16) and epi == few2many:
                    _guarded(monkeypatch, run, (inp, w, bias), y)


@pytest.mark.parametrize("exact", REGIMES)
@pytest.mark.parametrize("cid", list(P.F2M_CASES))
def test_few_to_many_on_the_vector_alus(cid, exact, monkeypatch):
    P.check_case(cid)
    B, few, many, H, W = P.F2M_CASES[cid][0]
    _thin_data_case(cid, exact, monkeypatch, few, many, B, H, W, True)


@pytest.mark.parametrize("exact", REGIMES)
@pytest.mark.parametrize("cid", list(P.M2F_CASES))
def test_many_to_few_on_the_vector_alus(cid, exact, monkeypatch):
    P.check_case(cid)
    B, few, many, H, W = P.M2F_CASES[cid][0]
    _thin_data_case(cid, exact, monkeypatch, many, few, B, H, W, False)


# ---- ops.conv3x3_thin_wrw ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("exact", REGIMES)
@pytest.mark.parametrize("cid", list(P.WRW_CASES))
def test_weight_gradient_on_the_vector_alus(cid, exact, monkeypatch):
    """ipsr_conv3x3_thin_wrw_io: with ONE bf16 operand the fp32 one is rounded to bf16 (thin_conv.hip:173, :191); two fp32 operands
    (and two bf16 ones) multiply as they are.  The result is fp32."""
    from deepinpainting_amd import ops
    plan = P.check_case(cid)
    B, Cb, Cs, H, W = P.WRW_CASES[cid][0]
    g = _gen(len(cid) * 149 + W + exact)
    big = _draw((B, Cb, H, W), g, exact)
    small = _draw((B, Cs, H, W), g, exact)
    for tr in (False, True):                              # Conv2d(Cs, Cb): big = dy;  ConvTranspose2d(Cb, Cs): big = x
        pair = (lambda bg, sm: (bg, sm)) if tr else (lambda bg, sm: (sm, bg))
        ref = {}
        for big_dt, small_dt in ((F32, F32), (F32, BF16), (BF16, F32), (BF16, BF16)):
            rounded = BF16 in (big_dt, small_dt)
            if rounded not in ref:
                bg, sm = (_rb(big), _rb(small)) if rounded else (big, small)
                x, dy = pair(bg, sm)
                xa, dya = pair(bg.abs(), sm.abs())
                ref[rounded] = (_wrw64(tr, x, dy, (Cb, Cs, 3, 3), 1), _wrw64(tr, xa, dya, (Cb, Cs, 3, 3), 1))
            x, dy = pair(big.to(big_dt), small.to(small_dt))
            run = lambda xx, dd: ops.conv3x3_thin_wrw(tr, xx, dd)
            dw = run(x, dy)
            assert dw.dtype == F32
            tag = "%s %s big %s small %s" % (cid, "convT" if tr else "conv", big_dt, small_dt)
            _check("conv3x3_thin_wrw", tag, exact, dw, *ref[rounded])
            assert _same(run(x, dy), dw), "%s: two calls differ" % tag
            if cid == "wrw_b2_6_6_130x516" and exact and (big_dt, small_dt) == ((BF16, F32) if tr else (F32, BF16)):
                _guarded(monkeypatch, run, (x, dy), dw, plan["ws"])


# ---- ops.conv_to_one / conv_to_one_wrw ------------------------------------------------------------------------------------------------
ONE_GUARDED = ("one_b2_c9_33x33_k4p1", "one_b2_c7_6x9_k3p1")


@pytest.mark.parametrize("exact", REGIMES)
@pytest.mark.parametrize("cid", list(P.TO_ONE_CASES))
def test_one_output_channel(cid, exact, monkeypatch):
    """ipsr_conv_to_one, forward (op 0) and weight gradient (op 2): fp32 tensors, nothing is rounded."""
    from deepinpainting_amd import ops
    plan = P.check_case(cid)
    B, C, H, W, K, pad = P.TO_ONE_CASES[cid][0]
    assert ops.conv_to_one_supported(B, C, H, W, K, 1, pad, 1)
    g = _gen(len(cid) * 151 + W + exact)
    x = _draw((B, C, H, W), g, exact)
    w = _draw((1, C, K, K), g, exact, weight=True)
    dy = _draw((B, 1, plan["Ho"], plan["Wo"]), g, exact)
    fwd = lambda xx, ww: ops.conv_to_one(xx, ww, pad)
    y = fwd(x, w)
    _check("conv_to_one", cid + " forward", exact, y, F.conv2d(x.double(), w.double(), None, 1, pad), F.conv2d(x.abs().double(), w.abs().double(), None, 1, pad), BAND_ONE)
    assert _same(fwd(x, w), y)
    wrw = lambda xx, dd: ops.conv_to_one_wrw(xx, dd, K, pad)
    dw = wrw(x, dy)
    _check("conv_to_one_wrw", cid + " weight gradient", exact, dw, _wrw64(False, x, dy, (1, C, K, K), 1, pad), _wrw64(False, x.abs(), dy.abs(), (1, C, K, K), 1, pad), BAND_ONE)
    assert _same(wrw(x, dy), dw)
    if cid in ONE_GUARDED and exact:
        _guarded(monkeypatch, fwd, (x, w), y, plan["ws"])
        _guarded(monkeypatch, wrw, (x, dy), dw)


# ---- refusals --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rid", list(P.THIN_IO_REFUSED))
def test_refused_thin_shapes_write_nothing(rid):
    from deepinpainting_amd import _lib, ops
    L = _lib.lib()
    kop, B, I, O, H, W = P.THIN_IO_REFUSED[rid]
    assert P.thin_io_plan(kop, B, I, O, H, W) is None
    x = torch.zeros(B, I, H, W, device="cuda")
    w = torch.zeros(O, I, 3, 3, device="cuda")
    assert not ops.thin_supported(ops.CONV_FWD, I, H, W, O)
    with pytest.raises(NotImplementedError):
        ops.conv3x3_thin(ops.CONV_FWD, x, w, (B, I, H, W), O)
    for io in range(4):
        xin = x.to(BF16) if io & 1 else x
        out = _nan_fill(torch.empty(B, O, H, W, device="cuda", dtype=BF16 if io & 2 else F32))
        keep = out.clone()
        torch.cuda.synchronize()
        rc = L.ipsr_conv3x3_thin_io(kop, xin.data_ptr(), w.data_ptr(), None, 0, out.data_ptr(), B, I, O, H, W, I * 9, 9, 0, io, ops._stream())
        torch.cuda.synchronize()
        assert rc == IPSR_ERR_UNSUPPORTED, (rid, io, rc, L.ipsr_last_error())
        assert _same(out, keep), "the output was written by a refused call"


def test_refused_one_channel_shape_writes_nothing():
    from deepinpainting_amd import _lib, ops
    L = _lib.lib()
    (B, C, H, W, K, pad), = P.TO_ONE_REFUSED.values()
    assert P.to_one_plan(B, C, H, W, K, pad) is None and L.ipsr_conv_to_one_workspace_bytes(B, C, H, W, K, pad) == 0
    assert not ops.conv_to_one_supported(B, C, H, W, K, 1, pad, 1)
    Ho, Wo = H + 2 * pad - K + 1, W + 2 * pad - K + 1
    x = torch.zeros(B, C, H, W, device="cuda")
    w = torch.zeros(1, C, K, K, device="cuda")
    dy = torch.zeros(B, 1, Ho, Wo, device="cuda")
    with pytest.raises(NotImplementedError):
        ops.conv_to_one(x, w, pad)
    with pytest.raises(NotImplementedError):
        ops.conv_to_one_wrw(x, dy, K, pad)
    ws = torch.empty(1 << 20, dtype=torch.uint8, device="cuda")
    for op, other, shape in ((0, w, (B, 1, Ho, Wo)), (2, dy, (1, C, K, K))):
        out = _nan_fill(torch.empty(shape, device="cuda"))
        keep = out.clone()
        torch.cuda.synchronize()
        rc = L.ipsr_conv_to_one(op, x.data_ptr(), other.data_ptr(), out.data_ptr(), B, C, H, W, K, pad, ws.data_ptr(), ws.numel(), ops._stream())
        torch.cuda.synchronize()
        assert rc == IPSR_ERR_UNSUPPORTED, (op, rc, L.ipsr_last_error())
        assert _same(out, keep), "the output was written by a refused call"
