"""The two fp32 matrix-core convolution engines in every launch variant, against torch in fp64 on the GPU: ipsr_conv_smallmap (the
`sm_*` kernels of csrc/smallmap.hip, planned by `sm_plan`) and ipsr_conv2d (csrc/conv_gemm.hip, planned by `make_plan` / `choose_split`).

Every case goes through `ops.conv_smallmap` / `ops.conv2d`.  tests/fp32_conv_plan.py restates the two launchers and holds the case
tables; tests/test_fp32_conv_plan.py proves without a GPU that the tables reach every row below, and each test here asserts its own
rows again (`P.check_case`) before it compares numbers.  A case id names the module (kind, channels in, map, channels out, geometry,
batch); the pass after the colon is data | wrw | fwd of ipsr_conv_smallmap, or fwd | bwd (the module's forward / input gradient) of
ipsr_conv2d.

  variant                                                                                       selected at                                       case id:pass
  --------------------------------------------------------------------------------------------  ------------------------------------------------  ----------------------------------------
  sm_data_kernel<1>                                                                             smallmap.hip: sm_plan nb, launch_smallmap         conv8_224_6x6_k4s2_b1:data, conv24_32_8x8_k4s2_b1:data
  sm_data_kernel<2>, one group                                                                  smallmap.hip: sm_plan nb (DATA), launch_smallmap  conv32_160_5x5_k4s1_b3:data
  sm_data_kernel<2>: blockIdx.z > 0, the last group half zero blocks                            smallmap.hip: sm_plan ngroups, sm_data_kernel     conv8_32_12x12_k4s2_b2:data, conv8_32_20x20_k4s2_b2:data
  sm_data_kernel<2>: blockIdx.z > 0, a ragged last block                                        smallmap.hip: sm_plan ngroups, sm_data_kernel     conv8_32_18x14_k4s2_b2:data, conv8_32_12x12_k4s2_b2:data
  sm_data_kernel<2>: 16 groups at the limit of 1024 positions                                   smallmap.hip: sm_plan, P > 1024                   conv8_64_32x32_k4s2_b4:data
  sm_data_kernel: three slabs, a short wave (4 of 20 rows)                                      smallmap.hip: sm_plan slabs, sm_data_kernel       conv8_224_6x6_k4s2_b1:data, convT224_8_3x3_k4s2_b1:data
  sm_data_kernel<1>: a full unroll group and a partly filled one                                smallmap.hip: sm_data_kernel unroll loop          conv128_96_3x3_k3s1_b1:data, conv8_224_6x6_k4s2_b1:data
  sm_data_kernel<1>: half an unroll group only                                                  smallmap.hip: sm_data_kernel unroll loop          conv24_32_8x8_k4s2_b1:data, conv120_32_8x8_k4s2_b1:data
  sm_data_kernel<2>: a partly filled unroll group                                               smallmap.hip: sm_data_kernel unroll loop          conv32_160_5x5_k4s1_b3:data
  sm_fwd_kernel<1>                                                                              smallmap.hip: sm_plan nb, launch_smallmap         conv8_224_6x6_k4s2_b1:fwd, conv24_32_8x8_k4s2_b1:fwd
  sm_fwd_kernel<2>                                                                              smallmap.hip: sm_plan nb, launch_smallmap         conv32_160_5x5_k4s1_b3:fwd
  sm_fwd_kernel<4> with one all-zero block (three position blocks)                              smallmap.hip: sm_plan nb, launch_smallmap         conv8_32_12x12_k4s2_b2:fwd
  sm_fwd_kernel<4> with a ragged last block                                                     smallmap.hip: sm_plan nb, launch_smallmap         conv8_32_18x14_k4s2_b2:fwd
  sm_fwd_kernel<4>: blockIdx.z > 0                                                              smallmap.hip: sm_plan ngroups, sm_fwd_kernel      conv8_32_20x20_k4s2_b2:fwd, conv8_64_32x32_k4s2_b4:fwd
  sm_fwd_kernel<4>: 8 groups at the limit of 1024 positions                                     smallmap.hip: sm_plan, P > 1024                   conv8_64_32x32_k4s2_b4:fwd
  sm_fwd_kernel: four slabs of 72 columns (two groups and one 8-column step over)               smallmap.hip: sm_plan slabs, sm_fwd_kernel `ok`   conv128_96_3x3_k3s1_b1:fwd
  sm_fwd_kernel: a short wave and an idle wave (`qa == qb`)                                     smallmap.hip: sm_plan slabs, sm_fwd_kernel        conv120_32_8x8_k4s2_b1:fwd
  sm_wrw_kernel: odd P, the zero row of Pp is read                                              smallmap.hip: sm_plan Pp, launch_smallmap         conv8_224_6x6_k4s2_b1:wrw, convT224_8_3x3_k4s2_b1:wrw
                                                                                                                                                  conv128_96_3x3_k3s1_b1:wrw
  sm_wrw_kernel: a partly filled unroll group (Pp % 8 != 0)                                     smallmap.hip: sm_wrw_kernel unroll loop           conv8_224_6x6_k4s2_b1:wrw, conv8_32_18x14_k4s2_b2:wrw
  sm_wrw_kernel: 1024 positions                                                                 smallmap.hip: sm_plan, P > 1024                   conv8_64_32x32_k4s2_b4:wrw
  sm_wrw_kernel: more than one block on x and y                                                 smallmap.hip: launch_smallmap, op 1 grid          conv128_96_3x3_k3s1_b1:wrw, conv32_160_5x5_k4s1_b3:wrw
  conv_gemm_kernel<9>: 1 stage                                                                  conv_gemm.hip:180-184                             conv2_9x7_c5_k3_b1:fwd, convT30_5x6_c2_k3_b2:bwd
  conv_gemm_kernel<9>: 2 stages                                                                 conv_gemm.hip:181                                 conv4_9x7_c6_k3_b2:fwd, conv4_13x11_c6_k3s3_b2:fwd
  conv_gemm_kernel<9>: 3 stages                                                                 conv_gemm.hip:182                                 conv6_11x13_c10_k3_b3:fwd, conv4_9x7_c6_k3_b2:bwd
  conv_gemm_kernel<9>: 5 stages, the ring wraps                                                 conv_gemm.hip:156, :193                           conv10_5x6_c30_k3_b1:fwd, conv6_11x13_c10_k3_b3:bwd
  conv_gemm_kernel<9>: 15 stages                                                                conv_gemm.hip:334                                 conv10_5x6_c30_k3_b1:bwd, convT30_5x6_c2_k3_b2:fwd
  conv_gemm_kernel<16>: 1 stage                                                                 conv_gemm.hip:180-184                             conv1_12x10_c4_k4s2_b2:fwd, convT20_6x4_c1_k4s2_b1:bwd
  conv_gemm_kernel<16>: 2 stages                                                                conv_gemm.hip:181                                 conv2_12x10_c8_k4s2_b1:fwd, convT12_3x5_c2_k4s2_b3:bwd
  conv_gemm_kernel<16>: 3 stages                                                                conv_gemm.hip:182                                 conv3_9x11_c12_k4s2_b3:fwd, convT4_4x6_c3_k4s2_b1:bwd
  conv_gemm_kernel<16>: 5 stages, the ring wraps                                                conv_gemm.hip:156, :193                           conv5_8x8_c20_k4s2_b1:fwd, convT8_5x3_c5_k4s2_b2:bwd
  conv_gemm_kernel<16>: 15 stages                                                               conv_gemm.hip:334                                 conv15_6x6_c60_k4s2_b1:fwd
  conv_gemm_kernel<4>: 1 stage                                                                  conv_gemm.hip:180-184                             conv1_12x10_c4_k4s2_b2:bwd, convT4_4x6_c3_k4s2_b1:fwd
  conv_gemm_kernel<4>: 2 stages                                                                 conv_gemm.hip:181                                 conv2_12x10_c8_k4s2_b1:bwd, convT8_5x3_c5_k4s2_b2:fwd
  conv_gemm_kernel<4>: 3 stages                                                                 conv_gemm.hip:182                                 conv3_9x11_c12_k4s2_b3:bwd, convT12_3x5_c2_k4s2_b3:fwd
  conv_gemm_kernel<4>: 5 stages, the ring wraps                                                 conv_gemm.hip:156, :193                           conv5_8x8_c20_k4s2_b1:bwd, convT20_6x4_c1_k4s2_b1:fwd
  conv_gemm_kernel<4>: 15 stages                                                                conv_gemm.hip:334                                 conv15_6x6_c60_k4s2_b1:bwd, convT60_2x3_c4_k4s2_b2:fwd
  split-K: two even splits of 8 stages                                                          conv_gemm.hip:334-336, :231                       conv32_6x5_c136_k3_b2:fwd
  split-K: a short last split of 2 stages (`ns > 2` false)                                      conv_gemm.hip:142, :182                           conv130_9x13_c70_k3_b3:fwd
  split-K: a short last split of 1 stage (`ns > 1` false), 16 splits                            conv_gemm.hip:142, :181                           conv17_5x5_c136_k4s1_b1:bwd
  split-K on the 16-tap kernel, last split one stage short                                      conv_gemm.hip:335-336                             conv17_5x5_c136_k4s1_b1:fwd
  two m tiles, the second with 8 live rows                                                      conv_gemm.hip:349, :238, :250                     conv32_6x5_c136_k3_b2:fwd, conv17_5x5_c136_k4s1_b1:fwd
                                                                                                                                                  conv4_24x23_c136_k3_b3:fwd
  two m tiles and split-K: partial tiles of the second m tile                                   conv_gemm.hip:232-238                             conv32_6x5_c136_k3_b2:fwd, conv17_5x5_c136_k4s1_b1:fwd
  one pixel tile partly filled                                                                  conv_gemm.hip:127, :230                           conv2_9x7_c5_k3_b1:fwd, conv4_9x7_c6_k3_b2:fwd
  several pixel tiles, a ragged last one                                                        conv_gemm.hip:127, :230                           conv6_11x13_c10_k3_b3:fwd, conv4_24x23_c136_k3_b3:fwd
                                                                                                                                                  conv130_9x13_c70_k3_b3:fwd
  a grid that is no multiple of 8 workgroups, above 8 (xcd_remap)                               ipsr_common.h:46-52                               conv4_24x23_c136_k3_b3:fwd
  parity classes: odd output extents, four different grids                                      conv_gemm.hip:366                                 conv4_21x19_c8_k4s2_b2:bwd, conv3_9x11_c12_k4s2_b3:bwd
                                                                                                                                                  conv8_15x13_c4_k4s2p1d3_b2:bwd
  parity classes without taps: need_zero, one 16-tap class                                      conv_gemm.hip:367, :411-412                       conv3_12x10_c5_k4s2p3d2_b2:bwd, conv3_2x2_c5_k4s2p3d2_b3:bwd
  the dilated input gradient on the 2 x 2 map                                                   conv_gemm.hip:366-367                             conv3_2x2_c5_k4s2p3d2_b3:bwd
  k = 2 on the direct forms: a 4-tap gather, stride 1 and 2, op 0 and op 3                      conv_gemm.hip:317, :355, :419                     conv4_9x8_c8_k2s1_b2:fwd, conv8_9x8_c6_k2s2p1_b1:fwd
                                                                                                                                                  convT6_5x4_c12_k2s2_b2:bwd, conv4_9x8_c8_k2s2p1d2_b1:fwd
  k = 2 on the stride-1 transposed form (op 1)                                                  conv_gemm.hip:353, :423                           conv4_9x8_c8_k2s1_b2:bwd
  k = 2, 3 with dilation 2 on the stride-2 transposed form: all taps in one parity class        conv_gemm.hip:363-367                             conv6_9x8_c4_k3s2p2d2_b2:bwd, conv4_9x8_c8_k2s2p1d2_b1:bwd
  stride 3 on the direct forms, k3 and k4, op 0 and op 3                                        conv_gemm.hip:421, :130                           conv4_13x11_c6_k3s3_b2:fwd, conv3_13x11_c6_k4s3p2_b1:fwd
                                                                                                                                                  convT6_4x5_c3_k4s3_b2:bwd
  dilation 3 on the stride-2 transposed forms: two taps per parity, offsets a step of -3 apart  conv_gemm.hip:325, :435-436                       conv8_15x13_c4_k4s2p1d3_b2:bwd, convT8_4x3_c4_k4s2p1d3_b1:fwd
  refused: 1088 positions, all three ops                                                        smallmap.hip: sm_plan, P > 1024                   conv8_32_32x34_k4s2_b4
  refused: k3 s2 transposed: one or two taps in a parity class                                  conv_gemm.hip:373                                 conv4_8x8_c4_k3s2_bwd, convT4_4x4_c4_k3s2_fwd
  refused: k = 1: one tap                                                                       conv_gemm.hip:373                                 conv4_6x6_c4_k1
  refused: k3: odd reduction channels                                                           conv_gemm.hip:376                                 conv3_6x6_c4_k3_odd, conv4_6x6_c3_k3_odd
  refused: 4-tap classes: reduction channels no multiple of 4                                   conv_gemm.hip:376                                 convT6_4x4_c4_k4s2_mod4, conv4_8x8_c6_k4s2_mod4
  refused: k2 direct: reduction channels no multiple of 4                                       conv_gemm.hip:376                                 conv6_9x8_c6_k2_mod4
  refused: stride 3 transposed                                                                  conv_gemm.hip:358                                 conv4_13x11_c4_k4s3_bwd, convT4_4x5_c4_k4s3_fwd

Not reached, with the reason: an idle wave (`ra == rb`) in sm_data_kernel.  Within the 224 channels these cases keep to, `sm_plan`
cannot produce one (test_fp32_conv_plan.py::test_no_data_wave_is_idle_within_the_case_limits enumerates it; the first R that has one
is 416, and the nets' own R split exactly).  The two launch-time refusals of the parity form (irregular tap set, `nr != nsx`) cannot
fire for k <= 4 (::test_launch_time_refusals_of_the_parity_form_cannot_fire).

The three sentences of include/ipsr_hip.h that nothing had compared with anything are settled as SERVED: k = 2 on the direct forms
(and on the stride-1 transposed form), stride 3 on the direct forms, dilation 3 on the stride-2 transposed forms all pass the exact
regime below, and the header now says so.  So does what the mirror showed the entry also accepts: k = 2, 3 with even dilation on the
stride-2 transposed forms (all taps in one parity class).

Two data regimes per case, both against fp64:

(a) exact.  Activations and dy are integers in [-3, 3], weights in [-2, 2].  The test first asserts that the fp64 convolution of the
absolute values stays below 2^24 — a condition on the data, held by orders of magnitude (the longest reduction here is ~16 k terms of
at most 6).  Then every product and every partial sum is an integer that fp32 holds exactly, in any order, so the fp32 result must
equal the fp64 reference bit for bit, on every element and for every op.  A dropped or doubled tap, row pair, slab, position block,
k-split or parity class changes an integer.

(b) real-valued.  Normal draws times a per-channel power of two in 2^-3 .. 2^3.  The band is elementwise: 2e-5 (the constant
tests/test_gpu_thin_variants.py holds the fp32 kernels to) times the fp64 convolution of the ABSOLUTE values.  Each check prints its
worst |err| / band.  Largest observed on an MI355X: 0.015 for ipsr_conv_smallmap (conv8_64_32x32_k4s2_b4:wrw), 0.021 for ipsr_conv2d
(conv6_11x13_c10_k3_b3:bwd).

A second call gives the same bits (fixed summation order: slabs and k-splits are added in order).  The most ragged case of each op runs
once more inside tests/guarded.py's Arena (guard bands around every tensor, NaN-filled scratch of exactly the size the query asks
for): guards intact, inputs unmodified, the same bits.  Refused calls leave a NaN-patterned output bitwise unchanged and surface as
NotImplementedError from `ops`.
"""
import pytest
import torch

import fp32_conv_plan as P
from guarded import Arena

pytestmark = pytest.mark.gpu

IPSR_ERR_UNSUPPORTED = -2
BAND = 2e-5                                               # tests/test_gpu_thin_variants.py: the fp32 kernels


def _bits(t):
    return t.contiguous().view(torch.int32)


def _same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(_bits(a), _bits(b))


def _draw(shape, g, exact, weight=False):
    """Regime (a): integers in [-3, 3] (activations, dy) or [-2, 2] (weights).  Regime (b): normal draws times a power of two in
    2^-3 .. 2^3 per channel (dimension 1 of an activation tensor, dimension 0 of a weight)."""
    if exact:
        r = 2 if weight else 3
        return torch.randint(-r, r + 1, shape, device="cuda", generator=g).float()
    t = torch.randn(shape, device="cuda", generator=g)
    sshape = [1] * len(shape)
    sshape[0 if weight else 1] = shape[0 if weight else 1]
    return t * torch.exp2(torch.randint(-3, 4, tuple(sshape), device="cuda", generator=g).float())


def _module64(kind, x, w, dy, st, pad, dil):
    """fp64 on the GPU of the module's three passes -> (y, dx, dw): the forward by torch's convolution, both gradients by its own
    backward (Conv2d [Cout,Cin,k,k] / ConvTranspose2d [Cin,Cout,k,k], output_padding 0)."""
    tr = kind == "convT"
    xd, wd = x.double(), w.double()
    y = torch.nn.functional.conv_transpose2d(xd, wd, None, st, pad, 0, 1, dil) if tr else torch.nn.functional.conv2d(xd, wd, None, st, pad, dil)
    dx, dw, _ = torch.ops.aten.convolution_backward(dy.double(), xd, wd, None, [st, st], [pad, pad], [dil, dil], tr, [0, 0], 1, [True, True, False])
    return y, dx, dw


class _Case:
    """The tensors of one case in one regime and the two references (of the values and of the absolute values), computed once and
    left unchanged; the tests of the case's passes share them."""
    cache = {}

    def __init__(self, case, exact, seed):
        kind, Cin, H, W, Cout, k, st, pad, dil, B = case                 # the order of CG_CASES
        tr = kind == "convT"
        g = torch.Generator(device="cuda").manual_seed(seed)
        fop = P.CONVT_FWD if tr else P.CONV_FWD
        self.Hy, self.Wy = P.conv_out_dim(fop, H, k, st, pad, dil), P.conv_out_dim(fop, W, k, st, pad, dil)
        self.x = _draw((B, Cin, H, W), g, exact)
        self.w = _draw((Cin, Cout, k, k) if tr else (Cout, Cin, k, k), g, exact, weight=True)
        self.dy = _draw((B, Cout, self.Hy, self.Wy), g, exact)
        self.ref = _module64(kind, self.x, self.w, self.dy, st, pad, dil)
        self.abs = _module64(kind, self.x.abs(), self.w.abs(), self.dy.abs(), st, pad, dil)
        assert tuple(self.ref[0].shape) == (B, Cout, self.Hy, self.Wy)
        self.keep = [t.clone() for t in (self.x, self.w, self.dy)]

    @classmethod
    def get(cls, cid, case, exact):
        key = (cid, exact)
        if key not in cls.cache:
            cls.cache.clear()                             # one case at a time stays resident
            cls.cache[key] = cls(case, exact, sum(map(ord, cid)) * 2 + exact)
        return cls.cache[key]

    def unchanged(self):
        return all(_same(a, b) for a, b in zip((self.x, self.w, self.dy), self.keep))


WORST = {}


def _check(engine, tag, exact, y, y64, abs64):
    """Regime (a): below 2^24 every product and partial sum is an integer fp32 holds exactly, in any order, so the fp32 result IS the
    fp64 one (`+ 0` gives a zero its positive sign on both sides).  Regime (b), elementwise: |y - y64| <= 2e-5 * (the fp64 convolution
    of the absolute values)."""
    assert y.shape == y64.shape and y.dtype == torch.float32, (tag, y.shape, y64.shape, y.dtype)
    if exact:
        assert float(abs64.max()) < 2.0 ** 24, (tag, float(abs64.max()))
        want = y64.float()
        if not _same(y + 0, want + 0):
            bad = (y.double() != want.double()).nonzero()
            raise AssertionError("%s: %d of %d elements differ from the exact result, first at %s: %r != %r" % (
                tag, bad.shape[0], y.numel(), bad[0].tolist(), float(y[tuple(bad[0])]), float(want[tuple(bad[0])])))
        return
    band = BAND * abs64
    err = (y.double() - y64).abs()
    worst = float((err / band.clamp_min(1e-300)).max())
    WORST[engine] = max(WORST.get(engine, 0.0), worst)
    print("%s %s: max |err| / band %.3f (worst of %s so far %.3f)" % (engine, tag, worst, engine, WORST[engine]))
    assert bool(torch.isfinite(y).all()) and worst <= 1.0, (engine, tag, worst)


def _nan_fill(t):
    _bits(t).fill_(0x7FC00DAD)
    return t


def _guarded(monkeypatch, run, tensors, want, ws_bytes):
    """`run(*tensors)` once more inside an Arena: guarded copies of the inputs, NaN-filled scratch of exactly the size asked for."""
    arena = Arena(ws_fill="nan")
    copies = [arena.guarded_copy(t, "in%d" % i) for i, t in enumerate(tensors)]
    with arena.installed(monkeypatch):
        yg = run(*copies)
    torch.cuda.synchronize()
    arena.check_guards()
    assert all(_same(c, t) for c, t in zip(copies, tensors)), "an input was modified"
    assert _same(yg, want), "the guarded run differs"
    assert arena.workspaces and arena.workspaces[0][0] == ws_bytes, (arena.workspaces and arena.workspaces[0][0], ws_bytes)


REGIMES = [pytest.param(True, id="exact"), pytest.param(False, id="real")]


# ---- ops.conv_smallmap -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("exact", REGIMES)
@pytest.mark.parametrize("cid", list(P.SM_CASES))
def test_smallmap_in_every_variant(cid, exact, monkeypatch):
    """ipsr_conv_smallmap, all three ops of the case.  A Conv2d reads DATA as its input gradient, FWD as its forward; a ConvTranspose2d
    DATA as its forward, FWD as its input gradient; WRW is the weight gradient of either (tests/test_gpu_conv.py:244-263)."""
    from deepinpainting_amd import ops
    case, req = P.SM_CASES[cid]
    geo = P.sm_geometry(case)
    kind, Ci, Co, H, W, k, st, pad, dil, B = case
    t = _Case.get(cid, (kind, Ci, H, W, Co, k, st, pad, dil, B), exact)          # _Case takes the order of the implicit-GEMM tables
    (y64, dx64, dw64), (ya, dxa, dwa) = t.ref, t.abs
    if case[0] == "convT":
        passes = {P.SM_DATA: ((t.x, t.w), y64, ya), P.SM_WRW: ((t.x, t.dy), dw64, dwa), P.SM_FWD: ((t.dy, t.w), dx64, dxa)}
    else:
        passes = {P.SM_DATA: ((t.dy, t.w), dx64, dxa), P.SM_WRW: ((t.dy, t.x), dw64, dwa), P.SM_FWD: ((t.x, t.w), y64, ya)}
    for op, (operands, want, wabs) in passes.items():
        pid = "%s:%s" % (cid, P.SM_OP_NAME[op])
        plan = P.check_case(pid)
        assert ops.smallmap_supported(op, *geo)
        run = lambda a, b: ops.conv_smallmap(op, a, b, *geo)
        y = run(*operands)
        _check("conv_smallmap", pid, exact, y, want, wabs)
        assert _same(run(*operands), y), "%s: two calls differ" % pid
        if exact and P.SM_GUARDED[op] == cid:
            _guarded(monkeypatch, run, operands, y, plan["ws"])
    assert t.unchanged()


@pytest.mark.parametrize("rid", list(P.SM_REFUSED))
def test_refused_smallmap_shapes_write_nothing(rid):
    """1088 positions: IPSR_ERR_UNSUPPORTED from all three ops before any launch, NotImplementedError from the wrapper."""
    from deepinpainting_amd import _lib, ops
    L = _lib.lib()
    kind, Ci, Co, H, W, k, st, pad, dil, B = P.SM_REFUSED[rid]
    geo = P.sm_geometry(P.SM_REFUSED[rid])
    _, R, Cq, Ho, Wo, Hf, Wf = geo[:7]
    coarse, fine, w = torch.zeros(B, R, Ho, Wo, device="cuda"), torch.zeros(B, Cq, Hf, Wf, device="cuda"), torch.zeros(R, Cq, k, k, device="cuda")
    ws = torch.empty(8 << 20, dtype=torch.uint8, device="cuda")
    for op, (a, b, oshape) in {P.SM_DATA: (coarse, w, fine.shape), P.SM_WRW: (coarse, fine, w.shape), P.SM_FWD: (fine, w, coarse.shape)}.items():
        assert P.sm_plan(op, *geo) is None and not ops.smallmap_supported(op, *geo)
        with pytest.raises(NotImplementedError):
            ops.conv_smallmap(op, a, b, *geo)
        out = _nan_fill(torch.empty(tuple(oshape), device="cuda"))
        keep = out.clone()
        torch.cuda.synchronize()
        rc = L.ipsr_conv_smallmap(op, a.data_ptr(), b.data_ptr(), out.data_ptr(), *geo, ws.data_ptr(), ws.numel(), ops._stream())
        torch.cuda.synchronize()
        assert rc == IPSR_ERR_UNSUPPORTED, (rid, op, rc, L.ipsr_last_error())
        assert b"positions" in L.ipsr_last_error()
        assert _same(out, keep), "the output was written by a refused call"


# ---- ops.conv2d ----------------------------------------------------------------------------------------------------------------------------
def _cg_pass(t, case, which):
    """(op, input, reference, reference of the absolute values) of a module pass: "fwd" reads x, "bwd" reads dy."""
    op = P.cg_ops(case[0])[which]
    return (op, t.x, t.ref[0], t.abs[0]) if which == "fwd" else (op, t.dy, t.ref[1], t.abs[1])


@pytest.mark.parametrize("exact", REGIMES)
@pytest.mark.parametrize("cid", list(P.CG_CASES))
def test_implicit_gemm_in_every_variant(cid, exact, monkeypatch):
    """ipsr_conv2d: the passes of the module that the case names (both where both are served)."""
    from deepinpainting_amd import ops
    case, req = P.CG_CASES[cid]
    kind, Cin, H, W, Cout, k, st, pad, dil, B = case
    t = _Case.get(cid, case, exact)
    for which in req:
        pid = "%s:%s" % (cid, which)
        plan = P.check_case(pid)
        op, inp, want, wabs = _cg_pass(t, case, which)
        assert ops.conv2d_supported(op, B, Cin, H, W, Cout, k, st, pad, dil)
        run = lambda a, ww: ops.conv2d(op, a, ww, (B, Cin, H, W), Cout, k, st, pad, dil)
        y = run(inp, t.w)
        _check("conv2d", pid, exact, y, want, wabs)
        assert _same(run(inp, t.w), y), "%s: two calls differ" % pid
        if exact and P.CG_GUARDED[op] == cid:
            _guarded(monkeypatch, run, (inp, t.w), y, plan["ws"])
    assert t.unchanged()


@pytest.mark.parametrize("rid", list(P.CG_REFUSED))
def test_refused_implicit_gemm_shapes_write_nothing(rid):
    """IPSR_ERR_UNSUPPORTED before any launch (every refusal is in make_plan, ahead of the memset and the first class), and
    NotImplementedError from the wrapper."""
    from deepinpainting_amd import _lib, ops
    L = _lib.lib()
    case, refused, why = P.CG_REFUSED[rid]
    kind, Cin, H, W, Cout, k, st, pad, dil, B = case
    tr = kind == "convT"
    fop = P.CONVT_FWD if tr else P.CONV_FWD
    Hy, Wy = P.conv_out_dim(fop, H, k, st, pad, dil), P.conv_out_dim(fop, W, k, st, pad, dil)
    x, dy = torch.zeros(B, Cin, H, W, device="cuda"), torch.zeros(B, Cout, Hy, Wy, device="cuda")
    w = torch.zeros((Cin, Cout, k, k) if tr else (Cout, Cin, k, k), device="cuda")
    ws = torch.empty(8 << 20, dtype=torch.uint8, device="cuda")
    for which in refused:
        a = P.cg_args(case, which)
        inp, oshape = (x, dy.shape) if which == "fwd" else (dy, x.shape)
        assert P.conv2d_plan(*a) is None and not ops.conv2d_supported(*a), (rid, which, why)
        with pytest.raises(NotImplementedError):
            ops.conv2d(a[0], inp, w, (B, Cin, H, W), Cout, k, st, pad, dil)
        out = _nan_fill(torch.empty(tuple(oshape), device="cuda"))
        keep = out.clone()
        torch.cuda.synchronize()
        rc = L.ipsr_conv2d(a[0], inp.data_ptr(), w.data_ptr(), out.data_ptr(), B, Cin, H, W, Cout, k, st, pad, dil, ws.data_ptr(), ws.numel(), ops._stream())
        torch.cuda.synchronize()
        assert rc == IPSR_ERR_UNSUPPORTED, (rid, which, rc, L.ipsr_last_error())
        assert _same(out, keep), "the output was written by a refused call"
