"""ipsr_conv_smallmap with its operands gathered in the main kernels and its streams software-pipelined (csrc/smallmap.hip).

The three main kernels (sm_data_kernel, sm_fwd_kernel, sm_wrw_kernel) read the small operand either from the image a pre-pass laid out in
the workspace ("staged", `ipsr_debug_set_option(3, 1)`) or straight from the NCHW tensor ("gathered", `ipsr_debug_set_option(3, 2)`;
the default gathers except in the weight gradient above 32 positions, where the pre-passes measured faster), and consume their
reduction range in groups of G loads that rotate through three register sets (`sm_stream`).  This file checks

  * gathered == staged == the default, bit for bit, for all three ops of every case of fp32_conv_plan.SM_CASES and of the table
    below, in the integer-exact and in the real-valued regime;
  * the boundaries of the pipeline: for each kernel, wave ranges of every length class around its group size G — below G, exactly G,
    G plus a partly filled group, 2G, 2G plus a partly filled group, and an empty range — and, because three sets rotate, every group
    count 3 .. 6 (the loop body runs once or twice, with 0, 1 or 2 groups left over).  The table is chosen with `wave_classes`, a
    restatement of how the kernels cut a range into groups on top of fp32_conv_plan.sm_plan, and a CPU test proves that it reaches
    every class.  Each case is compared with torch in fp64 in the exact regime (integers in [-3, 3] / [-2, 2]; the fp64 convolution of
    the absolute values is asserted below 2^24, so fp32 holds every partial sum and equality is bit for bit), twice (determinism);
  * a 1 x 1 coarse grid under k4 s2 p1 (12 of 16 taps outside the map), B = 1 and B = 3, P no multiple of 32, a non-square map, k = 3
    and a dilated k4 s2 p3 d2 geometry;
  * the most ragged case of each op once more inside guarded.Arena: guard bands around every tensor, NaN-filled scratch of exactly
    the size the query asks for; guards intact, inputs unmodified, the same bits.

Group sizes (smallmap.hip: SmDepth, sm_wrw_kernel): DATA 4 row pairs = 8 rows; FWD 4 groups of 8 columns = 32 columns, 2 = 16 columns
with four position blocks; WRW 4 position pairs = 8 positions.

The limits of the table are R <= 224, Q <= 2048, maps <= 12 x 12.  Two classes cannot be reached inside them, which
`test_classes_out_of_reach_inside_the_limits` enumerates: a DATA wave is never empty and never G plus a partly filled group (its
ranges there are 4, 8, 16, 20, 24, 32, 40, 48 or 56 rows), and the one range of WRW, [0, Pp), is never empty by construction.  The
DATA classes are therefore taken from the smallest shape that has them, R = 480 on a 1 x 1 grid with 8 channels on the other side (a
240 KB weight tensor: ranges of 18, 12 and 0 rows) — the one case outside the limits.
"""
import pytest
import torch

import fp32_conv_plan as P
from guarded import Arena

FORM_OPTION = 3           # ipsr_debug_set_option key: 0 = the shipped rule, 1 = staged in every call, 2 = gathered in every call
BAND = 2e-5               # tests/test_gpu_fp32_conv_variants.py: the fp32 kernels, times the fp64 convolution of the absolute values

gpu = pytest.mark.gpu


def group(op, nb):
    """Reduction elements per pipeline group: rows (DATA), columns (FWD), positions (WRW)."""
    if op == P.SM_FWD:
        return 16 if nb == 4 else 32
    return 8


def length_class(n, g):
    """'len0', or 'g<groups>' with a trailing 'p' when the last group is partly filled: g1p = below G, g1 = G, g2p = G plus a partial
    group, g2 = 2G, g3p = 2G plus a partial group ..."""
    if n == 0:
        return "len0"
    return "g%d%s" % (P.cdiv(n, g), "p" if n % g else "")


def wave_classes(op, case):
    plan = P.sm_plan(op, *P.sm_geometry(case))
    assert plan is not None, (op, case)
    return {length_class(b - a, group(op, plan["nb"])) for a, b in plan["waves"]}, plan


# id: (kind, Ci, Co, H, W, k, s, p, d, B) of the module, as in fp32_conv_plan.SM_CASES
CASES = {
    "conv8_32_2x2_k4s2_b1": ("conv", 8, 32, 2, 2, 4, 2, 1, 1, 1),            # 1 x 1 coarse grid, P = 1
    "conv120_64_4x4_k4s2_b3": ("conv", 120, 64, 4, 4, 4, 2, 1, 1, 3),        # B = 3; FWD: an idle wave, G + partial, 2G + partial
    "conv16_224_4x4_k4s2_b2": ("conv", 16, 224, 4, 4, 4, 2, 1, 1, 2),        # DATA: a wave of 4 rows, waves of 20
    "conv24_96_6x6_k4s2_b2": ("conv", 24, 96, 6, 6, 4, 2, 1, 1, 2),          # three full groups in DATA and FWD; WRW 2G + partial
    "conv56_32_6x6_k4s2_b3": ("conv", 56, 32, 6, 6, 4, 2, 1, 1, 3),          # P = 27: odd, the zero row; FWD below G
    "conv8_32_8x8_k4s2_b1": ("conv", 8, 32, 8, 8, 4, 2, 1, 1, 1),
    "conv8_32_6x8_k4s2_b2": ("conv", 8, 32, 6, 8, 4, 2, 1, 1, 2),            # non-square, P = 24
    "conv8_32_8x8_k4s2_b2": ("conv", 8, 32, 8, 8, 4, 2, 1, 1, 2),
    "conv8_32_12x12_k4s2_b1": ("conv", 8, 32, 12, 12, 4, 2, 1, 1, 1),
    "conv8_32_8x8_k4s2_b3": ("conv", 8, 32, 8, 8, 4, 2, 1, 1, 3),
    "conv16_128_12x12_k4s2_b2": ("conv", 16, 128, 12, 12, 4, 2, 1, 1, 2),
    "conv24_160_12x12_k4s2_b2": ("conv", 24, 160, 12, 12, 4, 2, 1, 1, 2),
    "conv40_192_12x12_k4s2_b2": ("conv", 40, 192, 12, 12, 4, 2, 1, 1, 2),
    "conv72_32_12x12_k4s2_b2": ("conv", 72, 32, 12, 12, 4, 2, 1, 1, 2),
    "conv88_32_11x11_k4s1_b3": ("conv", 88, 32, 11, 11, 4, 1, 1, 1, 3),
    "conv128_32_2x2_k3s1_b1": ("conv", 128, 32, 2, 2, 3, 1, 1, 1, 1),        # k = 3: four consecutive q cross a kernel row and a channel
    "convT32_128_2x2_k3s1_b3": ("convT", 32, 128, 2, 2, 3, 1, 1, 1, 3),
    "conv8_32_8x8_k4s2p3d2_b1": ("conv", 8, 32, 8, 8, 4, 2, 3, 2, 1),        # dilation 2
    "convT64_8_3x3_k4s2_b3": ("convT", 64, 8, 3, 3, 4, 2, 1, 1, 3),
    "conv8_480_2x2_k4s2_b1": ("conv", 8, 480, 2, 2, 4, 2, 1, 1, 1),          # outside the limits: DATA waves of 18, 12 and 0 rows
}
OUTSIDE_LIMITS = ("conv8_480_2x2_k4s2_b1",)
# the issue's six length classes first, then the group counts the three-set rotation adds
WANT = {
    P.SM_DATA: ("len0", "g1p", "g1", "g2p", "g2", "g3p", "g3", "g4", "g5", "g6"),
    P.SM_FWD: ("len0", "g1p", "g1", "g2p", "g2", "g3p", "g3", "g4", "g5", "g5p", "g6", "g6p"),
    P.SM_WRW: ("g1p", "g1", "g2p", "g2", "g3p", "g3", "g4", "g4p", "g5p", "g6"),
}
GUARDED = {P.SM_DATA: "conv8_480_2x2_k4s2_b1", P.SM_FWD: "conv120_64_4x4_k4s2_b3", P.SM_WRW: "conv56_32_6x6_k4s2_b3"}


# ---- without a GPU: the table reaches what it is there for ----------------------------------------------------------------------------------
def test_boundary_table_reaches_every_class():
    got = {op: set() for op in WANT}
    single = {op: set() for op in (P.SM_DATA, P.SM_FWD)}          # the same on the one-block kernels, which the training step runs
    for cid, case in CASES.items():
        geo = P.sm_geometry(case)
        B, R, Cq, Ho, Wo, Hf, Wf, k = geo[:8]
        if cid not in OUTSIDE_LIMITS:
            assert R <= 224 and Cq * k * k <= 2048 and max(Ho, Wo, Hf, Wf) <= 12, (cid, geo)
        for op in WANT:
            cl, plan = wave_classes(op, case)
            got[op] |= cl
            if op in single and plan["nb"] == 1:
                single[op] |= cl
    for op, want in WANT.items():
        assert set(want) <= got[op], (P.SM_OP_NAME[op], sorted(set(want) - got[op]))
    assert {"len0", "g1p", "g1", "g2p", "g2", "g3p", "g3"} <= single[P.SM_DATA], sorted(single[P.SM_DATA])
    assert {"len0", "g1p", "g1", "g2p", "g2", "g3p", "g3"} <= single[P.SM_FWD], sorted(single[P.SM_FWD])
    geos = {cid: P.sm_geometry(c) for cid, c in CASES.items()}
    assert any(g[3:5] == (1, 1) and g[7:10] == (4, 2, 1) for g in geos.values()), "no 1 x 1 coarse grid under k4 s2 p1"
    assert {1, 3} <= {g[0] for g in geos.values()}, "B = 1 and B = 3"
    assert any((g[0] * g[3] * g[4]) % 32 for g in geos.values()), "P no multiple of 32"
    assert any((g[0] * g[3] * g[4]) % 2 for g in geos.values()), "odd P: the zero row of Pp"
    assert any(g[3] != g[4] for g in geos.values()), "a non-square grid"
    assert {3, 4} <= {g[7] for g in geos.values()} and any(g[10] == 2 for g in geos.values())
    assert {c[0] for c in CASES.values()} == {"conv", "convT"}
    for op, cid in GUARDED.items():
        assert len(wave_classes(op, CASES[cid])[0]) >= (1 if op == P.SM_WRW else 3), (op, cid)


def test_classes_out_of_reach_inside_the_limits():
    """R <= 224, Q <= 2048, maps <= 12 x 12, B <= 3: no DATA wave is empty or G plus a partly filled group, whatever the geometry."""
    seen = set()
    for k, st, pad in ((4, 2, 1), (3, 1, 1), (4, 1, 1)):
        for R in range(32, 225, 32):
            for Cq in range(8, 2048 // (k * k) + 1, 8):
                if Cq * k * k % 128:
                    continue
                for H in range(1, 13):
                    for B in (1, 2, 3):
                        geo = P.sm_geometry(("conv", Cq, R, H, H, k, st, pad, 1, B))
                        if min(geo[3:7]) < 1:
                            continue
                        plan = P.sm_plan(P.SM_DATA, *geo)
                        if plan is not None:
                            seen |= {b - a for a, b in plan["waves"]}
    assert seen == {4, 8, 16, 20, 24, 32, 40, 48, 56}, sorted(seen)
    assert not any(length_class(n, 8) in ("len0", "g2p") for n in seen)
    cl, _ = wave_classes(P.SM_DATA, CASES["conv8_480_2x2_k4s2_b1"])
    assert {"len0", "g2p", "g3p"} <= cl, sorted(cl)


# ---- on the GPU ----------------------------------------------------------------------------------------------------------------------------
def _bits(t):
    return t.contiguous().view(torch.int32)


def _same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(_bits(a), _bits(b))


def _draw(shape, g, exact, weight=False):
    """Integers in [-3, 3] (activations, dy) / [-2, 2] (weights), or normal draws times a per-channel power of two in 2^-3 .. 2^3."""
    if exact:
        r = 2 if weight else 3
        return torch.randint(-r, r + 1, shape, device="cuda", generator=g).float()
    t = torch.randn(shape, device="cuda", generator=g)
    sshape = [1] * len(shape)
    sshape[0 if weight else 1] = shape[0 if weight else 1]
    return t * torch.exp2(torch.randint(-3, 4, tuple(sshape), device="cuda", generator=g).float())


def _module64(kind, x, w, dy, st, pad, dil):
    """fp64 on the GPU -> (y, dx, dw) of the module (Conv2d [Cout,Cin,k,k] / ConvTranspose2d [Cin,Cout,k,k], output_padding 0)."""
    tr = kind == "convT"
    xd, wd = x.double(), w.double()
    y = torch.nn.functional.conv_transpose2d(xd, wd, None, st, pad, 0, 1, dil) if tr else torch.nn.functional.conv2d(xd, wd, None, st, pad, dil)
    dx, dw, _ = torch.ops.aten.convolution_backward(dy.double(), xd, wd, None, [st, st], [pad, pad], [dil, dil], tr, [0, 0], 1, [True, True, False])
    return y, dx, dw


class _Case:
    """The tensors of one case in one regime and its fp64 references, computed once and left unchanged (one case stays resident)."""
    cache = {}

    def __init__(self, cid, case, exact):
        kind, Ci, Co, H, W, k, st, pad, dil, B = case
        tr = kind == "convT"
        g = torch.Generator(device="cuda").manual_seed(sum(map(ord, cid)) * 2 + exact)
        fop = P.CONVT_FWD if tr else P.CONV_FWD
        Hy, Wy = P.conv_out_dim(fop, H, k, st, pad, dil), P.conv_out_dim(fop, W, k, st, pad, dil)
        self.x = _draw((B, Ci, H, W), g, exact)
        self.w = _draw((Ci, Co, k, k) if tr else (Co, Ci, k, k), g, exact, weight=True)
        self.dy = _draw((B, Co, Hy, Wy), g, exact)
        y, dx, dw = _module64(kind, self.x, self.w, self.dy, st, pad, dil)
        ya, dxa, dwa = _module64(kind, self.x.abs(), self.w.abs(), self.dy.abs(), st, pad, dil)
        assert tuple(y.shape) == (B, Co, Hy, Wy)
        x, w, dy = self.x, self.w, self.dy
        # op -> (operands, reference, reference of the absolute values): tests/test_gpu_conv.py:244-263
        if tr:
            self.passes = {P.SM_DATA: ((x, w), y, ya), P.SM_WRW: ((x, dy), dw, dwa), P.SM_FWD: ((dy, w), dx, dxa)}
        else:
            self.passes = {P.SM_DATA: ((dy, w), dx, dxa), P.SM_WRW: ((dy, x), dw, dwa), P.SM_FWD: ((x, w), y, ya)}
        self.keep = [t.clone() for t in (x, w, dy)]

    @classmethod
    def get(cls, cid, case, exact):
        if (cid, exact) not in cls.cache:
            cls.cache.clear()
            cls.cache[(cid, exact)] = cls(cid, case, exact)
        return cls.cache[(cid, exact)]

    def unchanged(self):
        return all(_same(a, b) for a, b in zip((self.x, self.w, self.dy), self.keep))


def _set_option(value):
    from deepinpainting_amd import _lib
    _lib.check(_lib.lib().ipsr_debug_set_option(FORM_OPTION, value), "ipsr_debug_set_option")


ALL_CASES = {**{cid: c for cid, (c, _) in P.SM_CASES.items()}, **CASES}
REGIMES = [pytest.param(True, id="exact"), pytest.param(False, id="real")]


@gpu
@pytest.mark.parametrize("exact", REGIMES)
@pytest.mark.parametrize("cid", list(ALL_CASES))
def test_gathered_equals_staged(cid, exact):
    """All three ops: the default (gathered) result against the one with the pre-pass launches, bit for bit; the real-valued regime is
    also held to the band of tests/test_gpu_fp32_conv_variants.py so that the common result is a right one."""
    from deepinpainting_amd import _lib, ops
    case = ALL_CASES[cid]
    geo = P.sm_geometry(case)
    t = _Case.get(cid, case, exact)
    try:
        for op, (operands, want, wabs) in t.passes.items():
            assert ops.smallmap_supported(op, *geo)
            _set_option(1)
            staged = ops.conv_smallmap(op, *operands, *geo)
            _set_option(2)
            gathered = ops.conv_smallmap(op, *operands, *geo)
            _set_option(0)
            assert _same(ops.conv_smallmap(op, *operands, *geo), staged), "%s:%s: the default differs from staged" % (cid, P.SM_OP_NAME[op])
            tag = "%s:%s" % (cid, P.SM_OP_NAME[op])
            if not _same(gathered, staged):
                bad = (_bits(gathered) != _bits(staged)).nonzero()
                raise AssertionError("%s: %d of %d elements differ between gathered and staged, first at %s: %r != %r" % (
                    tag, bad.shape[0], staged.numel(), bad[0].tolist(), float(gathered[tuple(bad[0])]), float(staged[tuple(bad[0])])))
            if exact:
                assert float(wabs.max()) < 2.0 ** 24
                assert _same(gathered + 0, want.float() + 0), "%s: not the exact result" % tag
            else:
                worst = float(((gathered.double() - want).abs() / (BAND * wabs).clamp_min(1e-300)).max())
                print("%s: max |err| / band %.3f" % (tag, worst))
                assert bool(torch.isfinite(gathered).all()) and worst <= 1.0, (tag, worst)
    finally:
        _lib.lib().ipsr_debug_set_option(FORM_OPTION, 0)
    assert t.unchanged()


@gpu
@pytest.mark.parametrize("cid", list(CASES))
def test_pipeline_boundaries_exact(cid, monkeypatch):
    """The boundary table against torch fp64 in the exact regime, every op; two calls give the same bits; the most ragged case of each
    op once more between guard bands with NaN-filled scratch of exactly the size the query asks for."""
    from deepinpainting_amd import ops
    case = CASES[cid]
    geo = P.sm_geometry(case)
    t = _Case.get(cid, case, True)
    for op, (operands, want, wabs) in t.passes.items():
        tag = "%s:%s" % (cid, P.SM_OP_NAME[op])
        classes, plan = wave_classes(op, case)
        assert float(wabs.max()) < 2.0 ** 24, (tag, float(wabs.max()))
        run = lambda a, b: ops.conv_smallmap(op, a, b, *geo)
        y = run(*operands)
        ref = want.float()
        assert y.shape == ref.shape and y.dtype == torch.float32, (tag, y.shape, ref.shape)
        if not _same(y + 0, ref + 0):
            bad = (y.double() != ref.double()).nonzero()
            raise AssertionError("%s (%s): %d of %d elements differ from the exact result, first at %s: %r != %r" % (
                tag, sorted(classes), bad.shape[0], y.numel(), bad[0].tolist(), float(y[tuple(bad[0])]), float(ref[tuple(bad[0])])))
        assert _same(run(*operands), y), "%s: two calls differ" % tag
        if GUARDED[op] == cid:
            arena = Arena(ws_fill="nan")
            copies = [arena.guarded_copy(o, "in%d" % i) for i, o in enumerate(operands)]
            with arena.installed(monkeypatch):
                yg = run(*copies)
            torch.cuda.synchronize()
            arena.check_guards()
            assert all(_same(c, o) for c, o in zip(copies, operands)), "%s: an input was modified" % tag
            assert _same(yg, y), "%s: the guarded run differs" % tag
            assert arena.workspaces and arena.workspaces[0][0] == plan["ws"], (arena.workspaces and arena.workspaces[0][0], plan["ws"])
    assert t.unchanged()
