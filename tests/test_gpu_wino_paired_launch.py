"""csrc/winograd.hip, paired launches: the two transforms of a convolution that do not depend on each other (filter || input or
window transform of the data passes, tile || window transform of the weight gradients) run as one 1-D grid (wino_pair_kernel);
debug option 2 puts them back on two launches.  The arithmetic of every body is untouched, so for every entry that launches a pair

  * the output with the pair equals the output with two launches BIT FOR BIT (the two-launch path runs the same bodies on the
    grids and in the order the stand-alone kernels always had),
  * one case per family is also held to the fp64 band of tests/test_gpu_conv.py (1e-4), so that "equal to the other path" is not
    the only anchor,
  * every operand sits between guard bands and the scratch is exactly the queried size, NaN-poisoned (tests/guarded.py): a block of
    the merged grid decoded to the wrong coordinates writes a guard, leaves a padded row unwritten (NaN through the GEMM) or
    writes another block's rows (outputs differ).

Shapes, all B <= 2 and <= 256 channels (rp = (reduction, produced) channels of the GEMM):
  filter part as large as the data part (256 x 256 channels on one 128-tile block), data part far larger (16 x 16 channels on a
  64 x 64 map, B = 2); produced channels 63 / 64 / 65 / 129 (both values of wino_rows_padded: 64 rows and multiples of 128);
  reduction channels 16 and 48; tile counts below 128 and just above (36 x 36 with B = 2: 162 tiles of 4 x 4, 288 of 3 x 3); odd
  extents; nh / nw of 5, 6 and 16 for the stride-2 family; weight gradients whose tile operand has more blocks than the window
  operand and the other way round (the pair puts the longer one first).  The number of blocks of a remapped first part is always
  a multiple of 8 here (reductions are multiples of 16, tile counts of 128), so xcd_remap's ragged branch cannot be reached
  through these entries.
The 3x3 filter transform reads its taps through LDS where the produced channel is the weight's inner index (Conv2d backward-data,
ConvTranspose2d forward; the 4x4 family: backward-data) and directly elsewhere: all four ops / both modes are in every list."""
import pytest
import torch
import torch.nn.functional as F

from guarded import Arena, _bits

pytestmark = pytest.mark.gpu

PAIR_OPTION = 2          # ipsr_debug_set_option key: 1 = two launches


@pytest.fixture(autouse=True)
def _paired_by_default():
    yield
    from deepinpainting_amd import _lib
    _lib.lib().ipsr_debug_set_option(PAIR_OPTION, 0)


def _randn(shape, seed, scale=1.0):
    return (torch.randn(shape, generator=torch.Generator().manual_seed(seed)) * scale).cuda()


def _both_ways(monkeypatch, operands, call):
    """call(*guarded operands) with the pair and with two launches, each in a fresh arena -> (paired, two launches)."""
    from deepinpainting_amd import _lib
    outs = []
    for two in (0, 1):
        _lib.check(_lib.lib().ipsr_debug_set_option(PAIR_OPTION, two), "ipsr_debug_set_option")
        arena = Arena(ws_fill="nan")
        ops_ = [arena.guarded_copy(t, "operand%d" % i) for i, t in enumerate(operands)]
        with arena.installed(monkeypatch):
            out = call(*ops_)
        torch.cuda.synchronize()
        arena.check_guards()
        assert arena.workspaces, "the call took no workspace from the arena"
        assert not torch.isnan(out.float()).any(), "poisoned scratch reached the output"
        for t, g in zip(operands, ops_):
            assert torch.equal(_bits(t), _bits(g)), "an operand was written"
        outs.append(out)
    _lib.lib().ipsr_debug_set_option(PAIR_OPTION, 0)
    assert outs[0].dtype == outs[1].dtype and torch.equal(_bits(outs[0]), _bits(outs[1])), "paired launch != two launches"
    return outs


def _rel(a, b):
    return float((a.double().cpu() - b).abs().max() / b.abs().max().clamp_min(1e-30))


# (B, reduction channels, produced channels, H, W)
RP = [(1, 256, 256, 4, 4), (2, 16, 16, 64, 64), (2, 48, 63, 36, 36), (1, 16, 64, 9, 13), (2, 48, 65, 12, 20), (1, 16, 129, 8, 8)]
SPLIT = [(2, 48, 65, 12, 20, "bf16x3"), (1, 16, 129, 9, 13, "bf16x6")]


def _ids(v):
    return "x".join(str(e) for e in v) if isinstance(v, tuple) else None


# ---- 3x3 data passes: the four layouts of ipsr_conv3x3_winograd_mp -----------------------------------------------------------------
@pytest.mark.parametrize("op", [0, 1, 2, 3], ids=["conv_fwd", "conv_bwd", "convT_fwd", "convT_bwd"])
@pytest.mark.parametrize("case", [c + ("fp32",) for c in RP] + SPLIT, ids=_ids)
def test_conv3x3_data_pass_pair_equals_two_launches(monkeypatch, op, case):
    from deepinpainting_amd import ops
    B, red, prod, H, W, math = case
    fwd = op in (ops.CONV_FWD, ops.CONVT_FWD)
    Cin, Cout = (red, prod) if fwd else (prod, red)
    assert ops.winograd_supported(op, B, Cin, H, W, Cout)
    inp = _randn((B, red, H, W), 11 * red + H)
    w = _randn((Cout, Cin, 3, 3) if op in (ops.CONV_FWD, ops.CONV_BWD_DATA) else (Cin, Cout, 3, 3), 13 * prod + W, 0.1)
    y, _ = _both_ways(monkeypatch, (inp, w), lambda a, b: ops.conv3x3_winograd(op, a, b, (B, Cin, H, W), Cout, math=math))
    if case == RP[2] + ("fp32",):            # the fp64 anchor of the family, every layout
        xd, wd = inp.double().cpu(), w.double().cpu()
        if op == ops.CONV_FWD:
            ref = F.conv2d(xd, wd, None, 1, 1)
        elif op == ops.CONVT_FWD:
            ref = F.conv_transpose2d(xd, wd, None, 1, 1)
        elif op == ops.CONV_BWD_DATA:       # dx of y = conv2d(x, w) is the transposed convolution of dy
            ref = F.conv_transpose2d(xd, wd, None, 1, 1)
        else:
            ref = F.conv2d(xd, wd, None, 1, 1)
        assert _rel(y, ref) <= 1e-4


@pytest.mark.parametrize("op", [0, 1], ids=["conv_fwd_direct_taps", "conv_bwd_taps_through_lds"])
def test_conv3x3_filter_cache_with_the_pair(monkeypatch, op):
    """filter_cache: the invalid call fills it through the pair's filter part with the very bits the stand-alone filter kernel
    writes; the valid call launches the input part alone (a poisoned word of the cache survives it) and gives the same output."""
    from deepinpainting_amd import _lib, ops
    B, red, prod, H, W = 2, 48, 65, 12, 20
    Cin, Cout = (red, prod) if op == ops.CONV_FWD else (prod, red)
    inp, w = _randn((B, red, H, W), 5), _randn((Cout, Cin, 3, 3), 6, 0.1)
    L = _lib.lib()
    res = {}
    for two in (1, 0):
        _lib.check(L.ipsr_debug_set_option(PAIR_OPTION, two), "ipsr_debug_set_option")
        arena = Arena(ws_fill="nan")
        x, wt = arena.guarded_copy(inp, "in"), arena.guarded_copy(w, "w")
        with arena.installed(monkeypatch):
            cache = ops.winograd_filter_cache(op, Cin, Cout, x.device)           # NaN-filled by the arena
            y0 = ops.conv3x3_winograd(op, x, wt, (B, Cin, H, W), Cout, filter_cache=cache)
            filled = cache.clone()
            y1 = ops.conv3x3_winograd(op, x, wt, (B, Cin, H, W), Cout, filter_cache=cache, filter_cache_valid=True)
            assert torch.equal(_bits(cache), _bits(filled))
            cache[7] = 123.0                                                       # a word the filter part would overwrite
            poisoned = cache.clone()
            ops.conv3x3_winograd(op, x, wt, (B, Cin, H, W), Cout, filter_cache=cache, filter_cache_valid=True)
            assert torch.equal(_bits(cache), _bits(poisoned)), "the valid call ran a filter part"
        torch.cuda.synchronize()
        arena.check_guards()
        assert torch.equal(_bits(y0), _bits(y1)) and not torch.isnan(y0).any()
        assert float(filled[7]) != 123.0
        res[two] = (y0, filled)
    assert torch.equal(_bits(res[0][0]), _bits(res[1][0])), "outputs differ between the pair and two launches"
    assert torch.equal(_bits(res[0][1]), _bits(res[1][1])), "the pair fills the filter cache differently"
    plain = ops.conv3x3_winograd(op, inp, w, (B, Cin, H, W), Cout)
    assert torch.equal(_bits(plain), _bits(res[0][0]))


# ---- 3x3 weight gradient ------------------------------------------------------------------------------------------------------------
# (B, Cin, H, W, Cout): the last two: more tile-operand blocks than window-operand blocks, and the reverse
WRW = [(1, 256, 4, 4, 256), (2, 16, 64, 64, 16), (2, 48, 36, 36, 63), (1, 20, 9, 13, 64), (2, 48, 12, 20, 65), (1, 16, 8, 8, 129),
       (2, 16, 12, 12, 256), (2, 256, 12, 12, 16)]


@pytest.mark.parametrize("transposed", [0, 1], ids=["conv", "convT"])
@pytest.mark.parametrize("case", [c + ("fp32",) for c in WRW] + [(2, 48, 12, 20, 65, "bf16x3"), (2, 16, 12, 12, 256, "bf16x6"), (2, 256, 12, 12, 16, "bf16x6")], ids=_ids)
def test_conv3x3_weight_gradient_pair_equals_two_launches(monkeypatch, transposed, case):
    from deepinpainting_amd import ops
    B, Cin, H, W, Cout, math = case
    x, dy = _randn((B, Cin, H, W), 3 * Cin + H), _randn((B, Cout, H, W), 7 * Cout + W)
    dw, _ = _both_ways(monkeypatch, (x, dy), lambda a, b: ops.conv3x3_winograd_wrw(bool(transposed), a, b, Cout, math=math))
    if case == WRW[2] + ("fp32",):
        xd, dyd = x.double().cpu(), dy.double().cpu()
        wd = torch.zeros((Cin, Cout, 3, 3) if transposed else (Cout, Cin, 3, 3), dtype=torch.float64, requires_grad=True)
        y = F.conv_transpose2d(xd, wd, None, 1, 1) if transposed else F.conv2d(xd, wd, None, 1, 1)
        (ref,) = torch.autograd.grad(y, wd, dyd)
        assert tuple(dw.shape) == tuple(ref.shape) and _rel(dw, ref) <= 1e-4


# ---- 4x4 on 3x3 tiles: geometry 0 (k4 s2 p3 d2, even extents) and 1 (k4 s1 p1) x modes 0 / 1 / 2 ---------------------------------------
RP4 = {0: [(1, 256, 256, 8, 8), (2, 16, 16, 64, 64), (2, 48, 63, 72, 72), (1, 16, 64, 14, 22), (2, 48, 65, 24, 40), (1, 16, 129, 16, 16)],
       1: [(1, 256, 256, 5, 5), (2, 16, 16, 64, 64), (2, 48, 63, 37, 37), (1, 16, 64, 9, 13), (2, 48, 65, 12, 20), (1, 16, 129, 8, 8)]}


@pytest.mark.parametrize("geom", [0, 1], ids=["k4s2p3d2", "k4s1p1"])
@pytest.mark.parametrize("mode", [0, 1, 2], ids=["fwd", "bwd_data", "wrw"])
@pytest.mark.parametrize("idx", list(range(6)) + ["bf16x3"])
def test_conv4x4_pair_equals_two_launches(monkeypatch, geom, mode, idx):
    from deepinpainting_amd import ops
    math = "fp32" if isinstance(idx, int) else idx
    B, red, prod, H, W = RP4[geom][idx if isinstance(idx, int) else 4]
    Cin, Cout = (prod, red) if mode == 1 else (red, prod)
    Ho, Wo = (H // 2, W // 2) if geom == 0 else (H - 1, W - 1)
    assert ops.dilated_winograd_supported(mode, B, Cin, H, W, Cout, geom=geom)
    x, dy = _randn((B, Cin, H, W), 3 * Cin + H), _randn((B, Cout, Ho, Wo), 5 * Cout + W)
    w = _randn((Cout, Cin, 4, 4), Cin + Cout, 0.1)
    a, b = {0: (x, w), 1: (dy, w), 2: (x, dy)}[mode]
    got, _ = _both_ways(monkeypatch, (a, b), lambda p, q: ops.conv4x4_dilated_winograd(mode, p, q, (B, Cin, H, W), Cout, geom=geom, math=math))
    if idx == 2:
        st, pad, dil = (2, 3, 2) if geom == 0 else (1, 1, 1)
        xd, wd = x.double().cpu().requires_grad_(True), w.double().cpu().requires_grad_(True)
        y64 = F.conv2d(xd, wd, None, st, pad, dil)
        dx64, dw64 = torch.autograd.grad(y64, (xd, wd), dy.double().cpu())
        assert _rel(got, (y64.detach(), dx64, dw64)[mode]) <= 1e-4


# ---- 4x4 stride 2 (polyphase): modes 0 / 1 / 2 ----------------------------------------------------------------------------------------
# (B, Kc, Cf, nh, nw).  mode 0 reduces 4*Cf and produces Kc; mode 1 reduces Kc (a multiple of 16) and produces 4*Cf (60 / 64 / 68 / 132)
# The weight gradient (any channel counts) takes the list of mode 0 and two shapes whose tile / window operand is the longer one.
S2 = {0: [(1, 256, 64, 5, 6), (2, 16, 16, 32, 32), (2, 63, 12, 16, 16), (1, 64, 4, 6, 5), (2, 65, 12, 6, 16), (1, 129, 4, 5, 5)],
      1: [(1, 256, 64, 5, 6), (2, 16, 16, 32, 32), (2, 48, 15, 16, 16), (1, 16, 16, 6, 5), (2, 48, 17, 6, 16), (1, 16, 33, 5, 5)]}
S2[2] = S2[0] + [(2, 256, 4, 6, 6), (2, 16, 64, 6, 6)]
S2_SPLIT = {0: (2, 64, 16, 6, 16), 1: (2, 48, 32, 6, 16), 2: (2, 65, 12, 6, 16)}
S2_CASES = [(m, i) for m in (0, 1, 2) for i in list(range(len(S2[m]))) + ["bf16x3"]]


@pytest.mark.parametrize("mode,idx", S2_CASES, ids=["%s-%s" % (("fine_to_coarse", "coarse_to_fine", "wrw")[m], i) for m, i in S2_CASES])
def test_conv4x4s2_pair_equals_two_launches(monkeypatch, mode, idx):
    from deepinpainting_amd import ops
    math = "fp32" if isinstance(idx, int) else idx
    B, Kc, Cf, nh, nw = S2[mode][idx] if isinstance(idx, int) else S2_SPLIT[mode]
    assert ops.s2_winograd_supported(mode, B, Kc, Cf, nh, nw)
    fine, coarse = _randn((B, Cf, 2 * nh, 2 * nw), 3 * Cf + nh), _randn((B, Kc, nh, nw), 5 * Kc + nw)
    w = _randn((Kc, Cf, 4, 4), Kc + Cf, 0.1)
    a, b = {0: (fine, w), 1: (coarse, w), 2: (fine, coarse)}[mode]
    got, _ = _both_ways(monkeypatch, (a, b), lambda p, q: ops.conv4x4s2_winograd(mode, p, q, B, Kc, Cf, nh, nw, math=math))
    if idx == 2:
        fd, wd = fine.double().cpu().requires_grad_(True), w.double().cpu().requires_grad_(True)
        y64 = F.conv2d(fd, wd, None, 2, 1)
        dx64, dw64 = torch.autograd.grad(y64, (fd, wd), coarse.double().cpu())
        ref = (y64.detach(), dx64, dw64)[mode]
        assert _rel(got, ref) <= 1e-4
