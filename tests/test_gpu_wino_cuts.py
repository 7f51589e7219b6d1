"""Every Winograd reduction cut, on every planner and pass, against fp64.

The 36 GEMMs of a Winograd convolution may cut their reduction over workgroups; the output transforms then add the slabs of each
point (wino_load_sum, WinoSplit::of / slabs in csrc/winograd.hip).  wino_choose_split picks the cut with a timing
model, so the cuts today's layers land on are an accident of that model.  Here ipsr_debug_force_wino_split forces each cut form on
every planner (its workspace queries included) and ipsr_wino_gemm_split confirms, before each numeric check, that the force took
effect at that pass's stage count (the chooser ignores a force larger than the stage count).

  cut form (force nsplit, xi_split, nsplit_t)         ranges at S stages                 case
  --------------------------------------------------  ---------------------------------  -----------------------------------
  uncut                        (1, 36, 1)             S                                  cut "uncut" in every test below
  uniform, 2 ranges            (2, 36, 2)             even at S = 6, 8; 3 + 2 at S = 5   cut "uniform2"
  uniform, 3 ranges            (3, 36, 3)             3 + 3 + 2 at S = 8; 2+2+1 at S = 5 cut "uniform3"
  finest: one stage per range  (S, 36, S)             1 x S                              cut "finest"
  head / tail, xi_split 1      (1, 1, 3), (S, 1, 2)   head uncut / tail finer, and back  cuts "ht1_fine_tail", "ht1_fine_head"
  head / tail, xi_split 32     (3, 32, 1)             head finer than the tail           cut "ht32_fine_head"
  head / tail, xi_split 35     (2, 35, S)             tail finer than the head           cut "ht35_fine_tail"
  (test_every_cut_form_is_reached asserts that the passes below meet an even and an uneven uniform cut and both head/tail orders.)

  planner / pass (the split of each is chosen in wino_plan_gemm, called by)         test id (family), passes
  -----------------------------------------------  --------------------  ---------------------------------------------------
  3x3 Conv2d / ConvTranspose2d fwd, input grad     wino_plan             k3_conv*, k3_convT*: fwd, bwd_data
  3x3 weight gradient                              wino_wrw_plan         k3_conv*, k3_convT*: wrw
  k4 s2 p3 d2 (geometry 0), k4 s1 p1 (geometry 1)  dil_plan              dil_g0*, dil_g1*: mode 0, 1, 2
  k4 s2 p1 polyphase F(5x5, 2x2)                   s2_plan               s2*: mode 0, 1, 2

  arithmetic                                       GEMM kernel (launch_wino_gemm)                            tests
  -----------------------------------------------  --------------------------------------------------------  ------------------------
  fp32, <= 64 produced channels                    wino_gemm_kernel<64>                                      *-narrow-fp32 (fwd, wrw)
  fp32, > 64 produced channels                     wino_gemm_kernel<128>                                     *-wide-fp32, narrow bwd
  split bf16 x6 / x3                               wino_gemm_split_kernel<3> / <2>                           *-wide-bf16x6, *-wide-bf16x3
  bf16 activations in and out                      the same kernels, bf16 transforms                        k3_conv-wide-fp32-bf16io,
                                                                                                             s2-wide-bf16x3-bf16io
Shapes are small (5-8 reduction stages, 80-128 channels, ragged maps, batch 2-3) so the fp64 CPU reference is cheap.  Bands are
those of test_split_bf16_winograd_arithmetic_all_families: 1e-4 of the result's scale for fp32 and x6, 1e-3 for x3, plus 2^-8 for
bf16 outputs.

The force is process-global: every test resets it in a `finally`, and the module's autouse fixture fails a test after which the
automatic answer of ipsr_wino_gemm_split differs from before it (a leaked force would otherwise change the rest of the suite).
"""
import ctypes

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

# shapes at which the automatic rule takes each of its branches (wino_choose_split): uncut, head/tail, uniform
AUTO_PROBES = [(128, 128, 256), (512, 512, 512), (256, 512, 1024), (256, 2048, 256), (128, 128, 8192)]


def _lib():
    from deepinpainting_amd import _lib as lib
    return lib


def query(rows, cols, red):
    lib = _lib()
    out = (ctypes.c_int * 5)()
    lib.check(lib.lib().ipsr_wino_gemm_split(rows, cols, red, ctypes.cast(out, ctypes.c_void_p)), "ipsr_wino_gemm_split")
    return tuple(out)


def force(a, x, b):
    lib = _lib()
    lib.check(lib.lib().ipsr_debug_force_wino_split(a, x, b), "ipsr_debug_force_wino_split")


@pytest.fixture(autouse=True)
def automatic_rule_unchanged():
    before = [query(*p) for p in AUTO_PROBES]
    yield
    after = [query(*p) for p in AUTO_PROBES]
    assert after == before, "a forced Winograd cut leaked out of the test: %s -> %s" % (before, after)


def cdiv(a, b):
    return -(-a // b)


def forced_split(S, a, x, b):
    """What wino_choose_split returns under force (a, x, b) at S stages (the force branch of wino_choose_split in winograd.hip)."""
    pa, pb = cdiv(S, a), cdiv(S, b)
    return (cdiv(S, pa), pa, x, cdiv(S, pb), pb)


def cuts(S):
    """The cut forms of the module table at S stages: name -> force."""
    return {"uncut": (1, 36, 1), "uniform2": (2, 36, 2), "uniform3": (min(3, S), 36, min(3, S)), "finest": (S, 36, S),
            "ht1_fine_tail": (1, 1, min(3, S)), "ht1_fine_head": (S, 1, 2), "ht32_fine_head": (min(3, S), 32, 1),
            "ht35_fine_tail": (2, 35, S)}


def ranges(S, n, per):
    return [per] * (n - 1) + [S - per * (n - 1)]


def rows_padded(K, math):
    """wino_rows_padded (winograd.hip): the <64> tile for fp32 arithmetic on <= 64 produced channels."""
    return 64 if (math == "fp32" and K <= 64) else cdiv(K, 128) * 128


def gemm_kernel(prod, math):
    if math != "fp32":
        return "split<%d>" % {"bf16x3": 2, "bf16x6": 3}[math]
    return "<64>" if rows_padded(prod, math) == 64 else "<128>"


def wrw_stages(T):
    """Weight-gradient planners: the reduction runs over Tp = roundup(T, 128) tiles in stages of 16 (wino_plan_tiles; red = Tp in wino_wrw_plan, dil_plan and s2_plan)."""
    return cdiv(T, 128) * 128 // 16


# ---- the passes of each family: (pass name, stages, produced channels, fn(math, operands) -> result, fp64 reference) ------------------
def _randn(g, *shape, scale=1.0):
    return torch.randn(*shape, generator=g) * scale


def family_passes(family, shape, io_bf16, seed):
    """Operands (bf16-rounded where the activations are bf16) and the passes of one family on one shape."""
    from deepinpainting_amd import ops
    g = torch.Generator().manual_seed(seed)
    act = torch.bfloat16 if io_bf16 else torch.float32

    def A(*s):                  # an activation operand: on the GPU in its dtype, and its exact fp64 value
        t = _randn(g, *s).to(act)
        return t.cuda(), t.double()

    def Wt(*s):
        t = _randn(g, *s, scale=0.1)
        return t.cuda(), t.double()

    passes = []
    if family in ("k3_conv", "k3_convT"):
        tr = family == "k3_convT"
        B, Cin, H, W, Cout = shape
        (x, x64), (dy, dy64) = A(B, Cin, H, W), A(B, Cout, H, W)
        w, w64 = Wt(*((Cin, Cout, 3, 3) if tr else (Cout, Cin, 3, 3)))
        f = (lambda a, ww: F.conv_transpose2d(a, ww, None, 1, 1)) if tr else (lambda a, ww: F.conv2d(a, ww, None, 1, 1))
        fop, bop = (ops.CONVT_FWD, ops.CONVT_BWD_DATA) if tr else (ops.CONV_FWD, ops.CONV_BWD_DATA)
        xr, wr = x64.clone().requires_grad_(True), w64.clone().requires_grad_(True)
        y64 = f(xr, wr)
        dx64, dw64 = torch.autograd.grad(y64, (xr, wr), dy64)
        T = B * cdiv(H, 4) * cdiv(W, 4)
        passes += [("fwd", Cin // 16, Cout, lambda m: ops.conv3x3_winograd(fop, x, w, (B, Cin, H, W), Cout, math=m), y64.detach(), True),
                   ("bwd_data", Cout // 16, Cin, lambda m: ops.conv3x3_winograd(bop, dy, w, (B, Cin, H, W), Cout, math=m), dx64, True),
                   ("wrw", wrw_stages(T), Cin if tr else Cout, lambda m: ops.conv3x3_winograd_wrw(tr, x, dy, Cout, math=m), dw64, False)]
    elif family in ("dil_g0", "dil_g1"):
        geom = 0 if family == "dil_g0" else 1
        B, Cin, H, W, Cout = shape
        st_, pad, dil = (2, 3, 2) if geom == 0 else (1, 1, 1)
        Ho, Wo = (H // 2, W // 2) if geom == 0 else (H - 1, W - 1)
        (x, x64), (dy, dy64) = A(B, Cin, H, W), A(B, Cout, Ho, Wo)
        w, w64 = Wt(Cout, Cin, 4, 4)
        xr, wr = x64.clone().requires_grad_(True), w64.clone().requires_grad_(True)
        y64 = F.conv2d(xr, wr, None, st_, pad, dil)
        dx64, dw64 = torch.autograd.grad(y64, (xr, wr), dy64)
        T = B * cdiv(Ho, 3) * cdiv(Wo, 3)                                                    # dil_plan (winograd.hip)
        call = ops.conv4x4_dilated_winograd
        passes += [("mode0", Cin // 16, Cout, lambda m: call(0, x, w, (B, Cin, H, W), Cout, geom=geom, math=m), y64.detach(), True),
                   ("mode1", Cout // 16, Cin, lambda m: call(1, dy, w, (B, Cin, H, W), Cout, geom=geom, math=m), dx64, True),
                   ("mode2", wrw_stages(T), Cout, lambda m: call(2, x, dy, (B, Cin, H, W), Cout, geom=geom, math=m), dw64, False)]
    else:
        B, Kc, Cf, nh, nw = shape
        (fine, f64), (coarse, c64) = A(B, Cf, 2 * nh, 2 * nw), A(B, Kc, nh, nw)
        w, w64 = Wt(Kc, Cf, 4, 4)
        fr, wr = f64.clone().requires_grad_(True), w64.clone().requires_grad_(True)
        y64 = F.conv2d(fr, wr, None, 2, 1)
        dx64, dw64 = torch.autograd.grad(y64, (fr, wr), c64)
        T = B * cdiv(nh, 5) * cdiv(nw, 5)                                                    # s2_plan (winograd.hip)
        call = ops.conv4x4s2_winograd
        passes += [("mode0", 4 * Cf // 16, Kc, lambda m: call(ops.S2_FINE_TO_COARSE, fine, w, B, Kc, Cf, nh, nw, math=m), y64.detach(), True),
                   ("mode1", Kc // 16, 4 * Cf, lambda m: call(ops.S2_COARSE_TO_FINE, coarse, w, B, Kc, Cf, nh, nw, math=m), dx64, True),
                   ("mode2", wrw_stages(T), Kc, lambda m: call(ops.S2_WEIGHT_GRAD, fine, coarse, B, Kc, Cf, nh, nw, math=m), dw64, False)]
    return passes


# family -> {"wide": every pass produces > 64 channels (<128> tile), "narrow": forward / weight gradient produce <= 64 (<64> tile)}
SHAPES = {
    "k3_conv": {"wide": (2, 96, 9, 13, 80), "narrow": (2, 112, 11, 6, 48)},       # (B, Cin, H, W, Cout)
    "k3_convT": {"wide": (3, 80, 7, 11, 96), "narrow": (2, 96, 10, 9, 64)},
    "dil_g0": {"wide": (2, 96, 14, 10, 80), "narrow": (3, 80, 8, 12, 48)},
    "dil_g1": {"wide": (2, 96, 9, 12, 80), "narrow": (2, 80, 11, 7, 48)},
    "s2": {"wide": (2, 96, 24, 7, 6), "narrow": (3, 48, 20, 6, 9)},               # (B, Kc, Cf, nh, nw)
}
CASES = [(fam, "wide", m, False) for fam in SHAPES for m in ("fp32", "bf16x6", "bf16x3")]
CASES += [(fam, "narrow", "fp32", False) for fam in SHAPES]
CASES += [("k3_conv", "wide", "fp32", True), ("s2", "wide", "bf16x3", True)]


def _rel(a, b):
    return float((a.double().cpu() - b).abs().max() / b.abs().max())


@pytest.mark.parametrize("family,size,math,io_bf16", CASES,
                         ids=["%s-%s-%s%s" % (f, s, m, "-bf16io" if io else "") for f, s, m, io in CASES])
def test_every_cut_on_every_pass_vs_fp64(family, size, math, io_bf16):
    tol = {"fp32": 1e-4, "bf16x6": 1e-4, "bf16x3": 1e-3}[math]
    passes = family_passes(family, SHAPES[family][size], io_bf16, seed=sum(SHAPES[family][size]) * 31 + len(family))
    tiles = set()
    try:
        for name, S, prod, fn, ref, act_out in passes:
            assert 3 <= S <= 8, (family, name, S)
            tiles.add(gemm_kernel(prod, math))
            otol = tol + (2.0 ** -8 if (io_bf16 and act_out) else 0.0)
            for cut, (a, x, b) in cuts(S).items():
                force(a, x, b)
                want = forced_split(S, a, x, b)
                assert query(128, 128, 16 * S) == want, (family, name, cut, want)       # the force holds at this stage count
                got = fn(math)
                torch.cuda.synchronize()
                assert got.dtype == (torch.bfloat16 if (io_bf16 and act_out) else torch.float32)
                err = _rel(got, ref)
                assert err <= otol, (family, size, math, name, cut, want, err)
    finally:
        force(0, 0, 0)
    if math == "fp32" and size == "narrow":
        assert tiles == {"<64>", "<128>"}, tiles            # the forward / weight gradient on <64>, the input gradient on <128>
    elif math == "fp32":
        assert tiles == {"<128>"}, tiles
    else:
        assert tiles == {gemm_kernel(128, math)}


def test_every_cut_form_is_reached():
    """Across the passes above: uniform cuts with an even and with an uneven last range, the finest cut, and head/tail cuts at
    xi_split 1, 32 and 35 with the head cut finer than the tail and the other way round."""
    seen = set()
    for fam, sizes in SHAPES.items():
        for shape in sizes.values():
            B = shape[0]
            if fam.startswith("k3"):
                _, Cin, H, W, Cout = shape
                stages = [Cin // 16, Cout // 16, wrw_stages(B * cdiv(H, 4) * cdiv(W, 4))]
            elif fam.startswith("dil"):
                _, Cin, H, W, Cout = shape
                Ho, Wo = (H // 2, W // 2) if fam == "dil_g0" else (H - 1, W - 1)
                stages = [Cin // 16, Cout // 16, wrw_stages(B * cdiv(Ho, 3) * cdiv(Wo, 3))]
            else:
                _, Kc, Cf, nh, nw = shape
                stages = [4 * Cf // 16, Kc // 16, wrw_stages(B * cdiv(nh, 5) * cdiv(nw, 5))]
            for S in stages:
                for cut, f in cuts(S).items():
                    n, per, x, nt, pert = forced_split(S, *f)
                    r = ranges(S, n, per)
                    if x >= 36 and n > 1:
                        seen.add("uniform_even" if len(set(r)) == 1 else "uniform_uneven")
                    if x >= 36 and per == 1 and n == S:
                        seen.add("finest")
                    if x < 36 and n != nt:
                        seen.add("ht%d_%s" % (x, "fine_head" if n > nt else "fine_tail"))
    assert {"uniform_even", "uniform_uneven", "finest", "ht1_fine_head", "ht1_fine_tail", "ht32_fine_head", "ht35_fine_tail"} <= seen, seen
