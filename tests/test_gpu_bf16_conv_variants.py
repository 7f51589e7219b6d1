"""Every launch variant of the direct bf16 convolutions (csrc/conv_bf16.hip) against fp64.

The launchers choose a kernel instantiation and an LDS plan from the shape alone: `conv_bf16_kernel<MODE, KT, P, TOUT>` (MODE S1 /
F2C / C2F, KT 128 or 64, P 256 or 512 pixels per tile, one raw buffer `raw1`, a reduction cut into 1..4 runs with a possibly shorter
last one) and the two weight-gradient kernels (`stages_per_wg` lowered until it divides an image's stages, `nsplit` slabs).  Every
case below first asserts, through tests/bf16_conv_plan.py (tied to the library's workspace queries by tests/test_bf16_conv_plan.py,
and once more here), the plan each of its passes reaches, then compares with fp64.  Function names are conv_bf16.hip's.

  variant                                                                              selected in                              case id(s)
  -----------------------------------------------------------------------------------  ---------------------------------------- ----------------------------
  S1 KT128 P256, 3 tiles per image (W 32)                                              tiles_per_img, data_geometry ptiles      k3_c64_24x32_k160_b3
  S1 KT128 P256, 3 / 5 tiles per image at W 64 / 128                                   tiles_per_img, data_geometry ptiles      k3_c64_12x64_k128_b2, k3_c32_10x128_k80_b1
  S1 KT128 P256 at W 256: one row per tile, raw1, 6 tiles per image                    data_geometry rows, raw1                 k3_c32_6x256_k144_b2
  S1 KT64 P512 at W 16, 3 tiles per image                                              data_geometry                            k3_c48_96x16_k32_b2
  S1 KT64 P512 at W 32, 3 tiles per image                                              data_geometry                            k3T_c32_48x32_k64_b1
  S1 KT64, P512 refused by the rows -> P256                                            data_geometry 512 -> 256                 k3_c64_24x32_k160_b3, k3_c64_12x64_k128_b2, k3_c32_10x128_k80_b1, k3_c256_16x16_k64_b1
  S1 KT64 P256, reduction cut in 2 / in 4                                              cb_cut_reduction                         k3_c64_24x32_k160_b3, k3_c256_16x16_k64_b1
  S1 KT64 P512, cut in 3 uneven (5 + 5 + 3 blocks)                                     cb_cut_reduction                         k3T_c208_32x16_k48_b1
  S1 KT64 P512 raw1 (W 256), cut in 2 uneven (5 + 4 blocks)                            cb_cut_reduction, data_geometry raw1     k3_c32_6x256_k144_b2
  F2C KT64 P512 raw1 at nw 16                                                          data_geometry raw1                       s2_64_32_32x16_b2
  F2C KT64 P512 raw1 at nw 32, 3 tiles per image                                       data_geometry raw1                       s2_48_32_48x32_b1
  F2C KT64 P512 raw1 at nw 64, 3 tiles per image                                       data_geometry raw1                       s2_16_16_24x64_b2
  F2C KT64 P512 raw1 at nw 128 (LDS 156 672 B)                                         data_geometry raw1                       s2_48_16_4x128_b1, s2_32_80_4x128_b1
  F2C KT128 P256 raw1 at nw 128 (LDS 139 776 B), 3 tiles per image                     data_geometry raw1                       s2_128_64_6x128_b1
  F2C cut in 2 uneven, a run = bps x nsub stages (10 + 8)                              cb_cut_reduction                         s2_128_144_16x16_b1
  F2C KT64 cut in 3 uneven                                                             cb_cut_reduction                         s2_64_208_16x16_b1
  F2C 3 tiles per image (KT128)                                                        tiles_per_img, data_geometry ptiles      s2_96_48_24x32_b2
  C2F KT64 P512 at nw 128                                                              data_geometry                            s2_48_16_4x128_b1
  C2F KT128 P256 at nw 128                                                             data_geometry                            s2_32_80_4x128_b1
  C2F KT64 P512 raw1 at nw 256                                                         data_geometry raw1                       s2_16_16_2x256_b1
  C2F KT64 P512 raw1 at nw 256 over 3 stages, 2 tiles per image                        data_geometry, the raw1 stage loop       s2_48_16_4x256_b2
  C2F KT64 P256 (rows) cut in 2, 3 tiles per image                                     cb_cut_reduction                         s2_128_64_6x128_b1
  C2F KT64 cut in 3 uneven                                                             cb_cut_reduction                         s2_208_64_16x16_b1
  C2F 3 tiles per image, both row phases                                               tiles_per_img, data_geometry ptiles      s2_96_48_24x32_b2, s2_48_32_48x32_b1
  k3 weight gradient: groups 6 / 10 / 12 (not a power of two)                          wrw_geometry                             k3_c64_24x32_k160_b3, k3_c32_10x128_k80_b1, k3_c48_96x16_k32_b2
  k3 weight gradient: stages_per_wg lowered by the loop (4 -> 3), 1 < spw < groups     cb_cut_runs                              k3w_ka512_cb256_48x16_b9
  k3 weight gradient: spw = groups, ONE slab                                           cb_cut_runs                              k3w_ka1024_cb1088_16x16_b1
  k4 s2 weight gradient: groups 12 / 24 (not a power of two)                           wrw_geometry                             s2_96_48_24x32_b2, s2_48_32_48x32_b1
  k4 s2 weight gradient: spw = groups 12, one slab per image                           cb_cut_runs                              s2w_512_512_24x32_b5
  k4 s2 weight gradient: ONE slab                                                      cb_cut_runs                              s2w_512_1056_8x16_b1
  refusals: W 24, C % 16, rows % R, F2C nw 256, wrw W 256, s2 wrw nw 128               data_geometry, wrw_geometry              refuse_* (and the `dw` / `f2c` passes the
                                                                                                                                case tables mark refused)
(The 512-pixel tile is never turned down by its LDS plan on a width the form accepts, only by the rows: test_bf16_conv_plan.py.)

Reference and bounds are those of test_direct_bf16_conv_all_passes / test_direct_bf16_stride2_family (tests/test_gpu_conv.py):
F.conv2d / F.conv_transpose2d / aten.convolution_backward in fp64 on the SAME bf16-rounded operands (weights rounded for forward and
input gradient, not for the weight gradient); fp32 outputs within 1e-5 of the reference's max |value|, bf16 outputs within 2^-8,
weight gradients within 1e-5.  Both output types for every forward / input-gradient pass.  Per case in addition:
  * a second call gives the same bits (the cut's runs and the slabs are added in a fixed order);
  * once more inside a guarded.Arena (NaN-filled workspace of exactly the queried size, every operand and result between guard
    bands): bit-equal to the unguarded run, guard bands intact;
  * with B >= 2 and more than one tile per image: image by image against a batch-of-one call — bit for bit where the mirror gives
    both calls the same cut, within the bounds otherwise.  A halo row taken from the neighbouring image shows here.
Measured worst errors (MI355X) are in DESIGN.md §5.9, "Launch variants and what checks them".
"""
import pytest
import torch
import torch.nn.functional as F

import bf16_conv_plan as P
from guarded import Arena
from test_gpu_conv import _f64, _relerr

pytestmark = pytest.mark.gpu

IPSR_ERR_UNSUPPORTED = -2
F32, BF16 = torch.float32, torch.bfloat16
TOL32, TOL16, TOLW = 1e-5, 2.0 ** -8, 1e-5


def _bits(t):
    return t.contiguous().view({4: torch.int32, 2: torch.int16}[t.element_size()])


def _same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(_bits(a), _bits(b))


def _err(a, ref, scale_of=None):
    """max |a - ref| over the max |value| of the reference (`scale_of`: the whole batch's reference when `ref` is one image of it)."""
    return float((a.double() - ref).abs().max() / (ref if scale_of is None else scale_of).abs().max())


def _brief(p):
    """The fields of a plan worth a line in the log."""
    if p is None:
        return None
    names = ("groups", "spw", "lowered", "nsplit") if "RS" in p else ("mode", "kt", "ptile", "tiles_per_img", "raw1", "lds", "nsplit", "bps", "last_bps")
    return {f: p[f] for f in names}


def _check(cid, errs):
    """Print every figure, then assert: keys ending in 32 -> 1e-5, in 16 -> 2^-8, dw -> 1e-5."""
    print("%s: %s" % (cid, ", ".join("%s %.2e" % kv for kv in sorted(errs.items()))))
    bad = {k: v for k, v in errs.items() if not v <= (TOL16 if k.split("@")[0].endswith("16") else (TOLW if k.startswith("dw") else TOL32))}
    assert not bad, (cid, bad)


def _guarded(monkeypatch, tensors, fn, normal):
    """Run fn(*guarded copies) inside an Arena; results bit-equal to `normal`, guard bands intact, inputs unchanged."""
    arena = Arena(ws_fill="nan")
    placed = [arena.guarded_copy(t, "in%d" % i) for i, t in enumerate(tensors)]
    with arena.installed(monkeypatch):
        got = fn(*placed)
    torch.cuda.synchronize()
    arena.check_guards()
    for g, t in zip(placed, tensors):
        assert _same(g, t), "an input was modified"
    assert set(got) == set(normal)
    for k in got:
        assert _same(got[k], normal[k]), "%s differs between the guarded and the unguarded run" % k
    assert arena.guard_bytes() > 0 and arena.workspaces


# ---- k3 s1 p1 -------------------------------------------------------------------------------------------------------------------------
def _k3_inputs(tr, Cin, H, W, Cout, B, seed=29):
    g = torch.Generator(device="cuda").manual_seed(seed)
    x = torch.randn(B, Cin, H, W, device="cuda", generator=g).to(BF16)
    dy = torch.randn(B, Cout, H, W, device="cuda", generator=g).to(BF16)
    w = torch.randn((Cin, Cout, 3, 3) if tr else (Cout, Cin, 3, 3), device="cuda", generator=g) * 0.1
    return x, dy, w


def _k3_run(ops, tr, dims, plans, x, dy, w):
    Cin, H, W, Cout = dims
    B = x.shape[0]
    fop, bop = (ops.CONVT_FWD, ops.CONVT_BWD_DATA) if tr else (ops.CONV_FWD, ops.CONV_BWD_DATA)
    res = {}
    if plans.get("fwd") is not None:
        res["y32"] = ops.conv3x3_bf16(fop, x, w, (B, Cin, H, W), Cout, out_dtype=F32)
        res["y16"] = ops.conv3x3_bf16(fop, x, w, (B, Cin, H, W), Cout)
    if plans.get("dx") is not None:
        res["dx32"] = ops.conv3x3_bf16(bop, dy, w, (B, Cin, H, W), Cout, out_dtype=F32)
        res["dx16"] = ops.conv3x3_bf16(bop, dy, w, (B, Cin, H, W), Cout)
    if plans.get("dw") is not None:
        res["dw"] = ops.conv3x3_bf16_wrw(tr, x, dy, Cout)
    return res


def _k3_library_agrees(ops, tr, B, Cin, H, W, Cout, plans):
    """The library's own queries give the byte counts the mirror's plans imply (and 0 where it refuses)."""
    from deepinpainting_amd import _lib
    L = _lib.lib()
    fop, bop = (ops.CONVT_FWD, ops.CONVT_BWD_DATA) if tr else (ops.CONV_FWD, ops.CONV_BWD_DATA)
    if "fwd" in plans:
        assert L.ipsr_conv3x3_bf16_workspace_bytes(fop, B, Cin, H, W, Cout) == P.data_ws_bytes(plans["fwd"])
        assert L.ipsr_conv3x3_bf16_workspace_bytes(bop, B, Cin, H, W, Cout) == P.data_ws_bytes(plans["dx"])
    assert L.ipsr_conv3x3_bf16_wrw_workspace_bytes(int(tr), B, Cin, H, W, Cout) == P.wb_ws_bytes(plans["dw"])


@pytest.mark.parametrize("cid", list(P.K3_CASES))
def test_k3_variants(cid, monkeypatch):
    from deepinpainting_amd import ops
    (tr, Cin, H, W, Cout, B), _ = P.K3_CASES[cid]
    plans = P.check_case(cid)
    _k3_library_agrees(ops, tr, B, Cin, H, W, Cout, plans)
    print(cid, {k: _brief(p) for k, p in plans.items()})
    x, dy, w = _k3_inputs(tr, Cin, H, W, Cout, B)
    f = (lambda a, ww: F.conv_transpose2d(a, ww, None, 1, 1)) if tr else (lambda a, ww: F.conv2d(a, ww, None, 1, 1))
    y64, dx64, _ = _f64(f, x, w.to(BF16), dy)                  # the kernel rounds the weights to bf16
    _, _, dw64 = _f64(f, x, w, dy)                             # the weight gradient does not read the weights
    run = lambda a, b, c: _k3_run(ops, tr, (Cin, H, W, Cout), plans, a, b, c)
    res = run(x, dy, w)
    torch.cuda.synchronize()
    assert res["y16"].dtype == BF16 and res["dx16"].dtype == BF16 and res["y32"].dtype == F32
    errs = dict(y32=_relerr(res["y32"], y64), y16=_relerr(res["y16"], y64), dx32=_relerr(res["dx32"], dx64), dx16=_relerr(res["dx16"], dx64))
    if plans["dw"] is None:
        assert not ops.conv3x3_bf16_wrw_supported(tr, B, Cin, H, W, Cout)
        with pytest.raises(NotImplementedError):
            ops.conv3x3_bf16_wrw(tr, x, dy, Cout)
    else:
        assert res["dw"].dtype == F32 and res["dw"].shape == w.shape
        errs["dw"] = _relerr(res["dw"], dw64)
    # image by image against a batch of one
    fop, bop = (ops.CONVT_FWD, ops.CONVT_BWD_DATA) if tr else (ops.CONV_FWD, ops.CONV_BWD_DATA)
    if B >= 2:
        for name, op, src, ref, plan in (("y", fop, x, y64, plans["fwd"]), ("dx", bop, dy, dx64, plans["dx"])):
            if plan["tiles_per_img"] < 2:
                continue
            one = P.k3_plan(op, 1, Cin, H, W, Cout)
            for b in range(B):
                o32 = ops.conv3x3_bf16(op, src[b:b + 1].contiguous(), w, (1, Cin, H, W), Cout, out_dtype=F32)
                o16 = ops.conv3x3_bf16(op, src[b:b + 1].contiguous(), w, (1, Cin, H, W), Cout)
                errs["%s32@%d" % (name, b)] = _err(o32, ref[b:b + 1], ref)
                errs["%s16@%d" % (name, b)] = _err(o16, ref[b:b + 1], ref)
                if P.same_cut(plan, one):
                    assert _same(o32, res[name + "32"][b:b + 1]) and _same(o16, res[name + "16"][b:b + 1]), \
                        "%s: image %d of the batch differs from the same image alone (%s)" % (cid, b, name)
    _check(cid, errs)
    again = run(x, dy, w)
    torch.cuda.synchronize()
    for k in res:
        assert _same(again[k], res[k]), "%s: %s differs between two calls" % (cid, k)
    _guarded(monkeypatch, (x, dy, w), run, res)


@pytest.mark.parametrize("cid", list(P.K3_WRW_CASES))
def test_k3_weight_gradient_variants(cid, monkeypatch):
    from deepinpainting_amd import ops
    (tr, Cin, H, W, Cout, B), _ = P.K3_WRW_CASES[cid]
    plans = P.check_case(cid)
    _k3_library_agrees(ops, tr, B, Cin, H, W, Cout, plans)
    x, dy, w = _k3_inputs(tr, Cin, H, W, Cout, B)
    dw64 = torch.ops.aten.convolution_backward(dy.double(), x.double(), w.double(), None, [1, 1], [1, 1], [1, 1], tr, [0, 0], 1, [False, True, False])[1]
    run = lambda a, b: dict(dw=ops.conv3x3_bf16_wrw(tr, a, b, Cout))
    res = run(x, dy)
    torch.cuda.synchronize()
    assert res["dw"].dtype == F32 and res["dw"].shape == w.shape
    _check(cid, dict(dw=_relerr(res["dw"], dw64)))
    assert _same(run(x, dy)["dw"], res["dw"]), "%s: dw differs between two calls" % cid
    _guarded(monkeypatch, (x, dy), run, res)


# ---- k4 s2 p1 -------------------------------------------------------------------------------------------------------------------------
def _s2_inputs(Kc, Cf, nh, nw, B, seed=31):
    g = torch.Generator(device="cuda").manual_seed(seed)
    fine = torch.randn(B, Cf, 2 * nh, 2 * nw, device="cuda", generator=g).to(BF16)
    coarse = torch.randn(B, Kc, nh, nw, device="cuda", generator=g).to(BF16)
    w = torch.randn(Kc, Cf, 4, 4, device="cuda", generator=g) * 0.1
    return fine, coarse, w


def _s2_run(ops, dims, plans, fine, coarse, w):
    Kc, Cf, nh, nw = dims
    B = fine.shape[0]
    res = {}
    if plans.get("f2c") is not None:
        res["c32"] = ops.conv4x4s2_bf16(ops.S2_FINE_TO_COARSE, fine, w, B, Kc, Cf, nh, nw, out_dtype=F32)
        res["c16"] = ops.conv4x4s2_bf16(ops.S2_FINE_TO_COARSE, fine, w, B, Kc, Cf, nh, nw)
    if plans.get("c2f") is not None:
        res["f32"] = ops.conv4x4s2_bf16(ops.S2_COARSE_TO_FINE, coarse, w, B, Kc, Cf, nh, nw, out_dtype=F32)
        res["f16"] = ops.conv4x4s2_bf16(ops.S2_COARSE_TO_FINE, coarse, w, B, Kc, Cf, nh, nw)
    if plans.get("dw") is not None:
        res["dw"] = ops.conv4x4s2_bf16_wrw(fine, coarse, B, Kc, Cf, nh, nw)
    return res


def _s2_library_agrees(B, Kc, Cf, nh, nw, plans):
    from deepinpainting_amd import _lib
    L = _lib.lib()
    if "f2c" in plans:
        assert L.ipsr_conv4x4s2_bf16_workspace_bytes(0, B, Kc, Cf, nh, nw) == P.data_ws_bytes(plans["f2c"])
        assert L.ipsr_conv4x4s2_bf16_workspace_bytes(1, B, Kc, Cf, nh, nw) == P.data_ws_bytes(plans["c2f"])
    assert L.ipsr_conv4x4s2_bf16_wrw_workspace_bytes(B, Kc, Cf, nh, nw) == P.w2_ws_bytes(plans["dw"])


def _s2_dw64(fine, coarse, w):
    return torch.ops.aten.convolution_backward(coarse.double(), fine.double(), w.double(), None, [2, 2], [1, 1], [1, 1], False, [0, 0], 1,
                                               [False, True, False])[1]


@pytest.mark.parametrize("cid", list(P.S2_CASES))
def test_s2_variants(cid, monkeypatch):
    from deepinpainting_amd import _lib, ops
    (Kc, Cf, nh, nw, B), _ = P.S2_CASES[cid]
    plans = P.check_case(cid)
    _s2_library_agrees(B, Kc, Cf, nh, nw, plans)
    print(cid, {k: _brief(p) for k, p in plans.items()})
    fine, coarse, w = _s2_inputs(Kc, Cf, nh, nw, B)
    wd = w.to(BF16).double()
    c64 = F.conv2d(fine.double(), wd, None, 2, 1)
    f64 = F.conv_transpose2d(coarse.double(), wd, None, 2, 1)
    run = lambda a, b, c: _s2_run(ops, (Kc, Cf, nh, nw), plans, a, b, c)
    res = run(fine, coarse, w)
    torch.cuda.synchronize()
    errs = {}
    for name, mode, ref in (("c", ops.S2_FINE_TO_COARSE, c64), ("f", ops.S2_COARSE_TO_FINE, f64)):
        plan = plans["f2c" if name == "c" else "c2f"]
        src = fine if name == "c" else coarse
        if plan is None:
            assert not ops.conv4x4s2_bf16_supported(mode, B, Kc, Cf, nh, nw)
            with pytest.raises(NotImplementedError):
                ops.conv4x4s2_bf16(mode, src, w, B, Kc, Cf, nh, nw)
            assert "does not fit the LDS plan" in _lib.lib().ipsr_last_error().decode("utf-8", "replace")
            continue
        assert res[name + "16"].dtype == BF16 and res[name + "32"].dtype == F32 and res[name + "32"].shape == ref.shape
        errs[name + "32"], errs[name + "16"] = _relerr(res[name + "32"], ref), _relerr(res[name + "16"], ref)
        if B >= 2 and plan["tiles_per_img"] >= 2:
            one = P.s2_plan(mode, 1, Kc, Cf, nh, nw)
            for b in range(B):
                o32 = ops.conv4x4s2_bf16(mode, src[b:b + 1].contiguous(), w, 1, Kc, Cf, nh, nw, out_dtype=F32)
                o16 = ops.conv4x4s2_bf16(mode, src[b:b + 1].contiguous(), w, 1, Kc, Cf, nh, nw)
                errs["%s32@%d" % (name, b)] = _err(o32, ref[b:b + 1], ref)
                errs["%s16@%d" % (name, b)] = _err(o16, ref[b:b + 1], ref)
                if P.same_cut(plan, one):
                    assert _same(o32, res[name + "32"][b:b + 1]) and _same(o16, res[name + "16"][b:b + 1]), \
                        "%s: image %d of the batch differs from the same image alone (%s)" % (cid, b, name)
    if plans["dw"] is None:
        assert not ops.conv4x4s2_bf16_wrw_supported(B, Kc, Cf, nh, nw)
        with pytest.raises(NotImplementedError):
            ops.conv4x4s2_bf16_wrw(fine, coarse, B, Kc, Cf, nh, nw)
    else:
        assert res["dw"].dtype == F32 and res["dw"].shape == w.shape
        errs["dw"] = _relerr(res["dw"], _s2_dw64(fine, coarse, w))
    _check(cid, errs)
    again = run(fine, coarse, w)
    torch.cuda.synchronize()
    for k in res:
        assert _same(again[k], res[k]), "%s: %s differs between two calls" % (cid, k)
    _guarded(monkeypatch, (fine, coarse, w), run, res)


@pytest.mark.parametrize("cid", list(P.S2_WRW_CASES))
def test_s2_weight_gradient_variants(cid, monkeypatch):
    from deepinpainting_amd import ops
    (Kc, Cf, nh, nw, B), _ = P.S2_WRW_CASES[cid]
    plans = P.check_case(cid)
    _s2_library_agrees(B, Kc, Cf, nh, nw, plans)
    fine, coarse, w = _s2_inputs(Kc, Cf, nh, nw, B)
    run = lambda a, b: dict(dw=ops.conv4x4s2_bf16_wrw(a, b, B, Kc, Cf, nh, nw))
    res = run(fine, coarse)
    torch.cuda.synchronize()
    assert res["dw"].dtype == F32 and res["dw"].shape == w.shape
    _check(cid, dict(dw=_relerr(res["dw"], _s2_dw64(fine, coarse, w))))
    assert _same(run(fine, coarse)["dw"], res["dw"]), "%s: dw differs between two calls" % cid
    _guarded(monkeypatch, (fine, coarse), run, res)


# ---- refusals ----------------------------------------------------------------------------------------------------------------------------
# id, entry, shape, message fragment.  k3: (op, B, Cin, H, W, Cout); s2: (mode, B, Kc, Cf, nh, nw); k3w: (tr, B, Cin, H, W, Cout); s2w: (B, Kc, Cf, nh, nw)
REFUSALS = [
    ("refuse_k3_w24", "k3", (0, 1, 16, 12, 24, 16), "grid width 24"),
    ("refuse_k3_c24", "k3", (0, 1, 24, 16, 16, 16), "24 reduction channels are not a multiple of 16"),
    ("refuse_k3_dx_c24", "k3", (1, 1, 16, 16, 16, 24), "24 reduction channels are not a multiple of 16"),
    ("refuse_k3_rows", "k3", (0, 2, 16, 12, 32, 128), "12 rows are not a multiple of the 8 rows of a tile"),
    ("refuse_s2_f2c_nw256", "s2", (0, 1, 16, 16, 2, 256), "does not fit the LDS plan"),
    ("refuse_s2_c2f_c24", "s2", (1, 1, 24, 16, 16, 16), "24 reduction channels are not a multiple of 16"),
    ("refuse_s2_rows", "s2", (1, 1, 16, 128, 12, 32), "12 rows are not a multiple of the 8 rows of a tile"),
    ("refuse_k3w_w256", "k3w", (0, 1, 16, 4, 256, 16), "image width 256"),
    ("refuse_k3w_rows", "k3w", (1, 2, 16, 12, 16, 32), "12 rows are not a multiple of 8"),
    ("refuse_s2w_nw128", "s2w", (1, 16, 16, 4, 128), "coarse width 128"),
    ("refuse_s2w_rows", "s2w", (2, 16, 32, 6, 16), "6 coarse rows are not a multiple of 4"),
]


def _nan_fill(t):
    _bits(t).fill_(0x7FC00DAD if t.element_size() == 4 else 0x7FC1)
    return t


@pytest.mark.parametrize("entry,shape,msg", [r[1:] for r in REFUSALS], ids=[r[0] for r in REFUSALS])
def test_refusals_write_nothing(entry, shape, msg):
    """Through `ops`: NotImplementedError.  At the C ABI: IPSR_ERR_UNSUPPORTED, the message names the limit, and the NaN-pre-filled
    output is bitwise unchanged after a synchronise (the geometry is checked before the first launch)."""
    from deepinpainting_amd import _lib, ops
    L = _lib.lib()
    ws = torch.empty(1 << 20, dtype=torch.uint8, device="cuda")
    z = lambda *s, dtype=BF16: torch.zeros(*s, device="cuda", dtype=dtype)
    for out_bf16 in ((0, 1) if entry in ("k3", "s2") else (0,)):
        odt = BF16 if out_bf16 else F32
        if entry == "k3":
            op, B, Cin, H, W, Cout = shape
            fwd = op in (0, 2)
            assert P.k3_plan(*shape) is None and msg in P.k3_plan(*shape, why=True)[1]
            src = z(B, Cin if fwd else Cout, H, W)
            w = z(*((Cout, Cin, 3, 3) if op < 2 else (Cin, Cout, 3, 3)), dtype=F32)
            out = _nan_fill(torch.empty(B, Cout if fwd else Cin, H, W, device="cuda", dtype=odt))
            assert not ops.conv3x3_bf16_supported(*shape)
            with pytest.raises(NotImplementedError):
                ops.conv3x3_bf16(op, src, w, (B, Cin, H, W), Cout, out_dtype=odt)
            call = lambda: L.ipsr_conv3x3_bf16(op, src.data_ptr(), w.data_ptr(), out.data_ptr(), B, Cin, H, W, Cout, out_bf16, ws.data_ptr(), ws.numel(), ops._stream())
        elif entry == "s2":
            mode, B, Kc, Cf, nh, nw = shape
            assert P.s2_plan(*shape) is None and msg in P.s2_plan(*shape, why=True)[1]
            src = z(B, Cf, 2 * nh, 2 * nw) if mode == 0 else z(B, Kc, nh, nw)
            w = z(Kc, Cf, 4, 4, dtype=F32)
            out = _nan_fill(torch.empty((B, Kc, nh, nw) if mode == 0 else (B, Cf, 2 * nh, 2 * nw), device="cuda", dtype=odt))
            assert not ops.conv4x4s2_bf16_supported(*shape)
            with pytest.raises(NotImplementedError):
                ops.conv4x4s2_bf16(mode, src, w, B, Kc, Cf, nh, nw, out_dtype=odt)
            call = lambda: L.ipsr_conv4x4s2_bf16(mode, src.data_ptr(), w.data_ptr(), out.data_ptr(), B, Kc, Cf, nh, nw, out_bf16, ws.data_ptr(), ws.numel(), ops._stream())
        elif entry == "k3w":
            tr, B, Cin, H, W, Cout = shape
            assert P.k3_wrw_plan(*shape) is None and msg in P.k3_wrw_plan(*shape, why=True)[1]
            x, dy = z(B, Cin, H, W), z(B, Cout, H, W)
            out = _nan_fill(torch.empty((Cin, Cout, 3, 3) if tr else (Cout, Cin, 3, 3), device="cuda"))
            assert not ops.conv3x3_bf16_wrw_supported(*shape)
            with pytest.raises(NotImplementedError):
                ops.conv3x3_bf16_wrw(bool(tr), x, dy, Cout)
            call = lambda: L.ipsr_conv3x3_bf16_wrw(tr, x.data_ptr(), dy.data_ptr(), out.data_ptr(), B, Cin, H, W, Cout, ws.data_ptr(), ws.numel(), ops._stream())
        else:
            B, Kc, Cf, nh, nw = shape
            assert P.s2_wrw_plan(*shape) is None and msg in P.s2_wrw_plan(*shape, why=True)[1]
            fine, coarse = z(B, Cf, 2 * nh, 2 * nw), z(B, Kc, nh, nw)
            out = _nan_fill(torch.empty(Kc, Cf, 4, 4, device="cuda"))
            assert not ops.conv4x4s2_bf16_wrw_supported(*shape)
            with pytest.raises(NotImplementedError):
                ops.conv4x4s2_bf16_wrw(fine, coarse, B, Kc, Cf, nh, nw)
            call = lambda: L.ipsr_conv4x4s2_bf16_wrw(fine.data_ptr(), coarse.data_ptr(), out.data_ptr(), B, Kc, Cf, nh, nw, ws.data_ptr(), ws.numel(), ops._stream())
        keep = out.clone()
        torch.cuda.synchronize()
        rc = call()
        text = L.ipsr_last_error().decode("utf-8", "replace")
        torch.cuda.synchronize()
        assert rc == IPSR_ERR_UNSUPPORTED, (rc, text)
        assert msg in text, text
        assert _same(out, keep), "the output was written by a refused call"
