"""Guard bands and poisoned scratch around every kernel-launching C entry (tests/guarded.py).

Each case runs twice through the `ops` wrappers: once normally, once with every input, output, cache and workspace placed between
4 KiB guard bands (ops._empty / ops._zeros / ops._workspace replaced), outputs starting NaN-filled and each workspace exactly the
size its query reported.  Then:
  1. every guard band is bit-identical to its fill, and every input is bit-identical to what was passed (in-place operands excepted);
  2. the guarded results equal the normal ones bit for bit (fixed summation orders, no float atomics);
  3. results that are finite in the normal run contain no NaN: every element was written;
  4. results do not depend on workspace contents: workspaces audited to hold floats alone start NaN-filled; the ones that also
     hold integers start zero-filled and are compared with the normal run, which meets whatever the previous case left behind.

Workspace audit (what the carve code puts in each scratch buffer):
  floats only  wino_launch_head (winograd.hip), launch_smallmap (smallmap.hip) (transformed operands, products, split partials);
               conv_bf16.hip data_ws_bytes / cb_partial_bytes (zero page, packed bf16 weights, fp32 split partials); conv_gemm.hip:379-387 (packed operands,
               split-K partials); thin_conv.hip (fp32 partials of the weight gradients); innercos.hip innercos_ws_bytes (fp64 block partials)
  integers     api.hip:89 (layer forward / backward: arg-max partial indices, rank flags, the sparse index); api.hip:209 (feat_mask
               bit masks); corr_argmax partial indices
"""
import os
import re

import pytest
import torch

from guarded import NAN16, NAN32, Arena

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32, BF16 = torch.float32, torch.bfloat16


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def rn(*shape, seed, dtype=F32, scale=1.0, pos=False):
    t = torch.randn(*shape, generator=_gen(seed)) * scale
    return (t.abs() if pos else t).to(dtype).cuda()


def nan_like(shape, dtype):
    t = torch.empty(shape, dtype=dtype)
    t.view(torch.int32 if dtype == F32 else torch.int16).fill_(NAN32 if dtype == F32 else NAN16)
    return t.cuda()


def untouched(t, lo, hi):
    """Channels outside [lo, hi) of a wide [B,Ctot,H,W] tensor still hold the NaN guard pattern, bit for bit."""
    torch.cuda.synchronize()
    b = t.view(torch.int32 if t.dtype == F32 else torch.int16)
    word = NAN32 if t.dtype == F32 else NAN16
    assert bool((b[:, :lo] == word).all()) and bool((b[:, hi:] == word).all()), "a slice writer touched channels outside [%d, %d)" % (lo, hi)


def finite(*ts):
    torch.cuda.synchronize()
    for t in ts:
        assert bool(torch.isfinite(t.float()).all()), "a result depends on channels outside its slice"


def _mask(h, w, seed, p=0.4):
    return (torch.rand(h, w, generator=_gen(seed)) < p).to(torch.uint8).cuda()


# ---------------------------------------------------------------------------------------------------------------- the cases
# (id, C entries reached, workspace fill, in-place operands, fn(mk) -> {name: tensor}).  mk(name, tensor) places an input.
CASES = []


def case(cid, entries, ws="nan", inplace=()):
    def deco(fn):
        CASES.append((cid, tuple(entries), ws, tuple(inplace), fn))
        return fn
    return deco


def _layer_inputs(mk, B, C, h, seed, p=0.4):
    from deepinpainting_amd import ops
    x = mk("x", rn(B, C, h, h, seed=seed, pos=True))
    ref = mk("ref", rn(B, C, h, h, seed=seed + 1, pos=True))
    _, mpi, cnt = ops.index_prep(mk("feat", _mask(h, h, seed + 2, p)), 1, 1, 1)
    M = int(cnt.item())
    return x, ref, mpi, M


for _B, _C, _h in ((2, 64, 16), (3, 20, 8), (1, 512, 32)):
    @case("layer_fwd_bwd_b%d_c%d_%d" % (_B, _C, _h), ["ipsr_index_prep", "ipsr_forward", "ipsr_backward"], ws="zero")
    def _(mk, B=_B, C=_C, h=_h):
        from deepinpainting_amd import ops
        x, ref, mpi, M = _layer_inputs(mk, B, C, h, B + C + h)
        f = ops.forward(x, ref, mk("mpi", mpi[:M].contiguous()), want_attn=True)
        gin = ops.backward(mk("g", rn(B, C, h, h, seed=5)), f.bwd_index, 0.75, M)
        return dict(out=f.out, ind=f.ind, vmax=f.vmax, attn=f.attn_rows, bidx=f.bwd_index, gin=gin)


@case("layer_masks_b5", ["ipsr_forward_masks", "ipsr_backward"], ws="zero")
def _(mk):
    from deepinpainting_amd import ops
    B, C, h = 5, 64, 16
    x, ref = mk("x", rn(B, C, h, h, seed=1, pos=True)), mk("ref", rn(B, C, h, h, seed=2, pos=True))
    rows = [ops.index_prep(mk("feat%d" % i, _mask(h, h, 10 + i, p)), 1, 1, 1) for i, p in enumerate((0.3, 0.1, 0.55, 0.0, 1.0))]
    mpi = mk("mpi", torch.stack([r[1] for r in rows]))
    counts = mk("counts", torch.cat([r[2] for r in rows]))
    f = ops.forward(x, ref, mpi, want_attn=True, counts=counts)
    gin = ops.backward(mk("g", rn(B, C, h, h, seed=3)), f.bwd_index, 0.75, h * h)
    return dict(out=f.out, ind=f.ind, vmax=f.vmax, attn=f.attn_rows, bidx=f.bwd_index, gin=gin)


@case("layer_bf16corr_b2_c512_32", ["ipsr_forward_bf16corr"], ws="zero")
def _(mk):
    from deepinpainting_amd import ops
    x, ref, mpi, M = _layer_inputs(mk, 2, 512, 32, 7)
    f = ops.forward(x, ref, mk("mpi", mpi[:M].contiguous()), corr="bf16")
    return dict(out=f.out, ind=f.ind, vmax=f.vmax, bidx=f.bwd_index)


@case("layer_patch3_b2_c64_16", ["ipsr_forward", "ipsr_backward_patch"], ws="zero")
def _(mk):
    from deepinpainting_amd import ops
    B, C, h = 2, 64, 16
    x, ref = mk("x", rn(B, C, h, h, seed=1, pos=True)), mk("ref", rn(B, C, h, h, seed=2))
    _, mpi, cnt = ops.index_prep(mk("feat", _mask(h, h, 3)), 3, 1, 1)
    M = int(cnt.item())
    f = ops.forward(x, ref, mk("mpi", mpi[:M].contiguous()), patch=3, want_attn=True)
    gin = ops.backward(mk("g", rn(B, C, h, h, seed=4)), f.bwd_index, 0.5, M, patch=3)
    return dict(out=f.out, ind=f.ind, vmax=f.vmax, attn=f.attn_rows, bidx=f.bwd_index, gin=gin)


for _H, _W in ((256, 256), (100, 140)):
    @case("feat_mask_%dx%d" % (_H, _W), ["ipsr_feat_mask", "ipsr_index_prep"], ws="zero")
    def _(mk, H=_H, W=_W):
        from deepinpainting_amd import ops
        m = torch.zeros(H, W, dtype=torch.uint8)
        m[H // 4:3 * H // 4, W // 3:2 * W // 3] = 1
        feat = ops.feat_mask(mk("mask", m.cuda()), 3, 5 / 16.0)
        flag, mpi, cnt = ops.index_prep(feat, 3, 1, 1) if min(feat.shape) >= 3 else ops.index_prep(feat, 1, 1, 1)
        return dict(feat=feat, flag=flag, mpi=mpi, cnt=cnt)


for _B, _C, _N in ((3, 8, 100), (2, 512, 1024), (1, 100, 384)):
    @case("normalize_corr_%d_%d_%d" % (_B, _C, _N), ["ipsr_patch_normalize", "ipsr_corr_argmax"], ws="zero")
    def _(mk, B=_B, C=_C, N=_N):
        from deepinpainting_amd import ops
        xn, inv = ops.patch_normalize(mk("x", rn(B, C, N, seed=N, pos=True)))
        ind, vmax, S = ops.corr_argmax(xn, mk("ref", rn(B, C, N, seed=C, pos=True)), want_S=True)
        return dict(xn=xn, inv=inv, ind=ind, vmax=vmax, S=S)


for _B, _C, _N in ((1, 64, 128), (2, 512, 1024)):
    @case("corr_bf16_%d_%d_%d" % (_B, _C, _N), ["ipsr_corr_argmax_bf16"], ws="zero")
    def _(mk, B=_B, C=_C, N=_N):
        from deepinpainting_amd import ops
        xn, _ = ops.patch_normalize(mk("x", rn(B, C, N, seed=N, pos=True)))
        ind, vmax, _ = ops.corr_argmax(xn, mk("ref", rn(B, C, N, seed=C, pos=True)), corr="bf16")
        return dict(ind=ind, vmax=vmax)


for _B, _C in ((2, 8), (1, 512)):
    @case("innercos_%d_%d" % (_B, _C), ["innercos_loss", "innercos_loss_fused", "innercos_loss_backward"])
    def _(mk, B=_B, C=_C):
        from deepinpainting_amd import ops
        h = 8 if C == 8 else 32
        x = mk("x", rn(B, C + 3, h, h, seed=1))
        m = mk("mask", _mask(h, h, 2).float().reshape(-1))
        t = mk("target", rn(B, C, h, h, seed=3))
        return dict(loss=ops.innercos_loss(x, C, m, t, 0.5), fused=ops.innercos_loss(x, C, m, t, 0.5, one_launch=True),
                    gx=ops.innercos_loss_backward(x, C, m, t, 0.5, mk("gl", torch.ones(1).cuda())))


# ---- glue kernels (pointwise.hip / instnorm.hip): a plane that is a multiple of 4 (vector path), a ragged one, a step shape
GLUE_SHAPES = [(2, 24, 10, 10), (3, 5, 7, 9), (8, 64, 32, 32)]
for _dt in (F32, BF16):
    for _s in GLUE_SHAPES:
        _id = "%s_%s" % ("bf16" if _dt == BF16 else "fp32", "x".join(map(str, _s)))

        @case("bias_act_" + _id, ["ipsr_bias_act", "ipsr_bias_act_skip", "ipsr_bias_act_backward", "ipsr_bias_act_backward_skip"],
              inplace=("x", "x2", "wide"))
        def _(mk, s=_s, dt=_dt):
            from deepinpainting_amd import ops
            B, C, H, W = s
            bias = mk("bias", rn(C, seed=1))
            x = ops.bias_act_(mk("x", rn(*s, seed=2, dtype=dt)), bias, "leaky", 0.2)
            # the skip destination: channels [3, 3 + C) of a wider tensor whose other channels hold NaN and must keep it
            wide = mk("wide", nan_like((B, C + 5, H, W), dt))
            x2 = ops.bias_act_(mk("x2", rn(*s, seed=3, dtype=dt)), bias, "relu", relu_into=wide, relu_at=3)
            dx, db = ops.bias_act_backward(mk("dy", rn(*s, seed=4, dtype=dt)), x, "leaky", 0.2, True)
            dyw = rn(B, C + 5, H, W, seed=5, dtype=dt)
            dyw[:, :3] = nan_like((B, 3, H, W), dt)
            dyw[:, 3 + C:] = nan_like((B, 2, H, W), dt)
            dx2, db2 = ops.bias_act_backward(mk("dy2", rn(*s, seed=6, dtype=dt)), x2, "relu", 0.2, True, dy2=mk("dyw", dyw), dy2_at=3)
            untouched(wide, 3, 3 + C)
            finite(dx2, db2)
            return dict(x=x, x2=x2, wide=wide, dx=dx, db=db, dx2=dx2, db2=db2)

        @case("cat_pool_" + _id, ["ipsr_cat_relu_forward", "ipsr_cat_relu_backward", "ipsr_bias_relu_pool2"], inplace=("wide",))
        def _(mk, s=_s, dt=_dt):
            from deepinpainting_amd import ops
            B, C, H, W = s
            y, x = mk("y", rn(*s, seed=1, dtype=dt)), mk("x", rn(B, C + 3, H, W, seed=2, dtype=dt))
            out = ops.cat_relu_forward(y, x)
            dy, dx = ops.cat_relu_backward(mk("g", rn(B, 2 * C + 3, H, W, seed=3, dtype=dt)), out, C)
            _, dx_only = ops.cat_relu_backward(mk("g2", rn(B, 2 * C + 3, H, W, seed=4, dtype=dt)), out, C, skip_half_only=True)
            wide = mk("wide", nan_like((B, 2 * C + 3, H, W), dt))
            wide[:, :C] = 0
            ops.cat_relu_skip_half_(wide, x)
            res = dict(out=out, dy=dy, dx=dx, dx_only=dx_only, wide=wide)
            if H % 2 == 0 and W % 2 == 0:
                res["pool"] = ops.bias_relu_pool2(mk("p", rn(*s, seed=5, dtype=dt)), mk("bias", rn(C, seed=6)))
            return res

        @case("instnorm_" + _id, ["ipsr_instnorm_act_forward", "ipsr_instnorm_act_forward_slice", "ipsr_instnorm_act_backward",
                                  "ipsr_instnorm_act_backward_slice"], inplace=("into", "relu_into"))
        def _(mk, s=_s, dt=_dt):
            from deepinpainting_amd import ops
            B, C, H, W = s
            x = mk("x", rn(*s, seed=1, dtype=dt))
            bias, gamma, beta = mk("bias", rn(C, seed=2)), mk("gamma", rn(C, seed=3)), mk("beta", rn(C, seed=4))
            y, mean, rstd, tk = ops.instnorm_act_forward(x, bias, gamma, beta, 1e-5, "leaky", 0.2, return_tickets=True)
            into, relu_into = mk("into", nan_like((B, C + 4, H, W), dt)), mk("relu_into", nan_like((B, C + 6, H, W), dt))
            y2, mean2, rstd2, tk2 = ops.instnorm_act_forward(x, bias, gamma, beta, 1e-5, "relu", 0.2, into=into, into_at=4,
                                                             relu_into=relu_into, relu_at=1, return_tickets=True)
            dx, dg, db, dbias = ops.instnorm_act_backward(mk("dy", rn(*s, seed=5, dtype=dt)), y, x, bias, gamma, mean, rstd, "leaky", 0.2,
                                                          True, True, tickets=tk)
            # the slice form: dy / y wide with NaN outside the operand channels, a second gradient likewise
            dyw = rn(B, C + 4, H, W, seed=6, dtype=dt)
            dyw[:, :4] = nan_like((B, 4, H, W), dt)
            d2 = rn(B, C + 6, H, W, seed=7, dtype=dt)
            d2[:, :1] = nan_like((B, 1, H, W), dt)
            d2[:, 1 + C:] = nan_like((B, 5, H, W), dt)
            dx2, dg2, db2, dbias2 = ops.instnorm_act_backward(mk("dyw", dyw), y2, x, bias, gamma, mean2, rstd2, "relu", 0.2, True, True,
                                                              at=4, dy2=mk("d2", d2), dy2_at=1, tickets=tk2)
            untouched(into, 4, 4 + C)
            untouched(relu_into, 1, 1 + C)
            finite(dx2, dg2, db2, dbias2)
            return dict(y=y, mean=mean, rstd=rstd, into=into, relu_into=relu_into, mean2=mean2, rstd2=rstd2, dx=dx, dg=dg, db=db,
                        dbias=dbias, dx2=dx2, dg2=dg2, db2=db2, dbias2=dbias2)


# ---- convolutions (fp32 weights throughout)
def _w(shape, seed):
    return rn(*shape, seed=seed, scale=0.1)


for _g in (("conv", 64, 5, 7, 20, 3, 1, 1, 1), ("convT", 16, 7, 9, 24, 4, 2, 1, 1), ("conv", 24, 6, 6, 24, 4, 2, 3, 2),
           ("conv", 512, 2, 2, 512, 4, 2, 1, 1)):
    @case("conv2d_%s_c%d_%dx%d_k%d_s%d" % (_g[0], _g[1], _g[2], _g[3], _g[5], _g[6]), ["ipsr_conv2d"])
    def _(mk, g=_g):
        from deepinpainting_amd import ops
        kind, Cin, H, W, Cout, k, st, pad, dil = g
        tr, B = kind == "convT", 3
        fop, bop = (ops.CONVT_FWD, ops.CONVT_BWD_DATA) if tr else (ops.CONV_FWD, ops.CONV_BWD_DATA)
        w = mk("w", _w((Cin, Cout, k, k) if tr else (Cout, Cin, k, k), 1))
        Ho, Wo = ops.conv_out_dim(fop, H, k, st, pad, dil), ops.conv_out_dim(fop, W, k, st, pad, dil)
        y = ops.conv2d(fop, mk("x", rn(B, Cin, H, W, seed=2)), w, (B, Cin, H, W), Cout, k, st, pad, dil)
        dx = ops.conv2d(bop, mk("dy", rn(B, Cout, Ho, Wo, seed=3)), w, (B, Cin, H, W), Cout, k, st, pad, dil)
        return dict(y=y, dx=dx)


for _tr, _Cin, _H, _W, _Cout, _B in ((False, 64, 16, 16, 96, 2), (False, 48, 9, 13, 80, 2), (True, 64, 12, 20, 48, 2), (False, 32, 6, 10, 40, 3)):
    for _math, _dt in ((None, F32), ("bf16x6", F32), ("bf16x3", BF16)):
        @case("winograd3_%s_c%d_%dx%d_k%d_%s_%s" % ("convT" if _tr else "conv", _Cin, _H, _W, _Cout, _math, "bf16" if _dt == BF16 else "fp32"),
              ["ipsr_conv3x3_winograd_mp", "ipsr_conv3x3_winograd_wrw_mp"], inplace=("cache",))
        def _(mk, tr=_tr, Cin=_Cin, H=_H, W=_W, Cout=_Cout, B=_B, math=_math, dt=_dt):
            from deepinpainting_amd import ops
            fop, bop = (ops.CONVT_FWD, ops.CONVT_BWD_DATA) if tr else (ops.CONV_FWD, ops.CONV_BWD_DATA)
            x, dy = mk("x", rn(B, Cin, H, W, seed=1, dtype=dt)), mk("dy", rn(B, Cout, H, W, seed=2, dtype=dt))
            w = mk("w", _w((Cin, Cout, 3, 3) if tr else (Cout, Cin, 3, 3), 3))
            bias = mk("bias", rn(Cout, seed=4))
            cache = ops.winograd_filter_cache(fop, Cin, Cout, x.device)
            y = ops.conv3x3_winograd(fop, x, w, (B, Cin, H, W), Cout, math=math)
            yr = ops.conv3x3_winograd(fop, x, w, (B, Cin, H, W), Cout, bias=bias, epilogue="relu", filter_cache=cache, math=math)
            yc = ops.conv3x3_winograd(fop, x, w, (B, Cin, H, W), Cout, bias=bias, epilogue="relu", filter_cache=cache, filter_cache_valid=True, math=math)
            res = dict(y=y, yr=yr, yc=yc, cache=cache)
            if H % 2 == 0 and W % 2 == 0:
                res["yp"] = ops.conv3x3_winograd(fop, x, w, (B, Cin, H, W), Cout, bias=bias, epilogue="relu_pool", math=math,
                                                 out_dtype=F32 if dt == BF16 else None)
            if ops.winograd_supported(bop, B, Cin, H, W, Cout):
                res["dx"] = ops.conv3x3_winograd(bop, dy, w, (B, Cin, H, W), Cout, math=math)
            res["dw"] = ops.conv3x3_winograd_wrw(tr, x, dy, Cout, math=math)
            return res


for _geom, _Cin, _H, _W, _Cout, _B, _math, _dt in [g + (None, F32) for g in ((0, 16, 6, 10, 24, 2), (0, 48, 14, 22, 20, 1), (1, 16, 7, 10, 32, 3),
                                                                              (1, 48, 13, 21, 20, 1), (0, 128, 32, 32, 128, 2))] + \
        [g + ("bf16x3", BF16) for g in ((0, 32, 16, 16, 48, 2), (1, 32, 7, 10, 32, 3))]:
    if True:
        @case("winograd4_g%d_c%d_%dx%d_k%d_%s" % (_geom, _Cin, _H, _W, _Cout, "bf16" if _dt == BF16 else "fp32"), ["ipsr_conv4x4_winograd_mp"])
        def _(mk, geom=_geom, Cin=_Cin, H=_H, W=_W, Cout=_Cout, B=_B, math=_math, dt=_dt):
            from deepinpainting_amd import ops
            Ho, Wo = (H // 2, W // 2) if geom == 0 else (H - 1, W - 1)
            x, dy = mk("x", rn(B, Cin, H, W, seed=1, dtype=dt)), mk("dy", rn(B, Cout, Ho, Wo, seed=2, dtype=dt))
            w = mk("w", _w((Cout, Cin, 4, 4), 3))
            ab = {0: (x, w), 1: (dy, w), 2: (x, dy)}
            return {"m%d" % m: ops.conv4x4_dilated_winograd(m, *ab[m], (B, Cin, H, W), Cout, geom=geom, math=math)
                    for m in (0, 1, 2) if ops.dilated_winograd_supported(m, B, Cin, H, W, Cout, geom)}


for _Kc, _Cf, _nh, _nw, _B, _math, _dt in [g + (None, F32) for g in ((16, 32, 5, 7, 3), (48, 20, 11, 6, 1), (64, 64, 1, 1, 4), (128, 64, 16, 16, 2))] + \
        [g + ("bf16x3", BF16) for g in ((48, 24, 11, 6, 1), (64, 32, 8, 8, 3))]:
    if True:
        @case("s2_%d_%d_%dx%d_%s" % (_Kc, _Cf, _nh, _nw, "bf16" if _dt == BF16 else "fp32"), ["ipsr_conv4x4s2_winograd_mp"])
        def _(mk, Kc=_Kc, Cf=_Cf, nh=_nh, nw=_nw, B=_B, math=_math, dt=_dt):
            from deepinpainting_amd import ops
            fine, coarse = mk("fine", rn(B, Cf, 2 * nh, 2 * nw, seed=1, dtype=dt)), mk("coarse", rn(B, Kc, nh, nw, seed=2, dtype=dt))
            w = mk("w", _w((Kc, Cf, 4, 4), 3))
            a = (B, Kc, Cf, nh, nw)
            return dict(c=ops.conv4x4s2_winograd(0, fine, w, *a, math=math), f=ops.conv4x4s2_winograd(1, coarse, w, *a, math=math),
                        dw=ops.conv4x4s2_winograd(2, fine, coarse, *a, math=math))


for _g in (("conv", 128, 128, 8, 8, 4, 2, 1, 1, 3), ("conv", 128, 256, 4, 6, 3, 1, 1, 1, 2), ("conv", 128, 256, 8, 8, 4, 2, 3, 2, 2),
           ("convT", 128, 64, 4, 4, 4, 2, 1, 1, 2), ("convT", 128, 128, 5, 3, 3, 1, 1, 1, 2), ("convT", 256, 128, 1, 1, 4, 2, 1, 1, 8)):
    @case("smallmap_%s_%d_%d_%dx%d_k%d_s%d_d%d" % (_g[0], _g[1], _g[2], _g[3], _g[4], _g[5], _g[6], _g[8]), ["ipsr_conv_smallmap"])
    def _(mk, g=_g):
        from deepinpainting_amd import ops
        import torch.nn.functional as F
        kind, Ci, Co, H, W, k, st, pad, dil, B = g
        tr = kind == "convT"
        w = mk("w", _w((Ci, Co, k, k) if tr else (Co, Ci, k, k), 1))
        x = mk("x", rn(B, Ci, H, W, seed=2))
        Hy, Wy = F.conv_transpose2d(torch.zeros(1, Ci, H, W), torch.zeros(Ci, Co, k, k), None, st, pad, 0, 1, dil).shape[2:] if tr else \
            F.conv2d(torch.zeros(1, Ci, H, W), torch.zeros(Co, Ci, k, k), None, st, pad, dil).shape[2:]
        dy = mk("dy", rn(B, Co, Hy, Wy, seed=3))
        if tr:
            geo = (B, Ci, Co, H, W, Hy, Wy, k, st, pad, dil)
            return dict(y=ops.conv_smallmap(ops.SM_DATA, x, w, *geo), dw=ops.conv_smallmap(ops.SM_WRW, x, dy, *geo),
                        dx=ops.conv_smallmap(ops.SM_FWD, dy, w, *geo))
        geo = (B, Co, Ci, Hy, Wy, H, W, k, st, pad, dil)
        return dict(dx=ops.conv_smallmap(ops.SM_DATA, dy, w, *geo), dw=ops.conv_smallmap(ops.SM_WRW, dy, x, *geo),
                    y=ops.conv_smallmap(ops.SM_FWD, x, w, *geo))


for _kind, _Ci, _Co, _H, _W, _B in (("conv", 3, 64, 32, 48, 2), ("conv", 6, 64, 20, 36, 3), ("convT", 128, 3, 24, 32, 2), ("convT", 32, 6, 9, 12, 1),
                                    ):
    for _io in ((F32, F32), (BF16, BF16), (F32, BF16), (BF16, F32)):
        @case("thin_%s_%d_%d_%dx%d_%s%s" % (_kind, _Ci, _Co, _H, _W, *("b" if d == BF16 else "f" for d in _io)),
              ["ipsr_conv3x3_thin_io", "ipsr_conv3x3_thin_wrw_io"])
        def _(mk, kind=_kind, Ci=_Ci, Co=_Co, H=_H, W=_W, B=_B, io=_io):
            from deepinpainting_amd import ops
            tr = kind == "convT"
            fop, bop = (ops.CONVT_FWD, ops.CONVT_BWD_DATA) if tr else (ops.CONV_FWD, ops.CONV_BWD_DATA)
            w = mk("w", _w((Ci, Co, 3, 3) if tr else (Co, Ci, 3, 3), 1))
            x, dy = mk("x", rn(B, Ci, H, W, seed=2, dtype=io[0])), mk("dy", rn(B, Co, H, W, seed=3, dtype=io[0]))
            res = {}
            if ops.thin_supported(fop, Ci, H, W, Co):
                few2many = Ci in (3, 6)
                res["y"] = ops.conv3x3_thin(fop, x, w, (B, Ci, H, W), Co, bias=mk("bias", rn(Co, seed=4)) if few2many else None, relu=few2many,
                                            out_dtype=io[1])
            if ops.thin_supported(bop, Ci, H, W, Co):
                res["dx"] = ops.conv3x3_thin(bop, dy, w, (B, Ci, H, W), Co, out_dtype=io[1])
            res["dw"] = ops.conv3x3_thin_wrw(tr, x, dy)
            return res


for _kind, _Ci, _Co, _H, _W, _B, _k, _st in (("conv", 6, 64, 20, 48, 3, 3, 1), ("conv", 3, 64, 32, 64, 2, 4, 2), ("convT", 128, 3, 24, 32, 2, 3, 1),
                                             ("convT", 72, 6, 12, 16, 2, 4, 2), ("conv", 3, 16, 8, 16, 1, 3, 1)):
    for _dt in (F32, BF16):
        @case("thin_mfma_%s_%d_%d_%dx%d_k%d_%s" % (_kind, _Ci, _Co, _H, _W, _k, "bf16" if _dt == BF16 else "fp32"),
              ["ipsr_conv_thin_wrw_mfma", "ipsr_conv_thin_f2m_mfma"])
        def _(mk, kind=_kind, Ci=_Ci, Co=_Co, H=_H, W=_W, B=_B, k=_k, st=_st, dt=_dt):
            from deepinpainting_amd import ops
            tr = kind == "convT"
            Ho, Wo = (H * st, W * st) if tr else (H // st, W // st)
            x, dy = mk("x", rn(B, Ci, H, W, seed=1, dtype=dt)), mk("dy", rn(B, Co, Ho, Wo, seed=2, dtype=dt))
            res = dict(dw=ops.conv_thin_wrw_mfma(tr, x, dy, k, st))
            w = mk("w", _w((Ci, Co, k, k) if tr else (Co, Ci, k, k), 3))
            op = ops.CONVT_BWD_DATA if tr else ops.CONV_FWD
            if ops.thin_f2m_mfma_supported(op, B, Ci, H, W, Co, k, st):
                inp = dy if tr else x
                for od in (BF16, F32):
                    res["f2m_%s" % od] = ops.conv_thin_f2m_mfma(op, inp, w, (B, Ci, H, W), Co, k, st, bias=None if tr else mk("bias", rn(Co, seed=4)),
                                                                relu=not tr, out_dtype=od)
            return res


for _B, _C, _H, _W, _K, _pad in ((3, 70, 9, 11, 3, 1), (2, 64, 20, 47, 4, 1), (1, 64, 5, 5, 4, 0), (8, 512, 31, 31, 4, 1)):
    @case("conv_to_one_%d_%d_%dx%d_k%d" % (_B, _C, _H, _W, _K), ["ipsr_conv_to_one"])
    def _(mk, B=_B, C=_C, H=_H, W=_W, K=_K, pad=_pad):
        from deepinpainting_amd import ops
        x, w = mk("x", rn(B, C, H, W, seed=1)), mk("w", _w((1, C, K, K), 2))
        y = ops.conv_to_one(x, w, pad)
        return dict(y=y, dw=ops.conv_to_one_wrw(x, mk("dy", rn(*y.shape, seed=3)), K, pad))


for _tr, _Cin, _H, _W, _Cout, _B in ((False, 32, 16, 16, 48, 2), (True, 64, 32, 64, 48, 2), (True, 32, 4, 256, 16, 2), (False, 256, 16, 16, 256, 2),
                                     (True, 512, 16, 16, 272, 3), (False, 512, 32, 32, 512, 16)):
    @case("bf16d_k3_%s_c%d_%dx%d_k%d_b%d" % ("convT" if _tr else "conv", _Cin, _H, _W, _Cout, _B), ["ipsr_conv3x3_bf16_packed", "ipsr_conv3x3_bf16_wrw"])
    def _(mk, tr=_tr, Cin=_Cin, H=_H, W=_W, Cout=_Cout, B=_B):
        from deepinpainting_amd import ops
        fop, bop = (ops.CONVT_FWD, ops.CONVT_BWD_DATA) if tr else (ops.CONV_FWD, ops.CONV_BWD_DATA)
        x, dy = mk("x", rn(B, Cin, H, W, seed=1, dtype=BF16)), mk("dy", rn(B, Cout, H, W, seed=2, dtype=BF16))
        w = mk("w", _w((Cin, Cout, 3, 3) if tr else (Cout, Cin, 3, 3), 3))
        res = {}
        if ops.conv3x3_bf16_supported(fop, B, Cin, H, W, Cout):
            res["y"] = ops.conv3x3_bf16(fop, x, w, (B, Cin, H, W), Cout)
            res["y32"] = ops.conv3x3_bf16(fop, x, w, (B, Cin, H, W), Cout, out_dtype=F32)
            res["y_miss"] = ops.conv3x3_bf16(fop, x, w, (B, Cin, H, W), Cout, keep_packed=True)         # packs into the cache
            res["y_hit"] = ops.conv3x3_bf16(fop, x, w, (B, Cin, H, W), Cout, keep_packed=True)          # reads it
        if ops.conv3x3_bf16_supported(bop, B, Cin, H, W, Cout):
            res["dx"] = ops.conv3x3_bf16(bop, dy, w, (B, Cin, H, W), Cout)
        if ops.conv3x3_bf16_wrw_supported(tr, B, Cin, H, W, Cout):
            res["dw"] = ops.conv3x3_bf16_wrw(tr, x, dy, Cout)
        assert res, "no bf16 direct pass supports this shape"
        return res


for _Kc, _Cf, _nh, _nw, _B in ((48, 32, 16, 16, 3), (200, 16, 32, 32, 1), (64, 64, 4, 64, 2), (256, 256, 16, 16, 2), (272, 512, 16, 16, 3)):
    @case("bf16d_s2_%d_%d_%dx%d_b%d" % (_Kc, _Cf, _nh, _nw, _B), ["ipsr_conv4x4s2_bf16", "ipsr_conv4x4s2_bf16_wrw"])
    def _(mk, Kc=_Kc, Cf=_Cf, nh=_nh, nw=_nw, B=_B):
        from deepinpainting_amd import ops
        fine, coarse = mk("fine", rn(B, Cf, 2 * nh, 2 * nw, seed=1, dtype=BF16)), mk("coarse", rn(B, Kc, nh, nw, seed=2, dtype=BF16))
        w = mk("w", _w((Kc, Cf, 4, 4), 3))
        a = (B, Kc, Cf, nh, nw)
        res = {}
        for mode in (ops.S2_FINE_TO_COARSE, ops.S2_COARSE_TO_FINE):
            if ops.conv4x4s2_bf16_supported(mode, *a):
                src = fine if mode == ops.S2_FINE_TO_COARSE else coarse
                res["m%d" % mode] = ops.conv4x4s2_bf16(mode, src, w, *a)
                res["m%d_f32" % mode] = ops.conv4x4s2_bf16(mode, src, w, *a, out_dtype=F32)
        if ops.conv4x4s2_bf16_wrw_supported(*a):
            res["dw"] = ops.conv4x4s2_bf16_wrw(fine, coarse, *a)
        assert res, "no bf16 stride-2 pass supports this shape"
        return res


# the split-bf16 kernels of the k4 s2 p1 layers on fp32 tensors.  Data passes: one channel block / ragged produced channels; the widest grid;
# the cut reduction (partials behind the packed planes)
for _B, _Kc, _Cf, _nh, _nw in ((2, 48, 16, 16, 16), (1, 64, 32, 4, 128), (1, 128, 128, 16, 16)):
    @case("bf16x3_s2_%d_%d_%dx%d_b%d" % (_Kc, _Cf, _nh, _nw, _B), ["ipsr_conv4x4s2_bf16x3"])
    def _(mk, Kc=_Kc, Cf=_Cf, nh=_nh, nw=_nw, B=_B):
        from deepinpainting_amd import ops
        fine, coarse = mk("fine", rn(B, Cf, 2 * nh, 2 * nw, seed=1)), mk("coarse", rn(B, Kc, nh, nw, seed=2))
        w = mk("w", rn(Kc, Cf, 4, 4, seed=3, scale=0.05))
        a = (B, Kc, Cf, nh, nw)
        return {"m0": ops.conv4x4s2_bf16x3(ops.S2_FINE_TO_COARSE, fine, w, *a), "m1": ops.conv4x4s2_bf16x3(ops.S2_COARSE_TO_FINE, coarse, w, *a)}


# weight gradient: one ragged tile, one stage; the widest grid, several runs per image; two stages per workgroup (the ring wraps)
for _B, _Kc, _Cf, _nh, _nw in ((1, 48, 16, 4, 16), (2, 64, 128, 3, 64), (2, 340, 380, 16, 16)):
    @case("bf16x3_s2_wrw_%d_%d_%dx%d_b%d" % (_Kc, _Cf, _nh, _nw, _B), ["ipsr_conv4x4s2_bf16x3_wrw"])
    def _(mk, Kc=_Kc, Cf=_Cf, nh=_nh, nw=_nw, B=_B):
        from deepinpainting_amd import ops
        fine, coarse = mk("fine", rn(B, Cf, 2 * nh, 2 * nw, seed=1)), mk("coarse", rn(B, Kc, nh, nw, seed=2))
        return {"dw": ops.conv4x4s2_bf16x3_wrw(fine, coarse, B, Kc, Cf, nh, nw)}


# ---- weight-gradient sinks: the gradient written straight into a slice of a bucket between two NaN neighbours, laid out as
# dist.py lays a bucket out (256-byte slots) and at the tightest offset the entries accept (16 bytes)
def _sink(mk, name, shape, pad_floats):
    n = 1
    for d in shape:
        n *= d
    lead = 64 if pad_floats == 64 else 4
    bucket = mk(name, nan_like((lead + n + (64 - n % 64) % 64 + 64,), F32))
    return bucket, bucket[lead:lead + n].view(shape), lead, n


def _neighbours_untouched(bucket, lead, n):
    torch.cuda.synchronize()
    b = bucket.view(torch.int32)
    assert bool((b[:lead] == NAN32).all()) and bool((b[lead + n:] == NAN32).all()), "a weight-gradient sink wrote into its neighbours"


for _pad in (64, 4):
    @case("sinks_offset%d" % (_pad * 4), ["ipsr_conv3x3_winograd_wrw_mp", "ipsr_conv4x4_winograd_mp", "ipsr_conv4x4s2_winograd_mp",
                                          "ipsr_conv_smallmap", "ipsr_conv3x3_thin_wrw_io", "ipsr_conv_thin_wrw_mfma", "ipsr_conv_to_one",
                                          "ipsr_conv3x3_bf16_wrw", "ipsr_conv4x4s2_bf16_wrw"],
          inplace=tuple("sink%d" % i for i in range(10)))
    def _(mk, pad=_pad):
        from deepinpainting_amd import ops
        res = {}
        calls = [
            ((20, 7, 3, 3), lambda o: ops.conv3x3_winograd_wrw(False, mk("x0", rn(2, 7, 9, 13, seed=1)), mk("dy0", rn(2, 20, 9, 13, seed=2)), 20, out=o)),
            ((24, 16, 4, 4), lambda o: ops.conv4x4_dilated_winograd(2, mk("x1", rn(2, 16, 6, 10, seed=3)), mk("dy1", rn(2, 24, 3, 5, seed=4)), (2, 16, 6, 10), 24, out=o)),
            ((16, 32, 4, 4), lambda o: ops.conv4x4s2_winograd(2, mk("f2", rn(3, 32, 10, 14, seed=5)), mk("c2", rn(3, 16, 5, 7, seed=6)), 3, 16, 32, 5, 7, out=o)),
            ((128, 128, 4, 4), lambda o: ops.conv_smallmap(ops.SM_WRW, mk("c3", rn(3, 128, 4, 4, seed=7)), mk("f3", rn(3, 128, 8, 8, seed=8)),
                                                           3, 128, 128, 4, 4, 8, 8, 4, 2, 1, 1, out=o)),
            ((64, 3, 3, 3), lambda o: ops.conv3x3_thin_wrw(False, mk("x4", rn(2, 3, 32, 48, seed=9)), mk("dy4", rn(2, 64, 32, 48, seed=10)), out=o)),
            ((64, 3, 4, 4), lambda o: ops.conv_thin_wrw_mfma(False, mk("x5", rn(2, 3, 32, 64, seed=11)), mk("dy5", rn(2, 64, 16, 32, seed=12)), 4, 2, out=o)),
            ((1, 70, 3, 3), lambda o: ops.conv_to_one_wrw(mk("x6", rn(3, 70, 9, 11, seed=13)), mk("dy6", rn(3, 1, 9, 11, seed=14)), 3, 1, out=o)),
            ((48, 32, 3, 3), lambda o: ops.conv3x3_bf16_wrw(False, mk("x7", rn(2, 32, 16, 16, seed=15, dtype=BF16)), mk("dy7", rn(2, 48, 16, 16, seed=16, dtype=BF16)), 48, out=o)),
            ((48, 32, 4, 4), lambda o: ops.conv4x4s2_bf16_wrw(mk("f8", rn(3, 32, 32, 32, seed=17, dtype=BF16)), mk("c8", rn(3, 48, 16, 16, seed=18, dtype=BF16)),
                                                              3, 48, 32, 16, 16, out=o)),
        ]
        for i, (shape, call) in enumerate(calls):
            bucket, sink, lead, n = _sink(mk, "sink%d" % i, shape, pad)
            try:
                call(sink)
            except RuntimeError as e:          # an entry that needs a 16-byte aligned destination refuses the 16-byte offset ... fine;
                assert pad != 64 and "align" in str(e), e      # on the bucket's own 256-byte slots every engine must take it
                continue
            _neighbours_untouched(bucket, lead, n)
            res["sink%d" % i] = bucket
        return res


# ---------------------------------------------------------------------------------------------------------------- the harness
def _declared():
    src = open(os.path.join(ROOT, "include", "ipsr_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(?:int|size_t|const char\s*\*)\s+((?:ipsr|innercos)_\w+)\s*\(", src)))


# entries that launch nothing: queries, workspace sizes, profile and debug switches
EXEMPT = {"ipsr_abi_version", "ipsr_last_error", "ipsr_bwd_index_ints", "ipsr_conv_thin_f2m_mfma_supported", "ipsr_conv3x3_winograd_filter_floats",
          "ipsr_wino_gemm_split", "ipsr_debug_force_wino_split", "ipsr_debug_set_option", "ipsr_profile_enable", "ipsr_profile_enable_mask",
          "ipsr_profile_read", "ipsr_profile_read_region", "ipsr_profile_read_region_work", "ipsr_profile_read_region_work2"}
# fp32-only / older forms that forward every argument to an entry of the table (same checks, same kernels)
ALIASES = {"ipsr_conv3x3_winograd": "ipsr_conv3x3_winograd_mp", "ipsr_conv3x3_winograd_ex": "ipsr_conv3x3_winograd_mp",
           "ipsr_conv4x4_winograd": "ipsr_conv4x4_winograd_mp", "ipsr_conv4x4_dilated_winograd": "ipsr_conv4x4_winograd_mp",
           "ipsr_conv4x4s2_winograd": "ipsr_conv4x4s2_winograd_mp", "ipsr_conv3x3_winograd_wrw": "ipsr_conv3x3_winograd_wrw_mp",
           "ipsr_conv3x3_thin": "ipsr_conv3x3_thin_io", "ipsr_conv3x3_thin_wrw": "ipsr_conv3x3_thin_wrw_io", "ipsr_conv3x3_bf16": "ipsr_conv3x3_bf16_packed"}


def test_every_launching_entry_has_a_row():
    """A new entry point of include/ipsr_hip.h without a row here (or an exemption by name) fails."""
    covered = {e for c in CASES for e in c[1]}
    missing = [n for n in _declared() if not n.endswith("_workspace_bytes") and n not in EXEMPT and ALIASES.get(n, n) not in covered]
    assert not missing, "entries without a guarded-memory case: %s" % missing
    assert set(ALIASES.values()) <= covered and not (EXEMPT | set(ALIASES)) - set(_declared())
    assert len({c[0] for c in CASES}) == len(CASES), "two rows share an id"


# outputs whose tail is capacity, not result: the backward's sparse index is sized by ipsr_bwd_index_ints (an upper bound) and filled
# to its used length; the Winograd filter cache is padded to the GEMM tiles and only the live rows are written.  Both sit between guard
# bands like every other buffer and start NaN / 0 in the guarded run; that their consumers (gin, yc) match the unguarded run bit for bit
# shows the unwritten tail is never read.
NOT_COMPARED = {"bidx", "cache"}


def _bits(t):
    return t.view({4: torch.int32, 2: torch.int16, 1: torch.uint8, 8: torch.int64}[t.element_size()])


def _same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(_bits(a.contiguous()), _bits(b.contiguous()))


@pytest.mark.gpu
@pytest.mark.parametrize("cid", [c[0] for c in CASES])
def test_guard_bands_and_poisoned_scratch(cid, monkeypatch):
    _, _, ws_fill, inplace, fn = next(c for c in CASES if c[0] == cid)
    torch.cuda.set_device(0)
    normal = fn(lambda name, t: t)
    torch.cuda.synchronize()
    normal = {k: v.clone() for k, v in normal.items() if v is not None}
    arena = Arena(ws_fill=ws_fill)
    placed = {}

    def mk(name, t):
        g = arena.guarded_copy(t, name)
        placed[name] = (g, t.clone())
        return g
    with arena.installed(monkeypatch):
        got = fn(mk)
    torch.cuda.synchronize()
    arena.check_guards()
    for name, (g, orig) in placed.items():
        if name not in inplace:
            assert _same_bits(g, orig), "%s: input %s was modified" % (cid, name)
    assert set(got) == set(normal)
    for k, v in got.items():
        if k in NOT_COMPARED:
            continue
        ref = normal[k]
        assert _same_bits(v, ref), "%s: %s differs from the unguarded run (max |diff| %s)" % (
            cid, k, float((v.double() - ref.double()).nan_to_num(1e30).abs().max()) if v.is_floating_point() else "n/a")
        if v.is_floating_point() and torch.isfinite(ref.float()).all():
            assert not torch.isnan(v.float()).any(), "%s: %s has unwritten elements" % (cid, k)
    assert arena.guard_bytes() > 0
