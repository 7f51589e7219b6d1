"""The bf16 correlation of the IPSR layer for shift_sz > 1 (p x p windows): `ops.forward(..., patch=p, corr="bf16")`.

Contract: the 1x1 correlation R = x^T ref of the shifted-sum form runs on the bf16 matrix cores, x and ref rounded to bf16
once (products exact, fp32 accumulation); the p x p window stencil, the window norm, the arg-max and its tie rule, and everything
after the correlation (recurrence, reconstruction, fold, backward index) are the fp32 p > 1 path unchanged.  The bf16 operands
have a row stride of h*w rounded up to 128.
"""
import ctypes

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from guarded import Arena
from oracle import ipsr_oracle as orc

pytestmark = pytest.mark.gpu

IPSR_ERR_UNSUPPORTED = -2


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    from deepinpainting_amd import ops as _ops
    return _ops


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def features(B, C, h, w, seed, signed_ref=False):
    """x >= 0 and ref = ReLU(noise) like relu4_3 features (signed_ref: ref = -|noise| for sample 0 (every correlation of
    that sample negative, so a zero pad row would win an arg-max it is not bounded out of), plain noise for the others)."""
    x = torch.randn(B, C, h, w, generator=_gen(seed)).abs()
    r = torch.randn(B, C, h, w, generator=_gen(seed + 1))
    if signed_ref:
        ref = r.clone()
        ref[0] = -r[0].abs()
    else:
        ref = r.clamp_min(0)
    return x.cuda(), ref.cuda()


def hole(ops, h, w, p):
    """centre-square hole on the feature grid -> (mask_point_idx [M] i32 on the window grid, masked-window flags [nH, nW])."""
    feat = torch.zeros(h, w, dtype=torch.uint8)
    feat[h // 4:h - h // 4, w // 4:w - w // 4] = 1
    _, mpi, cnt = ops.index_prep(feat.cuda(), p, 1, 1)
    M = int(cnt.item())
    masked = np.zeros((h - p + 1) * (w - p + 1), bool)
    masked[mpi[:M].cpu().numpy()] = True
    return mpi[:M].contiguous(), masked.reshape(h - p + 1, w - p + 1)


def window_corr64(x, ref, p):
    """fp64 window correlation on the unrounded operands: S[k'][q'] = <x_k' / (|x_k'| + 1e-8), ref_q'>, and the magnitude
    sum A[k'][q'] = sum over the window's taps of |xn * ref| (the scale of the two bf16 roundings)."""
    xu = F.unfold(x[None].double(), p)[0]                        # [K, N'], taps in (c, dy, dx) order
    ru = F.unfold(ref[None].double(), p)[0]
    xn = xu / (xu.pow(2).sum(0).sqrt() + 1e-8)
    return xn.t() @ ru, xn.abs().t() @ ru.abs()


@pytest.mark.parametrize("B,C,h,w,p,check", [(1, 512, 32, 32, 3, 1), (2, 64, 12, 20, 2, 2), (4, 512, 64, 64, 3, 2)])
def test_bf16_window_correlation_contract(ops, B, C, h, w, p, check):
    """vmax[q'] is within tol[q'] of the fp64 correlation at the reported index, and that index is within 2 tol[q'] of the
    column maximum.  tol = 2^-8 sum|xn * ref| (two bf16 roundings) + K 2^-24 of it (fp32 accumulation), the largest over the
    column.  [2,64,12,20] p = 2: h*w = 240 in a 256-column stride (N' = 209), K = 256; its sample 0 has only negative
    correlations, so a zero pad column would win an arg-max it reached."""
    x, ref = features(B, C, h, w, seed=B + C + h + p, signed_ref=(p == 2))
    mpi, _ = hole(ops, h, w, p)
    f16 = ops.forward(x, ref, mpi, patch=p, corr="bf16")
    f32 = ops.forward(x, ref, mpi, patch=p)
    torch.cuda.synchronize()
    Np, K = (h - p + 1) * (w - p + 1), C * p * p
    ind, vmax = f16.ind, f16.vmax
    assert int(ind.min()) >= 0 and int(ind.max()) < Np
    for b in range(check):
        S, A = window_corr64(x[b], ref[b], p)
        q = torch.arange(Np, device=S.device)
        got = S[ind[b].long(), q]
        tol = (2.0 ** -8 + K * 2.0 ** -24) * A.max(0).values
        assert bool(((vmax[b].double() - got).abs() <= tol).all()), "vmax is not the correlation at the reported index"
        assert bool((S.max(0).values - got <= 2 * tol).all()), "the reported index does not attain the column maximum"
        del S, A
    agree = float((ind == f32.ind).double().mean())
    print("bf16 vs fp32 window arg-max agreement B=%d C=%d %dx%d p=%d: %.4f" % (B, C, h, w, p, agree))
    assert agree > 0.80


def test_bf16_window_layer_p3_matches_fp32_where_the_windows_agree(ops):
    """Whole layer, p = 3, centre hole: a pixel covered only by unmasked windows whose arg-max is the same in both runs is the
    same sum of the same fp32 patch copies (fold) bit for bit; the error against the fp32 oracle is reported; the backward on
    the bf16 forward's index runs."""
    B, C, h, p = 2, 512, 32, 3
    x, ref = features(B, C, h, h, seed=7)
    mpi, masked = hole(ops, h, h, p)
    M = mpi.numel()
    f16 = ops.forward(x, ref, mpi, patch=p, corr="bf16")
    f32 = ops.forward(x, ref, mpi, patch=p)
    o16, o32 = f16.out.cpu().numpy(), f32.out.cpu().numpy()
    assert np.isfinite(o16).all()
    nW = h - p + 1
    same = (f16.ind == f32.ind).cpu().numpy().reshape(B, nW, nW)
    agree = same.mean()
    checked = 0
    for b in range(B):
        badw = masked | ~same[b]
        bad = np.zeros((h, h), bool)
        for dy in range(p):
            for dx in range(p):
                bad[dy:dy + nW, dx:dx + nW] |= badw
        good = ~bad
        checked += int(good.sum())
        np.testing.assert_array_equal(o16[b][:, good], o32[b][:, good])
    assert checked > 0
    fo = orc.forward(x[:1].cpu().numpy(), ref[:1].cpu().numpy(), mpi.cpu().numpy(), patch=p)
    err = np.abs(o16[0] - fo.out[0])
    print("bf16-corr layer p=3: arg-max agreement %.4f, %d pixels bit-equal to fp32, |out - fp32 oracle| max %.3e mean %.3e (sample 0)"
          % (agree, checked, err.max(), err.mean()))
    assert agree > 0.80
    g = torch.randn(B, C, h, h, generator=_gen(3)).cuda()
    gin = ops.backward(g, f16.bwd_index, 1.0, M, patch=p)
    assert bool(torch.isfinite(gin).all())


def test_bf16_window_per_sample_masks_equal_batch_of_one(ops):
    """ipsr_forward_masks with corr_bf16 = 1 and one index row per sample: each sample is bit for bit the batch-of-one call."""
    B, C, h, p = 3, 64, 16, 3
    x, ref = features(B, C, h, h, seed=11)
    rows = []
    for i, prob in enumerate((0.3, 0.1, 0.6)):
        feat = (torch.rand(h, h, generator=_gen(20 + i)) < prob).to(torch.uint8).cuda()
        rows.append(ops.index_prep(feat, p, 1, 1))
    mpi = torch.stack([r[1] for r in rows])
    counts = torch.cat([r[2] for r in rows])
    f = ops.forward(x, ref, mpi, patch=p, corr="bf16", counts=counts)
    for b in range(B):
        M = int(counts[b].item())
        assert M > 0
        one = ops.forward(x[b:b + 1].contiguous(), ref[b:b + 1].contiguous(), mpi[b, :M].contiguous(), patch=p, corr="bf16")
        for name in ("out", "ind", "vmax"):
            a, e = getattr(f, name)[b:b + 1], getattr(one, name)
            assert torch.equal(a.view(torch.int32), e.view(torch.int32)), "sample %d: %s differs from its batch-of-one call" % (b, name)


def used_index(bwd_index, N, M):
    """The defined part of the sparse trunc(kbar) (the tail past what a call uses is never written): offA, the N-M one-hot
    entries, offB, the offB[N] survivors (q, weight bits)."""
    capB = M * (M + 1) // 2
    out = []
    for row in bwd_index.cpu().numpy():
        offA, entA = row[:N + 1], row[N + 1:2 * N + 1]
        offB = row[2 * N + 1:3 * N + 2]
        nb = int(offB[N])
        entBq = row[3 * N + 2:3 * N + 2 + nb]
        entBw = row[3 * N + 2 + capB:3 * N + 2 + capB + nb]
        out.append(np.concatenate([offA, entA[:N - M], offB, entBq, entBw]))
    return out


def test_bf16_window_forward_is_repeatable(ops):
    B, C, h, p = 2, 512, 32, 3
    x, ref = features(B, C, h, h, seed=13)
    mpi, _ = hole(ops, h, h, p)
    a = ops.forward(x, ref, mpi, patch=p, corr="bf16")
    b = ops.forward(x, ref, mpi, patch=p, corr="bf16")
    for name in ("out", "ind", "vmax"):
        assert torch.equal(getattr(a, name).view(torch.int32), getattr(b, name).view(torch.int32)), name
    Np, M = (h - p + 1) ** 2, mpi.numel()
    for ra, rb in zip(used_index(a.bwd_index, Np, M), used_index(b.bwd_index, Np, M)):
        np.testing.assert_array_equal(ra, rb)


@pytest.mark.parametrize("ws_fill", ["zero", "stale"])
@pytest.mark.parametrize("B,C,h,w", [(2, 64, 16, 16), (2, 128, 20, 22)])
def test_bf16_window_forward_in_guarded_memory(ops, monkeypatch, ws_fill, B, C, h, w):
    """Every buffer between guard bands and the workspace exactly the size the query reports: the guards stay intact, the inputs
    are unchanged, and every result is bit for bit the unguarded run's."""
    p = 3
    x0, ref0 = features(B, C, h, w, seed=B + C + h)
    mpi0, _ = hole(ops, h, w, p)
    plain = ops.forward(x0, ref0, mpi0, patch=p, corr="bf16", want_attn=True)
    torch.cuda.synchronize()
    arena = Arena(ws_fill=ws_fill)
    x, ref, mpi = arena.guarded_copy(x0, "x"), arena.guarded_copy(ref0, "ref"), arena.guarded_copy(mpi0, "mpi")
    with arena.installed(monkeypatch):
        f = ops.forward(x, ref, mpi, patch=p, corr="bf16", want_attn=True)
    torch.cuda.synchronize()
    arena.check_guards()
    for name, t, t0 in (("x", x, x0), ("ref", ref, ref0), ("mpi", mpi, mpi0)):
        assert torch.equal(t.view(torch.int32), t0.view(torch.int32)), "input %s was written" % name
    for name in ("out", "ind", "vmax", "attn_rows"):
        assert torch.equal(getattr(f, name).view(torch.int32), getattr(plain, name).view(torch.int32)), name
    assert bool(torch.isfinite(f.out).all()) and bool(torch.isfinite(f.vmax).all())


def test_bf16_window_refuses_c_not_multiple_of_64(ops):
    """C = 24, p = 3: the bf16 correlation contracts over C, which is not a multiple of 64.  ops.forward raises; the C entry returns IPSR_ERR_UNSUPPORTED and leaves
    every pre-filled output as it was (no silent fp32 run, nothing written)."""
    from deepinpainting_amd import _lib
    L = _lib.lib()
    B, C, h, p = 1, 24, 12, 3
    x, ref = features(B, C, h, h, seed=17)
    mpi, _ = hole(ops, h, h, p)
    M, Np = mpi.numel(), (h - p + 1) ** 2
    with pytest.raises(NotImplementedError):
        ops.forward(x, ref, mpi, patch=p, corr="bf16")
    out = torch.full((B, C, h, h), 7.0, device="cuda")
    ind = torch.full((B, Np), 12345, dtype=torch.int32, device="cuda")
    vmax = torch.full((B, Np), -3.0, device="cuda")
    keep = [t.clone() for t in (out, ind, vmax)]
    nbytes = L.ipsr_forward_bf16corr_workspace_bytes(B, C, h, h, M, p, 1)
    assert nbytes > 0
    ws = torch.zeros(nbytes, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    rc = L.ipsr_forward_bf16corr(x.data_ptr(), ref.data_ptr(), mpi.data_ptr(), M, B, C, h, h, p, 1, out.data_ptr(), ind.data_ptr(),
                                 vmax.data_ptr(), None, None, ws.data_ptr(), ctypes.c_size_t(nbytes), ops._stream())
    torch.cuda.synchronize()
    assert rc == IPSR_ERR_UNSUPPORTED, (rc, L.ipsr_last_error())
    for name, a, e in zip(("out", "ind", "vmax"), (out, ind, vmax), keep):
        assert torch.equal(a, e), "%s was written by a refused call" % name


def _trainer(tmp_path, bf16_corr, steps):
    import contextlib
    import io
    from deepinpainting_amd import ops
    from deepinpainting_amd.options import Option
    from deepinpainting_amd.models.models import create_model
    g = torch.Generator(device="cuda").manual_seed(5)
    img = torch.rand(2, 3, 256, 256, device="cuda", generator=g) * 2 - 1
    ref = torch.rand(2, 3, 256, 256, device="cuda", generator=g) * 2 - 1
    mask = torch.zeros(1, 1, 256, 256, dtype=torch.bool, device="cuda")
    mask[:, :, 64:192, 64:192] = 1
    opt = Option(gpu_ids=[0], batchSize=2, fineSize=256, shift_sz=3, amp_bf16=True, bf16_corr=bf16_corr, allow_random_vgg=True,
                 use_dropout=False, quiet=True, checkpoints_dir=str(tmp_path / str(bf16_corr)))
    with contextlib.redirect_stdout(io.StringIO()):
        m = create_model(opt)
    seen = []
    real_forward = ops.forward

    def spying_forward(*a, **k):
        patch = a[3] if len(a) > 3 else k.get("patch", 1)
        corr = k.get("corr") or getattr(ops._precision, "corr", "fp32")
        seen.append((int(patch), corr))
        return real_forward(*a, **k)

    w0 = m.netG.model.model[0].weight.detach().clone()
    losses = []
    ops.forward = spying_forward
    try:
        for _ in range(steps):
            m.set_input(img, mask, ref)
            m.set_ref_latent()
            m.set_gt_latent()
            m.optimize_parameters()
            e = m.get_current_errors()
            losses.append([e['G_GAN'], e['G_L1'], e['D'], e['F'], float(m.ng_loss_value), float(m.ng_loss_value2)])
    finally:
        ops.forward = real_forward
    moved = not torch.equal(m.netG.model.model[0].weight, w0)
    del m
    torch.cuda.empty_cache()
    return losses, seen, moved


def test_trainer_amp_bf16_with_3x3_patches(tmp_path):
    """amp_bf16 with shift_sz = 3 trains (it raised NotImplementedError before): two steps, finite losses, netG's first weight
    moves, and the layer ran with the bf16 correlation at patch 3.  bf16_corr = False keeps the fp32 correlation."""
    losses, seen, moved = _trainer(tmp_path, True, 2)
    assert all(np.isfinite(v) for row in losses for v in row), losses
    assert moved
    assert seen and all(s == (3, "bf16") for s in seen), seen
    losses, seen, moved = _trainer(tmp_path, False, 1)
    assert all(np.isfinite(v) for row in losses for v in row), losses
    assert seen and all(s == (3, "fp32") for s in seen), seen
