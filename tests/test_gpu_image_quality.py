"""csrc/image_quality.hip on the GPU against the float64 restatement of tests/quality_ref.py (F.conv2d in double on the CPU), through
`ops.image_quality`, the C entry and `deepinpainting_amd.metrics`.

Shapes: the smallest at which tiling, halos and ownership of input pixels can go wrong, T = the kernel's output-tile edge (quality_ref.T):
one output pixel, one more row / column, exactly one tile, one row / column past it, several tiles in both directions with ragged edges,
a one-row strip of four tiles, and one 256 x 256; C in {1, 3, 4} and B in {1, 3}, every pair present.

Bound: |SSIM - ref| <= 1e-10.  The kernel sums 121 taps (and the one-off exact products) in fp64: a window sum carries at most
~121 * 2^-53 = 1.4e-14 of values <= 1, the variances are differences of two such sums, divided by denominators >= C2 = 9e-4: ~1.5e-11 per
map value, and the mean cannot exceed its largest term.  The two streaming means: 1e-12 relative (fp64 sums of exact terms, ~2^-53 per
addition level).  Neither bound was tuned to the kernel; the figures are printed before they are asserted.
"""
import functools

import pytest
import torch

import quality_ref as R
import test_gpu_memory_bounds as M

T = R.T
SSIM_BOUND = 1e-10
MEAN_RTOL = 1e-12
FAMILIES = ("random_pair", "identical", "negated", "noisy_copy", "smooth_small_noise", "constants", "flat_cancellation")

# (H, W, C, B)
CASES = [(11, 11, 1, 1), (11, 11, 3, 3), (11, 12, 4, 1), (12, 11, 1, 3),
         (T + 10, T + 10, 3, 1), (T + 10, T + 10, 4, 3), (T + 11, T + 10, 1, 1), (T + 10, T + 11, 3, 3),
         (2 * T + 15, T + 13, 4, 3), (2 * T + 15, T + 13, 1, 1), (11, 3 * T + 13, 3, 1), (11, 3 * T + 13, 1, 3),
         (256, 256, 3, 1)]
assert {(c, b) for _, _, c, b in CASES} == {(c, b) for c in (1, 3, 4) for b in (1, 3)}


def _pair(family, B, C, H, W, seed):
    """-> (X, Y) fp32 CPU tensors in [-1, 1]."""
    g = torch.Generator().manual_seed(seed)
    shape = (B, C, H, W)
    u = lambda: torch.rand(shape, generator=g) * 2 - 1                      # noqa: E731
    n = lambda s: torch.randn(shape, generator=g) * s                       # noqa: E731
    if family == "random_pair":
        return u(), u()
    if family == "identical":
        x = u()
        return x, x.clone()
    if family == "negated":
        x = u()
        return x, -x
    if family == "noisy_copy":
        x = u()
        return x, (x + n(0.05)).clamp(-1, 1)
    if family == "smooth_small_noise":
        yy, xx = torch.meshgrid(torch.arange(H, dtype=torch.float32), torch.arange(W, dtype=torch.float32), indexing="ij")
        ph = torch.arange(B * C, dtype=torch.float32).view(B, C, 1, 1)
        s = 0.8 * torch.sin(0.11 * yy + 0.07 * xx + ph) * torch.cos(0.05 * xx - 0.03 * yy + 0.5 * ph)
        return (s + n(1e-3)).clamp(-1, 1), (s + n(1e-3)).clamp(-1, 1)
    if family == "constants":
        return torch.full(shape, 0.25), torch.full(shape, -0.5)
    if family == "flat_cancellation":                                       # s = E[x^2] - mu^2 ~ 1e-6 out of 0.81, against C2 = 9e-4
        return 0.9 + n(1e-3), 0.9 + n(1e-3)
    raise KeyError(family)


@functools.lru_cache(maxsize=None)
def _case(family, H, W, C, B):
    """The operands (CPU) and the float64 reference, computed once and shared."""
    X, Y = _pair(family, B, C, H, W, seed=1000 + FAMILIES.index(family) + 17 * H + W + 3 * C + B)
    assert float(X.abs().max()) <= 1 and float(Y.abs().max()) <= 1 and X.dtype == torch.float32
    return X, Y, R.quality(X, Y)


def _bits(t):
    return t.contiguous().view(torch.int64)


def _same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(_bits(a), _bits(b))


@pytest.fixture(scope="module")
def ops():
    import __graft_entry__ as g
    g.build()
    from deepinpainting_amd import ops as o
    torch.cuda.set_device(0)
    return o


@pytest.mark.gpu
@pytest.mark.parametrize("H,W,C,B", CASES, ids=["%dx%d_c%d_b%d" % c for c in CASES])
def test_against_the_fp64_restatement(ops, H, W, C, B):
    worst = []
    for family in FAMILIES:
        X, Y, ref = _case(family, H, W, C, B)
        got = ops.image_quality(X.cuda(), Y.cuda())
        assert got.shape == (B, 3) and got.dtype == torch.float64 and got.is_cuda
        got = got.cpu()
        e_ssim = float((got[:, 0] - ref[:, 0]).abs().max())
        e_mean = float(((got[:, 1:] - ref[:, 1:]).abs() / ref[:, 1:].abs().clamp_min(1e-300)).max())
        print("%-20s %dx%d C=%d B=%d: SSIM %+.6f .. %+.6f, |SSIM - ref| %.2e, streaming means rel %.2e"
              % (family, H, W, C, B, float(ref[:, 0].min()), float(ref[:, 0].max()), e_ssim, e_mean))
        worst.append((family, e_ssim, e_mean))
    for family, e_ssim, e_mean in worst:
        assert e_ssim <= SSIM_BOUND, (family, e_ssim)
        assert e_mean <= MEAN_RTOL, (family, e_mean)


@pytest.mark.gpu
@pytest.mark.parametrize("H,W,C,B", [(11, 11, 1, 1), (T + 11, T + 10, 3, 3), (2 * T + 15, T + 13, 4, 1), (11, 3 * T + 13, 1, 3), (10, 2 * T + 1, 3, 1), (1, 1, 1, 1)])
def test_small_integers_give_the_exact_means(ops, H, W, C, B):
    """(x - y)^2 and |x - y| of small integers sum exactly in fp64 in any order: the means equal the exact quotient bit for bit, so a pixel
    counted twice or not at all shows.  (The last two shapes are below the window: SSIM bit off.)"""
    g = torch.Generator().manual_seed(H * 1000 + W)
    X = torch.randint(-3, 4, (B, C, H, W), generator=g).float()
    Y = torch.randint(-3, 4, (B, C, H, W), generator=g).float()
    # every pixel a different weight as well: a swapped or doubled pixel cannot cancel
    X[0, 0].view(-1)[::7] += 8
    ssim = H >= 11 and W >= 11
    got = ops.image_quality(X.cuda(), Y.cuda(), ssim=ssim).cpu()
    d = (X.long() - Y.long()).flatten(1)
    n = C * H * W
    want = torch.tensor([[int((r * r).sum()) / n, int(r.abs().sum()) / n] for r in d], dtype=torch.float64)
    assert _same(got[:, 1:], want), (got[:, 1:], want)
    assert bool(torch.isnan(got[:, 0]).all()) != ssim


@pytest.mark.gpu
def test_repeatable_and_every_image_on_its_own(ops):
    H, W, C, B = 2 * T + 15, T + 13, 3, 3
    X, Y, _ = _case("noisy_copy", H, W, C, B)
    X, Y = X.cuda(), Y.cuda()
    a, b = ops.image_quality(X, Y), ops.image_quality(X, Y)
    assert _same(a, b)
    for i in range(B):
        alone = ops.image_quality(X[i:i + 1].contiguous(), Y[i:i + 1].contiguous())
        assert _same(alone[0], a[i]), i
    # another position in a longer batch
    rolled = ops.image_quality(torch.cat((X[2:], X, X[:1])), torch.cat((Y[2:], Y, Y[:1])))
    assert _same(rolled[1:4], a) and _same(rolled[0], a[2]) and _same(rolled[4], a[0])
    # a NaN in one image: that row NaN, the others the same bits
    Xn = X.clone()
    Xn[1, 2, T + 3, 5] = float("nan")
    c = ops.image_quality(Xn, Y)
    assert bool(torch.isnan(c[1]).all()) and _same(c[0], a[0]) and _same(c[2], a[2])
    c = ops.image_quality(Xn, Y, ssim=False)
    assert bool(torch.isnan(c[1]).all()) and _same(c[0, 1:], a[0, 1:]) and _same(c[2, 1:], a[2, 1:])


@pytest.mark.gpu
@pytest.mark.parametrize("H,W,C,B", [(11, 11, 1, 1), (T + 10, T + 11, 3, 3), (2 * T + 15, T + 13, 4, 3), (256, 256, 3, 1)])
def test_ssim_bit_off_keeps_the_streaming_columns(ops, H, W, C, B):
    X, Y, _ = _case("random_pair", H, W, C, B)
    X, Y = X.cuda(), Y.cuda()
    on, off = ops.image_quality(X, Y, ssim=True), ops.image_quality(X, Y, ssim=False)
    assert _same(on[:, 1:], off[:, 1:]) and bool(torch.isnan(off[:, 0]).all()) and bool(torch.isfinite(on).all())


@pytest.mark.gpu
def test_below_the_window_without_the_ssim_bit(ops):
    for H, W in ((10, 64), (64, 10), (3, 5)):
        g = torch.Generator().manual_seed(H)
        X, Y = torch.rand(2, 3, H, W, generator=g) * 2 - 1, torch.rand(2, 3, H, W, generator=g) * 2 - 1
        got = ops.image_quality(X.cuda(), Y.cuda(), ssim=False).cpu()
        ref = R.quality(X, Y, with_ssim=False)
        assert float(((got[:, 1:] - ref[:, 1:]).abs() / ref[:, 1:].abs()).max()) <= MEAN_RTOL


@pytest.mark.gpu
def test_half_precision_inputs_are_widened(ops):
    X, Y, _ = _case("random_pair", T + 11, T + 10, 1, 1)
    for dt in (torch.bfloat16, torch.float16):
        xh, yh = X.cuda().to(dt), Y.cuda().to(dt)
        assert _same(ops.image_quality(xh, yh), ops.image_quality(xh.float(), yh.float()))


# ---- guard bands, poisoned scratch: rows of the registry of tests/test_gpu_memory_bounds.py, run through its harness ------------------
GUARDED = [(11, 11, 1, 1), (T + 11, T + 10, 3, 3), (2 * T + 15, T + 13, 4, 1), (11, 3 * T + 13, 3, 2)]


def _gid(H, W, C, B):
    return "image_quality_%dx%d_c%d_b%d" % (H, W, C, B)


for _H, _W, _C, _B in GUARDED:
    if _gid(_H, _W, _C, _B) not in {c[0] for c in M.CASES}:           # a second import of this file must not enter a row twice
        @M.case(_gid(_H, _W, _C, _B), ("ipsr_image_quality",))
        def _(mk, H=_H, W=_W, C=_C, B=_B):
            from deepinpainting_amd import ops
            x = mk("x", (torch.rand(B, C, H, W, generator=M._gen(1)) * 2 - 1).cuda())
            y = mk("y", (torch.rand(B, C, H, W, generator=M._gen(2)) * 2 - 1).cuda())
            return dict(quality=ops.image_quality(x, y), streaming=ops.image_quality(x, y, ssim=False))


def test_the_rows_are_in_the_registry():
    covered = {c[0]: c[1] for c in M.CASES}
    assert all(covered.get(_gid(*s)) == ("ipsr_image_quality",) for s in GUARDED)
    assert "ipsr_image_quality" in M._declared() and "ipsr_image_quality" not in M.EXEMPT and "ipsr_image_quality" not in M.ALIASES


@pytest.mark.gpu
@pytest.mark.parametrize("cid", [_gid(*s) for s in GUARDED])
def test_guard_bands_and_poisoned_scratch(ops, cid, monkeypatch):
    M.test_guard_bands_and_poisoned_scratch(cid, monkeypatch)


@pytest.mark.gpu
def test_guarded_workspace_is_exactly_the_queried_size(ops, monkeypatch):
    from deepinpainting_amd import _lib
    from guarded import Arena
    H, W, C, B = T + 11, T + 13, 3, 2
    X, Y, _ = _case("random_pair", H, W, C, B)
    want = ops.image_quality(X.cuda(), Y.cuda())
    arena = Arena(ws_fill="nan")
    x, y = arena.guarded_copy(X.cuda(), "x"), arena.guarded_copy(Y.cuda(), "y")
    with arena.installed(monkeypatch):
        got = ops.image_quality(x, y)
    torch.cuda.synchronize()
    arena.check_guards()
    need = _lib.lib().ipsr_image_quality_workspace_bytes(B, C, H, W, 1)
    assert [n for n, _ in arena.workspaces] == [need] and need == R.workspace_bytes(B, C, H, W)
    assert _same(got, want) and torch.equal(x.cpu(), X) and torch.equal(y.cpu(), Y)


# ---- refusals ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_refused_calls_write_nothing(ops):
    from deepinpainting_amd import _lib
    L = _lib.lib()
    B, C = 2, 3
    x, y = torch.rand(B, C, 64, 64, device="cuda"), torch.rand(B, C, 64, 64, device="cuda")
    win = ops._iq_window(x.device)
    need = L.ipsr_image_quality_workspace_bytes(B, C, 64, 64, 1)
    out = torch.full((B, 3), float("nan"), dtype=torch.float64, device="cuda")
    ws = torch.empty(need // 8, dtype=torch.float64, device="cuda")
    _bits(out).fill_(0x7ff8000000c0ffee)
    _bits(ws).fill_(0x7ff8000000c0ffee)
    keep_out, keep_ws = out.clone(), ws.clone()
    st = ops._stream()

    def call(xp=x.data_ptr(), shape=(B, C, 64, 64), flags=1, ws_bytes=need):
        return L.ipsr_image_quality(xp, y.data_ptr(), *shape, flags, win.data_ptr(), out.data_ptr(), ws.data_ptr(), ws_bytes, st)
    assert call(shape=(B, C, 10, 64)) == -2 and b"SSIM needs" in L.ipsr_last_error()
    assert call(shape=(B, C, 64, 10)) == -2 and b"SSIM needs" in L.ipsr_last_error()
    assert call(ws_bytes=need - 8) == -3 and b"workspace" in L.ipsr_last_error()
    assert call(xp=None) == -1 and b"null pointer" in L.ipsr_last_error()
    torch.cuda.synchronize()
    assert _same(out, keep_out) and _same(ws, keep_ws)
    assert call() == 0                                                  # the same buffers are fine for the call that is not refused
    torch.cuda.synchronize()
    assert bool(torch.isfinite(out).all())
    # through ops
    with pytest.raises(NotImplementedError, match="SSIM needs"):
        ops.image_quality(x[:, :, :10].contiguous(), y[:, :, :10].contiguous())
    with pytest.raises(NotImplementedError, match="SSIM needs"):
        ops.image_quality(x[:, :, :, :10].contiguous(), y[:, :, :, :10].contiguous())
    with pytest.raises(RuntimeError, match="bad size"):
        ops.image_quality(x[:0], y[:0])
    with pytest.raises(RuntimeError, match="one shape"):
        ops.image_quality(x, y[:1])
    with pytest.raises(TypeError):
        ops.image_quality(x.double(), y.double())


# ---- the module ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_metrics_module_is_the_kernel(ops):
    from deepinpainting_amd import metrics
    H, W, C, B = 2 * T + 15, T + 13, 3, 3
    X, Y, ref = _case("noisy_copy", H, W, C, B)
    Xc, Yc = X.cuda(), Y.cuda()
    q = ops.image_quality(Xc, Yc)
    s = metrics.SSIM(channels=3)(Xc, Yc, as_loss=False)
    assert s.shape == (B,) and s.dtype == torch.float32 and s.is_cuda and not s.requires_grad
    assert torch.equal(s, q[:, 0].float())
    p = metrics.psnr(Xc, Yc)
    assert p.shape == (B,) and p.is_cuda
    assert float((p.cpu() - R.psnr_of_mse(ref[:, 1])).abs().max()) <= 1e-9          # 10 log10 of a value good to 1e-12 relative
    assert float((metrics.psnr(Xc, Yc, peak=1.0).cpu() - R.psnr_of_mse(ref[:, 1], 1.0)).abs().max()) <= 1e-9
    same = metrics.psnr(Xc, Xc.clone())
    assert bool((same == 100.0).all())
