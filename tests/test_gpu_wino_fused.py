"""The one-launch Winograd F(4x4,3x3) kernel (csrc/wino_fused.hip) against an fp64 convolution of the same operands.

`ipsr_debug_set_option(7, v)` chooses the form of a 3x3 data pass inside launch_winograd: 0 = the size rule, 1 = always the three
launches (transforms, 36 GEMMs, output transform), 2 = the fused kernel wherever its envelope allows (fp32 arithmetic on fp32
tensors, at most 64 produced channels, reduction a multiple of 16) whatever the size, which is how these small shapes reach it.

Bound: the Winograd bound of tests/test_gpu_wino_cuts.py, max |got - ref| <= 1e-4 max |ref|, for the fused form and, on the same
operands, for the three-launch form.  The two forms need not agree bit for bit (and nothing here asks them to).

Shapes (B, reduction C, produced K, H x W): B 1 and 3; C 16 (one chunk) and 48; K 64, 40 and 16 (padded rows of the filter and of
the accumulators); 5x7 (one partial tile), 8x64 (exactly one block of 2 x 16 tiles, vector rows), 9x65 (one pixel over in both
directions: four blocks, three of them nearly empty), 37x70 / 38x70 (several blocks, ragged rows, no vector rows); all four ops;
bias present and absent; no epilogue, relu, relu_pool (even extents).  Each case also checks that a second run gives the same bits
and that a call on a valid filter cache (one launch) gives the bits of the call that filled it (two launches).

Which form a call took is observed from outside through the scratch buffer: with a valid filter cache the fused form writes nothing
to the workspace, while the three launches fill it with the transformed windows and the products.
"""
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

FUSED_OPTION = 7          # ipsr_debug_set_option key: 0 = the rule, 1 = never fused, 2 = fused wherever the envelope allows
TOL = 1e-4


def _set(v):
    from deepinpainting_amd import _lib
    _lib.check(_lib.lib().ipsr_debug_set_option(FUSED_OPTION, v), "ipsr_debug_set_option")


@pytest.fixture(autouse=True)
def option_restored():
    yield
    _set(0)


# (op, B, C reduced, K produced, H, W, bias, epilogue)
CASES = [
    ("conv_fwd", 1, 16, 64, 5, 7, False, None),
    ("conv_fwd", 3, 48, 40, 9, 65, True, "relu"),
    ("conv_fwd", 3, 16, 16, 8, 64, True, "relu_pool"),
    ("conv_fwd", 1, 48, 64, 38, 70, False, "relu_pool"),
    ("conv_fwd", 3, 48, 64, 37, 70, False, None),
    ("conv_fwd", 3, 48, 40, 8, 64, False, "relu"),
    ("conv_fwd", 1, 16, 40, 38, 70, True, "relu_pool"),
    ("conv_bwd", 1, 48, 40, 9, 65, False, None),
    ("conv_bwd", 3, 16, 64, 8, 64, False, None),
    ("convT_fwd", 3, 48, 16, 37, 70, True, "relu"),
    ("convT_fwd", 1, 16, 64, 8, 64, False, None),
    ("convT_bwd", 3, 16, 40, 5, 7, False, None),
    ("convT_bwd", 1, 48, 64, 37, 70, False, None),
]
IDS = ["%s-b%d-c%d-k%d-%dx%d-%s-%s" % (op, B, C, K, H, W, "bias" if bias else "nobias", epi or "none") for op, B, C, K, H, W, bias, epi in CASES]


def _operands(op, B, C, K, H, W, bias, seed):
    """-> (ops code, input, weight, bias, in_shape, Cout, fp64 convolution without bias or epilogue)."""
    from deepinpainting_amd import ops
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, C, H, W, generator=g)
    fwd = op.endswith("fwd")
    Cin, Cout = (C, K) if fwd else (K, C)
    w = torch.randn(*((Cin, Cout, 3, 3) if op.startswith("convT") else (Cout, Cin, 3, 3)), generator=g) * 0.1
    bv = torch.randn(K, generator=g) if bias else None
    x64, w64 = x.double(), w.double()
    if op in ("conv_fwd", "convT_bwd"):          # the input gradient of a transposed convolution is a convolution, and the other way round
        ref = F.conv2d(x64, w64, None, 1, 1)
    else:
        ref = F.conv_transpose2d(x64, w64, None, 1, 1)
    code = {"conv_fwd": ops.CONV_FWD, "conv_bwd": ops.CONV_BWD_DATA, "convT_fwd": ops.CONVT_FWD, "convT_bwd": ops.CONVT_BWD_DATA}[op]
    return code, x.cuda(), w.cuda(), (bv.cuda() if bias else None), (B, Cin, H, W), Cout, ref, bv


def _finish(ref, bv, epi):
    if epi is None:
        return ref
    if bv is not None:
        ref = ref + bv.double().view(1, -1, 1, 1)
    ref = torch.relu(ref)
    return F.max_pool2d(ref, 2, 2) if epi == "relu_pool" else ref


def _rel(got, ref):
    return float((got.double().cpu() - ref).abs().max() / ref.abs().max())


def _same_bits(a, b):
    return a.shape == b.shape and torch.equal(a.view(torch.int32), b.view(torch.int32))


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_fused_and_three_launch_forms_vs_fp64(case):
    from deepinpainting_amd import ops
    op, B, C, K, H, W, bias, epi = case
    code, x, w, bv, in_shape, Cout, ref, bv_cpu = _operands(op, B, C, K, H, W, bias, seed=B * 1000 + C * 7 + K + H * W)
    ref = _finish(ref, bv_cpu, epi)
    cache = ops.winograd_filter_cache(code, in_shape[1], Cout, x.device)

    def run(**kw):
        y = ops.conv3x3_winograd(code, x, w, in_shape, Cout, bias=bv, epilogue=epi, **kw)
        torch.cuda.synchronize()
        return y

    _set(2)
    y_plain = run()
    y_again = run()
    y_fill = run(filter_cache=cache, filter_cache_valid=False)
    y_hit = run(filter_cache=cache, filter_cache_valid=True)
    _set(1)
    y_three = run()
    _set(0)
    err_fused, err_three = _rel(y_plain, ref), _rel(y_three, ref)
    print("%s: fused %.3e  three launches %.3e  (bound %.0e)" % (IDS[CASES.index(case)], err_fused, err_three, TOL))
    assert tuple(y_plain.shape) == tuple(ref.shape) and y_plain.dtype == torch.float32
    assert err_fused <= TOL, ("fused", case, err_fused)
    assert err_three <= TOL, ("three launches", case, err_three)
    assert _same_bits(y_plain, y_again), "two runs of the fused kernel differ"
    assert _same_bits(y_fill, y_plain) and _same_bits(y_hit, y_fill), "the filter cache changes the fused kernel's result"


def test_relu_pool_propagates_nan_like_the_three_launch_form():
    """One NaN input: both forms give NaN in the same places, a superset of torch's (the 3x3 reach of the pixel, through ReLU and the
    max-pool), and meet the bound everywhere else."""
    from deepinpainting_amd import ops
    B, C, K, H, W = 1, 16, 40, 16, 64
    code, x, w, bv, in_shape, Cout, _, bv_cpu = _operands("conv_fwd", B, C, K, H, W, True, seed=5)
    x[0, 3, 7, 20] = float("nan")
    ref = _finish(F.conv2d(x.double().cpu(), w.double().cpu(), None, 1, 1), bv_cpu, "relu_pool")
    out = {}
    for v in (2, 1):
        _set(v)
        out[v] = ops.conv3x3_winograd(code, x, w, in_shape, Cout, bias=bv, epilogue="relu_pool")
        torch.cuda.synchronize()
    _set(0)
    nan_ref = torch.isnan(ref)
    assert bool(nan_ref.any())
    for v in (2, 1):
        got = out[v].cpu()
        nan_got = torch.isnan(got)
        assert bool((nan_got | ~nan_ref).all()), "a NaN of the reference is missing (option %d)" % v
        ok = ~nan_got
        err = float((got.double() - ref)[ok].abs().max() / ref[~nan_ref].abs().max())
        assert err <= TOL, (v, err)
    # (pixel (7, 20) lies in the windows of four tiles; which of their outputs turn NaN follows the zeros of B^T and A^T, the same in both forms)
    assert torch.equal(torch.isnan(out[2]), torch.isnan(out[1])), "the two forms put NaN in different places"


# ---- which form a call takes ---------------------------------------------------------------------------------------------------------
WORD = 0x7fc0beef          # a NaN pattern no kernel produces
RULE_MIN_TILES = 8192      # WF_MIN_TILES of csrc/wino_fused.hip: the measured rule (profiles/wino_fused_layers.txt)


def _workspace_written(monkeypatch, op, B, C, K, H, W, math=None, bf16=False):
    """Runs one call on a VALID filter cache with a scratch buffer full of WORD; True when the call wrote to the scratch."""
    from deepinpainting_amd import ops
    code = {"conv_fwd": ops.CONV_FWD, "convT_fwd": ops.CONVT_FWD}[op]
    dt = torch.bfloat16 if bf16 else torch.float32
    x = torch.randn(B, C, H, W, device="cuda").to(dt)
    w = torch.randn(*((C, K, 3, 3) if op == "convT_fwd" else (K, C, 3, 3)), device="cuda") * 0.1
    cache = ops.winograd_filter_cache(code, C, K, x.device)
    was = ops.conv3x3_winograd(code, x, w, (B, C, H, W), K, filter_cache=cache, filter_cache_valid=False, math=math)      # fills the cache
    held = {}

    def poisoned(nbytes, device):
        buf = torch.empty((int(nbytes) + 3) // 4, dtype=torch.int32, device=device)
        buf.fill_(WORD)
        held["ws"] = buf
        return buf.view(torch.uint8)

    monkeypatch.setattr(ops, "_workspace", poisoned)
    y = ops.conv3x3_winograd(code, x, w, (B, C, H, W), K, filter_cache=cache, filter_cache_valid=True, math=math)
    torch.cuda.synchronize()
    monkeypatch.undo()
    assert torch.equal(y.view(torch.int16 if bf16 else torch.int32), was.view(torch.int16 if bf16 else torch.int32))
    return not bool((held["ws"] == WORD).all())


def test_the_rule_leaves_a_small_shape_on_three_launches(monkeypatch):
    _set(0)
    assert _workspace_written(monkeypatch, "conv_fwd", 3, 48, 40, 9, 65)
    _set(2)
    assert not _workspace_written(monkeypatch, "conv_fwd", 3, 48, 40, 9, 65)
    _set(1)
    assert _workspace_written(monkeypatch, "conv_fwd", 3, 48, 40, 9, 65)


@pytest.mark.parametrize("op,B,C,K,H", [("conv_fwd", 8, 64, 64, 256), ("convT_fwd", 8, 256, 64, 128)], ids=["conv64to64_256", "convT256to64_128"])
def test_the_step_shapes_follow_the_rule(monkeypatch, op, B, C, K, H):
    """VGG conv1_2 and netG's outermost up convolution at batch 8: what the size rule of wino_fused.hip (WF_MIN_TILES) says about
    them is what launch_winograd does under option 0, and option 1 / 2 override it either way."""
    tiles = B * (H // 4) ** 2
    admitted = tiles >= RULE_MIN_TILES
    _set(0)
    assert _workspace_written(monkeypatch, op, B, C, K, H, H) == (not admitted)
    _set(1)
    assert _workspace_written(monkeypatch, op, B, C, K, H, H)


def test_bf16_tensors_and_split_arithmetic_never_take_the_fused_kernel(monkeypatch):
    _set(2)
    assert _workspace_written(monkeypatch, "conv_fwd", 2, 32, 48, 16, 32, bf16=True)
    for math in ("bf16x3", "bf16x6"):
        assert _workspace_written(monkeypatch, "conv_fwd", 2, 32, 48, 16, 32, math=math)
    assert not _workspace_written(monkeypatch, "conv_fwd", 2, 32, 48, 16, 32)          # the same shape in fp32: fused
