"""Per-sample masks through the batched entries: ipsr_mask_index (mask batch -> feature masks, flags, ordered index, counts in one
launch), innercos_loss_masks / innercos_loss_backward_masks (one mask per sample), and the modules routed through them.

References: the committed fixtures of tests/golden/masks.npz; the existing one-mask entries (ipsr_feat_mask + ipsr_index_prep,
innercos_loss + innercos_loss_backward), row by row, bit for bit where the arithmetic is the same; an fp64 sum of the fp32 terms.
"""
import contextlib
import io
import os

import numpy as np
import pytest
import torch

import golden_cases

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
GROUPS = {"64": ("center64", "edge64", "empty64", "full64"), "256": ("center256", "center256_overlap4", "stroke256_a", "stroke256_b")}
COUNTS_AT_0_3125 = {"64": (16, 24, 0, 64), "256": (256, 252, 300, 556)}
DENSITIES = (0.0, 0.3, 0.4, 0.55, 1.0)
SIZES = ((67, 73, 1), (130, 136, 2), (256, 256, 3), (96, 102, 4), (512, 512, 3), (40, 56, 3),
         # rows of whole 16-byte vectors take another path in levels 1 and 2 (256 and 512 above do, in both): level 1 alone, both
         # levels on a non-square mask, and both with the levels in the workspace instead of LDS
         (80, 48, 3), (70, 96, 4), (640, 608, 3))
INDEX_FORMS = ((1, 1, 1), (3, 1, 4), (2, 2, 1))         # (patch, stride, mask_thred)
THRESHOLDS = (0.1, 5 / 16.0, 0.7)


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    torch.cuda.set_device(0)
    from deepinpainting_amd import ops as _ops
    return _ops


def quiet(fn, *a, **k):
    with contextlib.redirect_stdout(io.StringIO()):
        return fn(*a, **k)


# ------------------------------------------------------------------------------------------ ipsr_mask_index
@pytest.mark.parametrize("thr", ["0.3125", "0.5"])
@pytest.mark.parametrize("group", sorted(GROUPS))
def test_mask_index_vs_golden(ops, group, thr):
    d = np.load(os.path.join(GOLDEN, "masks.npz"))
    tags = ["%s__thr%s" % (name, thr) for name in GROUPS[group]]
    masks = torch.from_numpy(np.stack([d[t + "__mask"] for t in tags])).cuda()
    feat, flag, mpi, counts = ops.mask_index(masks, 3, float(thr), 1, 1, 1)
    feat, flag, mpi, counts = feat.cpu().numpy(), flag.cpu().numpy(), mpi.cpu().numpy(), counts.cpu().numpy()
    assert flag.dtype == mpi.dtype == counts.dtype == np.int32 and feat.dtype == np.uint8
    if thr == "0.3125":
        assert tuple(counts) == COUNTS_AT_0_3125[group]            # an empty and a full row are among them
    for r, t in enumerate(tags):
        M = len(d[t + "__mask_point_idx"])
        assert counts[r] == M, t
        np.testing.assert_array_equal(feat[r], d[t + "__feat"], err_msg=t)
        np.testing.assert_array_equal(flag[r], d[t + "__flag"], err_msg=t)
        np.testing.assert_array_equal(mpi[r, :M], d[t + "__mask_point_idx"], err_msg=t)
        assert (mpi[r, M:] == -1).all(), t


@pytest.mark.parametrize("H,W,layers", SIZES)
def test_mask_index_equals_the_one_mask_entries(ops, H, W, layers):
    """R = 5 Bernoulli masks of densities 0 .. 1 (rows of different lengths, an empty and a full one side by side), every threshold
    and index form: each row bit for bit what ipsr_feat_mask followed by ipsr_index_prep gives; R = 1; layers = 0 on the feature masks."""
    rs = np.random.RandomState(H)
    masks = torch.from_numpy(np.stack([(rs.rand(H, W) < p).astype(np.uint8) for p in DENSITIES])).cuda()
    for thr in THRESHOLDS:
        want_feat = torch.stack([ops.feat_mask(m, layers, thr) for m in masks])
        for patch, stride, thred in INDEX_FORMS:
            want = [ops.index_prep(f, patch, stride, thred) for f in want_feat]
            w_flag, w_mpi, w_cnt = torch.stack([o[0] for o in want]), torch.stack([o[1] for o in want]), torch.cat([o[2] for o in want])
            feat, flag, mpi, counts = ops.mask_index(masks, layers, thr, patch, stride, thred)
            tag = (H, W, layers, thr, patch, stride, thred)
            assert torch.equal(feat, want_feat) and torch.equal(flag, w_flag) and torch.equal(counts, w_cnt), tag
            assert torch.equal(mpi, w_mpi), tag                      # the -1 tail included
            if thr == THRESHOLDS[1] and patch == 1:
                c = counts.tolist()
                assert c[0] == 0 and c[4] == flag.size(1) and 0 < c[1] < c[4], c     # empty, full and mid-length rows
            # layers == 0: the feature masks go in, only the index part runs
            none, flag0, mpi0, counts0 = ops.mask_index(want_feat, 0, 0.0, patch, stride, thred)
            assert none is None and torch.equal(flag0, w_flag) and torch.equal(mpi0, w_mpi) and torch.equal(counts0, w_cnt), tag
        # R = 1, as a 2-D mask
        f1, g1, m1, c1 = ops.mask_index(masks[1], layers, thr, 1, 1, 1)
        one = ops.index_prep(want_feat[1], 1, 1, 1)
        assert torch.equal(f1[0], want_feat[1]) and torch.equal(g1[0], one[0]) and torch.equal(m1[0], one[1]) and torch.equal(c1, one[2])
        assert (H, W, layers) != (67, 73, 1) or g1.size(1) == 33 * 36 == 1188            # two 1024-chunks of the compaction


def test_mask_index_bool_masks_and_determinism(ops):
    """A bool batch is the same as its bytes; two calls give the same bits whatever the scratch held in between."""
    g = torch.Generator().manual_seed(3)
    masks = (torch.rand(3, 100, 140, generator=g) < 0.4).cuda()
    a = ops.mask_index(masks, 3, 5 / 16.0, 1, 1, 1)
    ops._workspace(1 << 20, masks.device).fill_(0xA5)
    b = ops.mask_index(masks.to(torch.uint8), 3, 5 / 16.0, 1, 1, 1)
    assert all(torch.equal(x, y) for x, y in zip(a, b))
    # any non-zero byte is a masked pixel, as in ipsr_feat_mask (here through the 16-byte loads: 144 % 16 == 0)
    vals = torch.tensor([0, 1, 2, 16, 128, 255, 0, 0], dtype=torch.uint8)
    raw = vals[torch.randint(0, 8, (2, 96, 144), generator=g)].cuda()
    feat = ops.mask_index(raw, 3, 5 / 16.0, 1, 1, 1)[0]
    assert torch.equal(feat, torch.stack([ops.feat_mask(m, 3, 5 / 16.0) for m in raw])) and 0 < int(feat.sum()) < feat.numel()
    assert torch.equal(feat, ops.mask_index(raw != 0, 3, 5 / 16.0, 1, 1, 1)[0])


# ------------------------------------------------------------------------------------------ InnerCos, one mask per sample
IC_SHAPES = ((3, 8, 8, 5, 7),              # N = 35: the scalar path
             (2, 11, 8, 8, 8),             # the vector path, Cx > Cuse
             (5, 1023, 1023, 4, 4),        # 5115 rows: two rows per workgroup, a workgroup astride every sample boundary
             (5, 1023, 1023, 3, 5),        # the same rows on the scalar path (N = 15)
             (4, 64, 64, 32, 32),
             (2, 1024, 512, 32, 32))
STRENGTH = 0.7


def _ic_inputs(shape):
    B, Cx, Cuse, h, w = shape
    g = torch.Generator(device="cuda").manual_seed(B * 1000 + Cx + h)
    x = torch.randn(B, Cx, h, w, device="cuda", generator=g)
    t = torch.rand(B, Cuse, h, w, device="cuda", generator=g)
    rows = [(torch.rand(h, w, device="cuda", generator=g) < 0.4).float(), torch.ones(h, w, device="cuda"), torch.zeros(h, w, device="cuda"),
            (torch.rand(h, w, device="cuda", generator=g) < 0.7).float(), (torch.rand(h, w, device="cuda", generator=g) < 0.2).float()]
    return x, t, torch.stack(rows[:B])          # B >= 3: an all-one and an all-zero row among them


@pytest.mark.parametrize("shape", IC_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_innercos_masks_loss_and_gradient(ops, shape):
    B, Cx, Cuse, h, w = shape
    x, t, m = _ic_inputs(shape)
    loss = ops.innercos_loss(x, Cuse, m, t, STRENGTH)
    # against the mean of the B batch-of-one calls of the existing entry
    # (the samples as tensors of their own: the one-mask entries want 16-byte aligned operands, which row b of an odd-N batch is not)
    xs, ts, ms = [x[b:b + 1].clone() for b in range(B)], [t[b:b + 1].clone() for b in range(B)], [m[b].clone() for b in range(B)]
    per = [ops.innercos_loss(xs[b], Cuse, ms[b], ts[b], STRENGTH) for b in range(B)]
    want = float(torch.stack(per).double().mean())
    # against an fp64 sum of the fp32 terms
    d = (x[:, :Cuse] * m[:, None]) * STRENGTH - t
    want64 = float((d * d).double().sum() / d.numel())
    got = float(loss)
    print("innercos_masks %s: loss %.9g, per-sample mean %.9g (rel %.2e), fp64 %.9g (rel %.2e)"
          % (shape, got, want, abs(got - want) / want, want64, abs(got - want64) / want64))
    assert loss.dtype == torch.float32 and loss.dim() == 0
    assert abs(got - want) <= 1e-6 * abs(want) and abs(got - want64) <= 1e-6 * abs(want64)
    # gradient against the B batch-of-one calls of the existing backward, each fed grad_loss / B
    gl = torch.tensor([1.3], device="cuda")
    gx = ops.innercos_loss_backward(x, Cuse, m, t, STRENGTH, gl)
    ref = torch.cat([ops.innercos_loss_backward(xs[b], Cuse, ms[b], ts[b], STRENGTH, gl / B) for b in range(B)], 0)
    assert gx.shape == x.shape
    if B in (2, 4):
        assert torch.equal(gx, ref)              # both routes scale by the same power of two
    else:
        torch.testing.assert_close(gx, ref, rtol=1e-6, atol=0)
    assert Cx == Cuse or float(gx[:, Cuse:].abs().max()) == 0.0
    assert float(gx[:, :Cuse].abs().max()) > 0.0


@pytest.mark.parametrize("shape", IC_SHAPES[:2], ids=lambda s: "x".join(map(str, s)))
def test_innercos_masks_with_a_shared_mask_is_the_existing_entry(ops, shape):
    """mask_bstride = 0 through the new entries: the existing entries, bit for bit."""
    from deepinpainting_amd import _lib
    B, Cx, Cuse, h, w = shape
    N = h * w
    x, t, m = _ic_inputs(shape)
    m0 = m[0].contiguous()
    gl = torch.tensor([1.3], device="cuda")
    L = _lib.lib()
    ws = ops._workspace(L.innercos_workspace_bytes(B, Cuse, N), x.device)
    loss, gx = torch.empty((), device="cuda"), torch.empty_like(x)
    st = ops._stream()
    _lib.check(L.innercos_loss_masks(x.data_ptr(), B, Cx, Cuse, N, m0.data_ptr(), 0, t.data_ptr(), STRENGTH, loss.data_ptr(), ws.data_ptr(),
                                     ws.numel(), st), "innercos_loss_masks")
    _lib.check(L.innercos_loss_backward_masks(x.data_ptr(), B, Cx, Cuse, N, m0.data_ptr(), 0, t.data_ptr(), STRENGTH, gl.data_ptr(),
                                              gx.data_ptr(), st), "innercos_loss_backward_masks")
    assert torch.equal(loss, ops.innercos_loss(x, Cuse, m0, t, STRENGTH))
    assert torch.equal(gx, ops.innercos_loss_backward(x, Cuse, m0, t, STRENGTH, gl))
    # and the B*N form with B equal rows computes that loss too (other tree only where rows share a workgroup: not at these sizes)
    assert torch.equal(ops.innercos_loss(x, Cuse, m0.expand(B, h, w).contiguous(), t, STRENGTH), loss)


# ------------------------------------------------------------------------------------------ the modules
@pytest.fixture
def switch():
    from deepinpainting_amd.models.IPSR_model import IPSR_model
    was = IPSR_model.batched_masks
    yield IPSR_model
    IPSR_model.batched_masks = was


def _module_pass(on, masks, x, ref, dy, x2, tgt):
    from deepinpainting_amd.models.IPSR_model import IPSR_model, _Ref
    from deepinpainting_amd.models.InnerCos import InnerCos
    from deepinpainting_amd.models.InnerCos2 import InnerCos2
    from deepinpainting_amd.options import Option
    IPSR_model.batched_masks = on
    opt = Option(gpu_ids=[0])
    layer = IPSR_model(opt.threshold, 1, 1, 1, 1, 0.5)
    feat = layer.set_mask(masks, 3, opt.threshold)
    layer.set_ref(_Ref(ref))
    xa = x.clone().requires_grad_(True)
    y = layer(xa)
    (gx,) = torch.autograd.grad(y, xa, dy)
    res = dict(feat=feat, flag=layer._flag32, mpi=layer._mpi32, counts=layer._counts, y=y.detach(), gx=gx)
    for name, cls, inp in (("ic", InnerCos, x), ("ic2", InnerCos2, x2)):
        tap = cls(strength=0.7)
        tap.set_mask(masks, opt)
        tap.set_target(tgt if cls is InnerCos2 else tgt[:, :x.size(1)])
        xin = inp.clone().requires_grad_(True)
        assert tap(xin) is xin
        res[name + "_loss"] = tap.backward().detach()
        res[name + "_grad"] = xin.grad
    return res


def test_modules_switch_on_equals_switch_off(ops, switch):
    from deepinpainting_amd.util.staging import random_stroke_mask
    B, C, h = 3, 64, 16
    g = torch.Generator(device="cuda").manual_seed(21)
    x = torch.randn(B, C, h, h, device="cuda", generator=g).abs()
    ref = torch.rand(B, C, h, h, device="cuda", generator=g)
    dy = torch.randn(B, C, h, h, device="cuda", generator=g)
    x2 = torch.randn(B, 1024, h, h, device="cuda", generator=g)
    tgt = torch.rand(B, 512, h, h, device="cuda", generator=g)
    masks = torch.cat([random_stroke_mask(128, torch.Generator().manual_seed(40 + b), width=(8, 24)) for b in range(B)], 0).cuda()
    on = _module_pass(True, masks, x, ref, dy, x2, tgt)
    off = _module_pass(False, masks, x, ref, dy, x2, tgt)
    assert on["feat"].shape == (B, h, h) and len({int(f.sum()) for f in on["feat"]}) > 1          # different hole sizes
    for k in ("feat", "flag", "mpi", "counts", "y", "gx"):
        assert on[k].dtype == off[k].dtype and torch.equal(on[k], off[k]), k
    for k in ("ic_loss", "ic2_loss", "ic_grad", "ic2_grad"):
        torch.testing.assert_close(on[k], off[k], rtol=1e-6, atol=0)
    assert float(on["ic2_grad"][:, 512:].abs().max()) == 0.0 and float(on["ic_grad"].abs().max()) > 0.0


COUNTED = ("ipsr_mask_index", "ipsr_feat_mask", "ipsr_index_prep", "innercos_loss", "innercos_loss_masks", "innercos_loss_backward",
           "innercos_loss_backward_masks")


@pytest.fixture
def calls(monkeypatch):
    """Library calls counted by name, through wrappers on the handle every front-end calls through."""
    from deepinpainting_amd import _lib
    L = _lib.lib()
    seen = {name: 0 for name in COUNTED}
    for name in COUNTED:
        def wrapper(*a, _fn=getattr(L, name), _name=name):
            seen[_name] += 1
            return _fn(*a)
        monkeypatch.setattr(L, name, wrapper)
    return seen


def test_call_counts_of_a_training_step(ops, switch, calls, tmp_path):
    from deepinpainting_amd.models.models import create_model
    from deepinpainting_amd.options import Option
    from deepinpainting_amd.util.staging import random_stroke_mask
    B = 3
    assert switch.batched_masks is True
    opt = Option(gpu_ids=[0], batchSize=B, use_dropout=False, quiet=True, checkpoints_dir=str(tmp_path))
    m = quiet(create_model, opt)
    img, one_mask, refimg = golden_cases.trainer_inputs(B=B)
    img, refimg = img.cuda(), refimg.cuda()
    big = torch.cat([random_stroke_mask(256, torch.Generator().manual_seed(60 + b)) for b in range(B)], 0)

    def reset():
        for k in calls:
            calls[k] = 0

    def nonzero():
        return {k: v for k, v in calls.items() if v}

    # per-sample masks: one call for feature masks + index, one per tap; two whole steps
    for step in range(2):
        reset()
        m.set_input(img, big.cuda(), refimg)
        assert nonzero() == {"ipsr_mask_index": 1}, nonzero()
        m.set_ref_latent()
        m.set_gt_latent()
        reset()
        m.optimize_parameters()
        assert nonzero() == {"innercos_loss_masks": 2}, nonzero()
    assert all(np.isfinite(v) for v in m.get_current_errors().values())
    for b in range(B):
        assert float(m.real_A[b][:, big[b, 0]].abs().max()) == 0.0
    # one mask for the batch: today's calls, none of the new entries
    reset()
    m.set_input(img, one_mask.cuda(), refimg)
    m.set_ref_latent()
    m.set_gt_latent()
    m.optimize_parameters()
    assert nonzero() == {"ipsr_feat_mask": 1, "ipsr_index_prep": 1, "innercos_loss": 2}, nonzero()
    assert all(np.isfinite(v) for v in m.get_current_errors().values())
