"""The fused loss heads (csrc/loss_head.hip: ipsr_ragan_loss, ipsr_l1_pair_loss, ipsr_loss_grad_scale) without a GPU: header, exports and
binding table, the refusals that come before any HIP call, the switch that selects the route, and the PyTorch route of CPU tensors, which
must give today's bits.  Nothing here launches a kernel; the calls on fake addresses run in a child process with every GPU hidden.
"""
import os
import re
import types

import pytest
import torch

from bf16x3_harness import ROOT, fake_pointers, lib, refused_calls  # noqa: F401  (fixtures by name)

IPSR_ERR_INVALID, IPSR_ERR_WORKSPACE = -1, -3
ENTRIES = ("ipsr_ragan_loss", "ipsr_l1_pair_loss_workspace_bytes", "ipsr_l1_pair_loss", "ipsr_loss_grad_scale")


def test_header_exports_and_bindings_carry_the_entries(lib):
    from deepinpainting_amd import _lib
    header = open(os.path.join(ROOT, "include", "ipsr_hip.h")).read()
    for name in ENTRIES:
        assert re.search(r"\b%s\(" % name, header), name
        assert name in _lib.SIGNATURES and getattr(lib, name).argtypes == _lib.SIGNATURES[name][1]
    assert lib.ipsr_abi_version() == 15
    assert "loss_head.hip" in open(os.path.join(ROOT, "deepinpainting_amd", "csrc", "Makefile")).read()


def test_workspace_query(lib):
    assert lib.ipsr_l1_pair_loss_workspace_bytes(0) == 0 and b"bad size" in lib.ipsr_last_error()
    assert lib.ipsr_l1_pair_loss_workspace_bytes(-5) == 0
    assert lib.ipsr_l1_pair_loss_workspace_bytes(1) == 8                       # one workgroup, one fp64 partial
    sizes = [lib.ipsr_l1_pair_loss_workspace_bytes(n) for n in (1, 2048, 2049, 8 * 3 * 256 * 256, 2 ** 31 - 1)]
    assert sizes == sorted(sizes) and sizes[2] == 16 and sizes[-1] == 8 * 1024  # grows with n up to 1024 workgroups


@pytest.fixture(scope="module")
def refusals(lib):
    p = fake_pointers([0] * 6)
    need = lib.ipsr_l1_pair_loss_workspace_bytes(5000)
    assert need == 8 * 3
    calls = {
        "ragan_null_fake": ("ipsr_ragan_loss", (None, 4, p[1], 4, 1.0, p[2], p[3], p[4], None)),
        "ragan_null_real": ("ipsr_ragan_loss", (p[0], 4, None, 4, 1.0, p[2], p[3], p[4], None)),
        "ragan_null_loss": ("ipsr_ragan_loss", (p[0], 4, p[1], 4, 1.0, None, p[3], p[4], None)),
        "ragan_n_fake_0": ("ipsr_ragan_loss", (p[0], 0, p[1], 4, 1.0, p[2], None, None, None)),
        "ragan_n_real_neg": ("ipsr_ragan_loss", (p[0], 4, p[1], -1, 1.0, p[2], None, None, None)),
        "l1_null_a1": ("ipsr_l1_pair_loss", (None, p[1], p[2], 5000, 1.0, p[3], None, None, p[4], need, None)),
        "l1_null_a2": ("ipsr_l1_pair_loss", (p[0], None, p[2], 5000, 1.0, p[3], None, None, p[4], need, None)),
        "l1_null_t": ("ipsr_l1_pair_loss", (p[0], p[1], None, 5000, 1.0, p[3], None, None, p[4], need, None)),
        "l1_null_loss": ("ipsr_l1_pair_loss", (p[0], p[1], p[2], 5000, 1.0, None, None, None, p[4], need, None)),
        "l1_null_ws": ("ipsr_l1_pair_loss", (p[0], p[1], p[2], 5000, 1.0, p[3], None, None, None, need, None)),
        "l1_n_0": ("ipsr_l1_pair_loss", (p[0], p[1], p[2], 0, 1.0, p[3], None, None, p[4], need, None)),
        "l1_ws_short": ("ipsr_l1_pair_loss", (p[0], p[1], p[2], 5000, 1.0, p[3], None, None, p[4], need - 1, None)),
        "l1_ws_odd": ("ipsr_l1_pair_loss", (p[0], p[1], p[2], 5000, 1.0, p[3], None, None, p[4] + 4, need, None)),
        "scale_null_scalar": ("ipsr_loss_grad_scale", (None, p[1], p[2], 4, None, None, 0, None)),
        "scale_null_g1": ("ipsr_loss_grad_scale", (p[0], None, p[2], 4, None, None, 0, None)),
        "scale_null_out1": ("ipsr_loss_grad_scale", (p[0], p[1], None, 4, None, None, 0, None)),
        "scale_null_g2": ("ipsr_loss_grad_scale", (p[0], p[1], p[2], 4, None, p[4], 4, None)),
        "scale_null_out2": ("ipsr_loss_grad_scale", (p[0], p[1], p[2], 4, p[3], None, 4, None)),
        "scale_n1_0": ("ipsr_loss_grad_scale", (p[0], p[1], p[2], 0, None, None, 0, None)),
        "scale_n2_neg": ("ipsr_loss_grad_scale", (p[0], p[1], p[2], 4, p[3], p[4], -2, None)),
    }
    return refused_calls(calls)


@pytest.mark.parametrize("case,rc,msg", [
    ("ragan_null_fake", IPSR_ERR_INVALID, "null pointer"), ("ragan_null_real", IPSR_ERR_INVALID, "null pointer"),
    ("ragan_null_loss", IPSR_ERR_INVALID, "null pointer"), ("ragan_n_fake_0", IPSR_ERR_INVALID, "bad size"),
    ("ragan_n_real_neg", IPSR_ERR_INVALID, "bad size"),
    ("l1_null_a1", IPSR_ERR_INVALID, "null pointer"), ("l1_null_a2", IPSR_ERR_INVALID, "null pointer"), ("l1_null_t", IPSR_ERR_INVALID, "null pointer"),
    ("l1_null_loss", IPSR_ERR_INVALID, "null pointer"), ("l1_null_ws", IPSR_ERR_INVALID, "null pointer"), ("l1_n_0", IPSR_ERR_INVALID, "bad size"),
    ("l1_ws_short", IPSR_ERR_WORKSPACE, "workspace"), ("l1_ws_odd", IPSR_ERR_INVALID, "8-byte aligned"),
    ("scale_null_scalar", IPSR_ERR_INVALID, "null pointer"), ("scale_null_g1", IPSR_ERR_INVALID, "null pointer"),
    ("scale_null_out1", IPSR_ERR_INVALID, "null pointer"), ("scale_null_g2", IPSR_ERR_INVALID, "null pointer"),
    ("scale_null_out2", IPSR_ERR_INVALID, "null pointer"), ("scale_n1_0", IPSR_ERR_INVALID, "bad size"), ("scale_n2_neg", IPSR_ERR_INVALID, "bad size")])
def test_refused_before_any_hip_call(refusals, case, rc, msg):
    got, text = refusals[case]
    assert got == rc and msg in text, (got, text)


# ---- the switch ------------------------------------------------------------------------------------------------------------------------
@pytest.fixture
def networks(lib, monkeypatch):
    from deepinpainting_amd.models import networks as nw
    monkeypatch.delenv("IPSR_NO_FUSED_LOSS", raising=False)
    nw.set_fused_losses(None)
    yield nw
    nw.set_fused_losses(None)


def test_switch_and_environment(networks, monkeypatch):
    nw = networks
    assert nw.fused_losses() is True                                   # the default
    nw.set_fused_losses(False)
    assert nw.fused_losses() is False
    nw.set_fused_losses(True)
    assert nw.fused_losses() is True
    monkeypatch.setenv("IPSR_NO_FUSED_LOSS", "1")
    assert nw.fused_losses() is True                                   # an explicit setting holds; the environment is read once
    nw.set_fused_losses(None)
    assert nw.fused_losses() is False
    monkeypatch.setenv("IPSR_NO_FUSED_LOSS", "0")
    assert nw.fused_losses() is False                                  # read once
    nw.set_fused_losses(None)
    assert nw.fused_losses() is True


def _stub(cuda=True, dtype=torch.float32, contiguous=True, index=0, shape=(2, 1, 3, 3), requires_grad=False):
    n = 1
    for s in shape:
        n *= s
    return types.SimpleNamespace(is_cuda=cuda, dtype=dtype, is_contiguous=lambda: contiguous, numel=lambda: n, shape=torch.Size(shape),
                                 device=types.SimpleNamespace(index=index), requires_grad=requires_grad, size=lambda d: shape[d])


def test_the_route_is_taken_by_cuda_fp32_contiguous_tensors_only(networks, monkeypatch):
    nw = networks
    monkeypatch.setattr(torch._C, "_cuda_getDevice", lambda: 0)
    assert nw._fused_route(_stub(), _stub())
    assert not nw._fused_route(_stub(), _stub(cuda=False))
    assert not nw._fused_route(_stub(dtype=torch.bfloat16), _stub())
    assert not nw._fused_route(_stub(), _stub(contiguous=False))
    assert not nw._fused_route(_stub(index=1))                         # another GPU than the current one
    assert not nw._fused_route(_stub(shape=(0, 1, 3, 3)))
    with monkeypatch.context() as m:
        m.setattr(nw._lib, "LIB_PATH", os.path.join(ROOT, "no_such_library.so"))
        assert not nw._fused_route(_stub(), _stub())                   # no library: the PyTorch expression
    assert nw._fused_route(_stub(), _stub())
    nw.set_fused_losses(False)
    assert not nw._fused_route(_stub(), _stub())
    monkeypatch.setenv("IPSR_NO_FUSED_LOSS", "1")
    nw.set_fused_losses(None)
    assert not nw._fused_route(_stub(), _stub())


def test_ganloss_and_l1_pair_dispatch_on_the_route(networks, monkeypatch):
    nw = networks
    monkeypatch.setattr(torch._C, "_cuda_getDevice", lambda: 0)
    calls = []

    def recorder(tag):
        return types.SimpleNamespace(apply=lambda *a: calls.append((tag,) + a[-1:]) or tag)
    monkeypatch.setattr(nw, "_RaGANLoss", recorder("ragan"))
    monkeypatch.setattr(nw, "_RaGANLossBatched", recorder("batched"))
    monkeypatch.setattr(nw, "_L1PairLoss", recorder("l1"))
    gl = nw.GANLoss(gan_type="lsgan")
    assert gl(_stub(), _stub(), True) == "ragan" and gl(_stub(), _stub(), False) == "ragan"
    assert calls == [("ragan", 1.0), ("ragan", -1.0)]                  # s = sign * label, the label 1.0 for both target kinds
    with torch.enable_grad():
        assert gl.batched(_stub(shape=(4, 1, 3, 3), requires_grad=True), 2, True) == "batched"
    assert calls[-1] == ("batched", 1.0)
    a, t = _stub(shape=(2, 3, 4, 4), requires_grad=True), _stub(shape=(2, 3, 4, 4))
    assert nw.l1_pair_loss(a, a, t, 100.0, torch.nn.L1Loss()) == "l1" and calls[-1] == ("l1", 100.0)
    assert nw.l1_pair_loss(a, a, t, 100.0) == "l1"
    # off: the Functions are not reached (the PyTorch expression fails on the stubs, which is the point)
    nw.set_fused_losses(False)
    n = len(calls)
    with pytest.raises((TypeError, AttributeError)):
        gl(_stub(), _stub(), True)
    with pytest.raises((TypeError, AttributeError)):
        nw.l1_pair_loss(a, a, t, 100.0)
    assert len(calls) == n
    # another criterion than the mean L1 keeps the expression too
    nw.set_fused_losses(True)
    with pytest.raises((TypeError, AttributeError)):
        nw.l1_pair_loss(a, a, t, 100.0, torch.nn.L1Loss(reduction="sum"))
    assert len(calls) == n


# ---- CPU tensors: today's expressions, bit for bit ---------------------------------------------------------------------------------------
def _today_gan(fake, real, sign):
    t = torch.full(fake.size(), 1.0, dtype=fake.dtype)
    a = torch.mean((real - torch.mean(fake) - sign * t) ** 2)
    b = torch.mean((fake - torch.mean(real) + sign * t) ** 2)
    return (a + b) / 2


@pytest.mark.parametrize("on", [True, False])
def test_cpu_tensors_take_the_pytorch_route_bit_for_bit(networks, on):
    nw = networks
    nw.set_fused_losses(on)
    g = torch.Generator().manual_seed(5)
    gl = nw.GANLoss(gan_type="lsgan")
    for is_real, sign in ((True, 1.0), (False, -1.0)):
        fake = torch.randn(4, 1, 30, 30, generator=g, requires_grad=True)
        real = torch.randn(4, 1, 30, 30, generator=g, requires_grad=True)
        got = gl(fake, real, is_real)
        gf, gr = torch.autograd.grad(got, (fake, real))
        want = _today_gan(fake, real, sign)
        wf, wr = torch.autograd.grad(want, (fake, real))
        assert torch.equal(got, want) and torch.equal(gf, wf) and torch.equal(gr, wr)
        both = torch.cat((fake, real), 0).detach().requires_grad_(True)
        got_b = gl.batched(both, 4, is_real)
        assert torch.equal(got_b, want) and torch.equal(torch.autograd.grad(got_b, both)[0], torch.cat((wf, wr), 0))
    a1 = torch.randn(2, 3, 16, 16, generator=g, requires_grad=True)
    a2 = torch.randn(2, 3, 16, 16, generator=g, requires_grad=True)
    t = torch.randn(2, 3, 16, 16, generator=g)
    crit = torch.nn.L1Loss()
    got = nw.l1_pair_loss(a1, a2, t, 100.0, crit)
    want = (crit(a1, t) + crit(a2, t)) * 100.0
    assert torch.equal(got, want)
    assert all(torch.equal(x, y) for x, y in zip(torch.autograd.grad(got, (a1, a2)), torch.autograd.grad(want, (a1, a2))))


def test_the_trainer_uses_the_heads():
    src = open(os.path.join(ROOT, "deepinpainting_amd", "models", "IPSR.py")).read()
    assert src.count("networks.l1_pair_loss(self.fake_B, self.fake_P, self.real_B, self.opt.lambda_A, self.criterionL1)") == 2
    assert "self.criterionGAN.batched(both, nb, True)" in src and "self.criterionGAN.batched(both_F, nb, True)" in src
