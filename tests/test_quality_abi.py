"""The image-quality path (csrc/image_quality.hip: ipsr_image_quality, ipsr_image_quality_workspace_bytes; deepinpainting_amd/metrics.py)
without a GPU: header, exports and binding table, the workspace query on the shapes the entry refuses, the refusals that come before any
HIP call (on fake addresses, in a child process with every GPU hidden), the `IQA_pytorch` alias of INTEGRATION.md read from the file,
the known answers of the float64 restatement (tests/quality_ref.py), and the torch composite of `metrics.SSIM` against it.
Nothing here launches a kernel.
"""
import ctypes
import os
import re
import sys

import pytest
import torch

import quality_ref as R
from bf16x3_harness import ROOT, fake_pointers, lib, refused_calls  # noqa: F401  (fixtures by name)

IPSR_ERR_INVALID, IPSR_ERR_UNSUPPORTED, IPSR_ERR_WORKSPACE = -1, -2, -3
ENTRIES = ("ipsr_image_quality", "ipsr_image_quality_workspace_bytes")


def test_header_exports_and_bindings_carry_the_entries(lib):
    from deepinpainting_amd import _lib, ops
    header = open(os.path.join(ROOT, "include", "ipsr_hip.h")).read()
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for name in ENTRIES:
        assert re.search(r"\b%s\(" % name, header), name
        assert hasattr(raw, name), "libipsr_hip.so lacks %s" % name
        assert name in _lib.SIGNATURES and getattr(lib, name).argtypes == _lib.SIGNATURES[name][1]
    assert re.search(r"#define\s+IPSR_IQ_SSIM\s+1\b", header) and ops.IQ_SSIM == R.IQ_SSIM == 1
    assert lib.ipsr_abi_version() == _lib.ABI_VERSION
    assert "image_quality.hip" in open(os.path.join(ROOT, "deepinpainting_amd", "csrc", "Makefile")).read()


def test_workspace_query(lib):
    q = lib.ipsr_image_quality_workspace_bytes
    # the shapes the entry refuses: 0, with the reason
    assert q(1, 3, 10, 64, 1) == 0 and b"SSIM needs" in lib.ipsr_last_error()
    assert q(1, 3, 64, 10, 1) == 0 and b"SSIM needs" in lib.ipsr_last_error()
    for bad in ((0, 3, 64, 64), (1, 0, 64, 64), (1, 3, 0, 64), (1, 3, 64, -1)):
        assert q(*bad, 1) == 0 and b"bad size" in lib.ipsr_last_error()
    assert q(1, 3, 64, 64, 2) == 0 and b"flag" in lib.ipsr_last_error()
    assert q(65536, 3, 64, 64, 1) == 0 and b"grid overflow" in lib.ipsr_last_error()
    assert q(1, 3, 2 ** 20, 2 ** 20, 1) == 0 and b"grid overflow" in lib.ipsr_last_error()
    # without the SSIM bit any H, W >= 1 is taken
    assert q(2, 3, 10, 64, 0) == R.workspace_bytes(2, 3, 10, 64) == 2 * 3 * 2 * 24
    assert q(1, 1, 1, 1, 0) == 24
    # one fp64 triple per (image, channel, tile), the same with and without the bit
    T = R.T
    for B, C, H, W in ((1, 1, 11, 11), (1, 3, T + 10, T + 10), (3, 4, T + 11, T + 10), (1, 1, 2 * T + 15, T + 13), (16, 3, 256, 256)):
        assert q(B, C, H, W, 1) == q(B, C, H, W, 0) == R.workspace_bytes(B, C, H, W), (B, C, H, W)
    assert R.tiles(T + 10) == 1 and R.tiles(T + 11) == 2 and R.tiles(256) == 8


@pytest.fixture(scope="module")
def refusals(lib):
    p = fake_pointers([0] * 5)
    need = lib.ipsr_image_quality_workspace_bytes(2, 3, 64, 64, 1)
    assert need == R.workspace_bytes(2, 3, 64, 64)

    def call(x=p[0], y=p[1], shape=(2, 3, 64, 64), flags=1, win=p[2], out=p[3], ws=p[4], ws_bytes=need):
        return ("ipsr_image_quality", (x, y) + tuple(shape) + (flags, win, out, ws, ws_bytes, None))
    return refused_calls({
        "h10": call(shape=(2, 3, 10, 64)), "w10": call(shape=(2, 3, 64, 10)),
        "null_x": call(x=None), "null_y": call(y=None), "null_out": call(out=None), "null_ws": call(ws=None), "null_window": call(win=None),
        "b0": call(shape=(0, 3, 64, 64)), "c_neg": call(shape=(2, -3, 64, 64)), "flags": call(flags=3),
        "ws_short": call(ws_bytes=need - 1), "ws_odd": call(ws=p[4] + 4), "b_over": call(shape=(65536, 3, 64, 64), ws_bytes=1 << 40),
    })


@pytest.mark.parametrize("case,rc,msg", [
    ("h10", IPSR_ERR_UNSUPPORTED, "SSIM needs"), ("w10", IPSR_ERR_UNSUPPORTED, "SSIM needs"),
    ("null_x", IPSR_ERR_INVALID, "null pointer"), ("null_y", IPSR_ERR_INVALID, "null pointer"), ("null_out", IPSR_ERR_INVALID, "null pointer"),
    ("null_ws", IPSR_ERR_INVALID, "null pointer"), ("null_window", IPSR_ERR_INVALID, "null pointer"),
    ("b0", IPSR_ERR_INVALID, "bad size"), ("c_neg", IPSR_ERR_INVALID, "bad size"), ("flags", IPSR_ERR_INVALID, "flag"),
    ("ws_short", IPSR_ERR_WORKSPACE, "workspace"), ("ws_odd", IPSR_ERR_INVALID, "8-byte aligned"), ("b_over", IPSR_ERR_UNSUPPORTED, "grid overflow")])
def test_refused_before_any_hip_call(refusals, case, rc, msg):
    got, text = refusals[case]
    assert got == rc and msg in text, (got, text)


def test_ops_refuses_cpu_tensors(lib):
    from deepinpainting_amd import ops
    with pytest.raises(RuntimeError, match="CUDA/HIP tensor"):
        ops.image_quality(torch.zeros(1, 3, 16, 16), torch.zeros(1, 3, 16, 16))


def test_iqa_pytorch_resolves_through_the_alias_of_the_integration_guide(lib, monkeypatch):
    text = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    lines = [ln for ln in text.splitlines() if "IQA_pytorch" in ln and "sys.modules.setdefault" in ln]
    assert len(lines) == 1, lines
    monkeypatch.delitem(sys.modules, "IQA_pytorch", raising=False)
    try:
        import deepinpainting_amd
        import deepinpainting_amd.metrics
        exec(lines[0].strip(), {"sys": sys, "deepinpainting_amd": deepinpainting_amd})
        from IQA_pytorch import SSIM
        assert SSIM is deepinpainting_amd.metrics.SSIM
        assert isinstance(SSIM(channels=3), torch.nn.Module)
        # a real install wins: setdefault leaves a module that is already there
        sentinel = type(sys)("IQA_pytorch")
        sys.modules["IQA_pytorch"] = sentinel
        exec(lines[0].strip(), {"sys": sys, "deepinpainting_amd": deepinpainting_amd})
        assert sys.modules["IQA_pytorch"] is sentinel
    finally:
        sys.modules.pop("IQA_pytorch", None)


# ---- the restatement's known answers ---------------------------------------------------------------------------------------------------
def _textured(B, C, H, W, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.rand(B, C, H, W, generator=g) * 2 - 1, torch.rand(B, C, H, W, generator=g) * 2 - 1


def test_window_is_the_float32_gaussian():
    w = R.window()
    assert w.shape == (11, 11) and w.dtype.name == "float32"
    assert abs(float(w.astype("float64").sum()) - 1.0) < 1e-6 and (w == w.T).all() and (w == w[::-1, ::-1]).all()
    assert w[5, 5] == w.max() and abs(float(w[5, 5]) - 0.0707) < 1e-3
    from deepinpainting_amd import ops
    assert (ops.ssim_window() == w).all()


def test_known_answers_of_the_restatement():
    X, _ = _textured(2, 3, 24, 29, 1)
    assert float((R.ssim(X, X) - 1).abs().max()) < 1e-12
    assert float(R.ssim(X, -X).abs().max()) < 1e-12                  # s12 = -s1, 2 s1 >> C2: cs clamps to 0
    c = R.ssim(torch.full((1, 3, 16, 17), 0.25), torch.full((1, 3, 16, 17), -0.5))
    assert round(float(c), 5) == -0.79942                            # flat: cs = 1, (2 mu1 mu2 + C1) / (mu1^2 + mu2^2 + C1) = -0.2499 / 0.3126
    # (the float32 window sums to 1 + e, |e| ~ 1e-7: s = E[x^2](1 + e) - mu^2 (1 + e)^2 is ~0.06 e against C2 = 9e-4, so the closed
    #  form holds to ~1e-5, not to rounding)
    assert abs(float(c) - (-0.2499 / 0.3126)) < 1e-5
    q = R.quality(torch.zeros(1, 1, 11, 11), torch.full((1, 1, 11, 11), 0.5))
    assert float(q[0, 1]) == 0.25 and float(q[0, 2]) == 0.5
    assert float(R.psnr_of_mse(0.04)) == pytest.approx(20.0, abs=1e-12) and float(R.psnr_of_mse(4.0)) == 0.0
    assert float(R.psnr_of_mse(0.0)) == 100.0


def test_psnr_of_the_module_on_cpu_tensors(lib):
    from deepinpainting_amd import metrics
    real = torch.zeros(2, 3, 12, 12)
    fake = torch.zeros(2, 3, 12, 12)
    fake[1] = 0.25                                                    # mse 1/16 -> 10 log10(64)
    p = metrics.psnr(real, fake)
    assert p.shape == (2,) and float(p[0]) == 100.0 and float(p[1]) == pytest.approx(10 * 1.806179973983887, abs=1e-5)
    assert float(metrics.psnr(real, fake, peak=1.0)[1]) == pytest.approx(10 * 1.2041199826559248, abs=1e-5)


def test_cpu_composite_equals_the_restatement(lib):
    from deepinpainting_amd import metrics
    X, Y = _textured(2, 3, 40, 37, 2)
    Y = 0.6 * X + 0.4 * Y
    want = R.ssim(X, Y)
    mod = metrics.SSIM(channels=3)
    got = mod(X, Y, as_loss=False)
    assert got.shape == (2,) and got.dtype == torch.float32 and not got.requires_grad
    assert float((got.double() - want).abs().max()) <= 1e-6
    got64 = mod(X.double(), Y.double(), as_loss=False)
    assert float((got64.double() - want).abs().max()) <= 1e-6
    with pytest.raises(NotImplementedError):
        mod(X[:, :, :10], Y[:, :, :10], as_loss=False)


def test_as_loss_backpropagates(lib):
    from deepinpainting_amd import metrics
    X, Y = _textured(2, 3, 20, 23, 3)
    X.requires_grad_(True)
    loss = metrics.SSIM(channels=3)(X, Y)                             # as_loss=True is the default, as in IQA_pytorch
    assert loss.dim() == 0 and loss.requires_grad
    assert float((loss.detach().double() - (1 - R.ssim(X, Y).mean())).abs()) <= 1e-6
    loss.backward()
    assert X.grad is not None and torch.isfinite(X.grad).all() and float(X.grad.abs().max()) > 0


def test_evaluator_keeps_the_host_out_of_update():
    """Structure only (the numbers are checked on the GPU): `update` and `step` hold no .item() / .cpu() / float(); `result` has the one read."""
    import inspect
    from deepinpainting_amd import metrics
    for fn in (metrics.Evaluator.update, metrics.Evaluator.step):
        src = inspect.getsource(fn)
        assert ".item(" not in src and ".cpu(" not in src and "float(" not in src and ".numpy(" not in src
    assert inspect.getsource(metrics.Evaluator.result).count(".cpu()") == 1
