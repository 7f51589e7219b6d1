"""What the tests of the direct split-bf16 family share (tests/test_gpu_bf16x3*.py on the GPU, tests/test_bf16x3*_abi.py without one): bit
comparison, the operand draw, the band check, the checks every front-end gets after its first result, the module-level fixtures, and the
child process that calls entries on fake addresses with every GPU hidden.  A plain module: the test files import what they need by name,
fixtures included.  The cases, bands and recorded tables stay in the test files and the *_plan.py modules.
"""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAN_BITS = 0x7FC00DAD                   # a NaN no kernel produces: what refused calls and out='s neighbours must leave in place


def _bits(t):
    import torch
    return t.contiguous().view(torch.int32)


def _same(a, b):
    import torch
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(_bits(a), _bits(b))


def draw(g, shape, dim):
    """Normal draws times a power of two in 2^-6 .. 2^6 per index of `dim` (the channel of an activation, the first dimension of a weight):
    not bf16-representable, wide range, far from subnormals."""
    import torch
    t = torch.randn(shape, device="cuda", generator=g)
    per = [shape[dim] if i == dim else 1 for i in range(len(shape))]
    return t * torch.exp2(torch.randint(-6, 7, per, device="cuda", generator=g).float())


def _in_band(tag, y, y64, band, ref="y64"):
    import torch
    err = (y.double() - y64).abs()
    worst = float((err / band).max())
    print("%s: max |err| / band %.3f, max |err| / max|%s| %.2e" % (tag, worst, ref, float(err.max() / y64.abs().max())))
    assert torch.isfinite(y).all() and worst <= 1.0, (tag, worst)


def check_guarded(monkeypatch, run, operands, names, result, ws_bytes, tag):
    """run(*operands) again between guard bands, on a NaN-filled workspace of exactly the size asked for: the same bits, no input written."""
    import torch
    from guarded import Arena
    keep = [t.clone() for t in operands]
    arena = Arena(ws_fill="nan")
    guarded = [arena.guarded_copy(t, n) for t, n in zip(operands, names)]
    with arena.installed(monkeypatch):
        got = run(*guarded)
    torch.cuda.synchronize()
    arena.check_guards()
    assert all(_same(g, k) and _same(t, k) for g, t, k in zip(guarded, operands, keep)), "an input was modified"
    assert _same(got, result), "%s: the guarded run differs" % tag
    assert arena.workspaces and arena.workspaces[0][0] == ws_bytes


def check_out_slice(run_out, d, tag):
    """run_out(out) writes into the middle of a larger buffer (a gradient bucket slice): the same bits, the neighbours untouched."""
    import torch
    n, pad = d.numel(), 96
    buf = torch.empty(n + 2 * pad, device="cuda")
    _bits(buf).fill_(NAN_BITS)
    keep = buf.clone()
    got = run_out(buf[pad:pad + n].view(d.shape))
    torch.cuda.synchronize()
    assert got.data_ptr() == buf.data_ptr() + 4 * pad and _same(got, d)
    assert _same(buf[:pad], keep[:pad]) and _same(buf[pad + n:], keep[pad + n:]), "%s: out='s neighbours were written" % tag


def check_bf16_representable(run, ref64, operands, tag, scale="the output scale"):
    """bf16-representable operands: lo = 0, the products are exact, only the fp32 accumulation is left."""
    import torch
    rounded = [t.to(torch.bfloat16).float() for t in operands]
    r64 = ref64(*rounded)
    e = float((run(*rounded).double() - r64).abs().max() / r64.abs().max())
    print("%s bf16-representable operands: %.2e of %s" % (tag, e, scale))
    assert e <= 1e-5, (tag, e)


# ---- through the modules ---------------------------------------------------------------------------------------------------------------
def _direct_math(request, deterministic):
    import torch
    from deepinpainting_amd.models import hipconv
    was = (hipconv._MATH["fp32"], hipconv._check_hook, torch.backends.cudnn.deterministic)

    def restore():
        hipconv.set_conv_math(fp32=was[0])
        hipconv._check_hook = was[1]
        torch.backends.cudnn.deterministic = was[2]
    request.addfinalizer(restore)
    if deterministic:
        torch.backends.cudnn.deterministic = True        # MIOpen: ask for solvers that repeat their bits, so that bits can be compared
    return hipconv


@pytest.fixture
def direct_math(request):
    return _direct_math(request, False)


@pytest.fixture(name="direct_math")
def direct_math_deterministic(request):
    """`direct_math` for the tests that compare a weight gradient of MIOpen's bit for bit."""
    return _direct_math(request, True)


def _module_pass(hipconv, m, x, dy):
    import torch
    seen = {}
    hipconv._check_hook = lambda kind, eng, geom, operands, result: seen.__setitem__(kind, eng)
    xr = x.clone().requires_grad_(True)
    y = hipconv.conv_nobias(m, xr)
    dx, dw = torch.autograd.grad(y, (xr, m.weight), dy)
    torch.cuda.synchronize()
    return seen, y.detach(), dx, dw


# ---- without a GPU ----------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    from deepinpainting_amd import _lib
    return _lib.lib()


@pytest.fixture
def hipconv(lib, monkeypatch):
    """The dispatcher with no engine forced, no A/B switch set and the default arithmetic; restored afterwards."""
    from deepinpainting_amd.models import hipconv as hc
    monkeypatch.setattr(hc, "_FORCE", None)
    for name in ("IPSR_CONV_ENGINE", "IPSR_NO_SMALLMAP", "IPSR_NO_THIN", "IPSR_SMALLMAP_MAX_POS", "IPSR_BF16_ENGINES"):
        monkeypatch.delenv(name, raising=False)
    hc.reload_env()
    was = hc._MATH["fp32"]
    yield hc
    hc._FORCE = None
    hc.set_conv_math(fp32=was)
    hc.reload_env()


def fake_pointers(offsets, stride=1 << 28, base=1 << 40):
    """One far-apart fake address per operand, moved by its offset; None stays a null pointer."""
    return [None if o is None else base + i * stride + o for i, o in enumerate(offsets)]


def refused_calls(calls):
    """calls: {name: (entry, [arguments])} on fake addresses.  Runs them in a child process with every GPU hidden (a call that got past its
    argument checks would fail there, not launch) -> {name: [return code, ipsr_last_error()]}."""
    env = dict(os.environ, HIP_VISIBLE_DEVICES="-1", CUDA_VISIBLE_DEVICES="-1", ROCR_VISIBLE_DEVICES="-1")
    res = subprocess.run([sys.executable, os.path.abspath(__file__), json.dumps(calls)], env=env, cwd=ROOT, capture_output=True, text=True, timeout=120)
    assert res.returncode == 0, res.stderr[-2000:]
    return json.loads(res.stdout.strip().splitlines()[-1])


def _child(calls):
    sys.path.insert(0, ROOT)
    from deepinpainting_amd import _lib
    L = _lib.lib()
    out = {}
    for name, (entry, args) in calls.items():
        rc = getattr(L, entry)(*args)
        out[name] = (rc, L.ipsr_last_error().decode("utf-8", "replace"))
    print(json.dumps(out))


if __name__ == "__main__":
    _child(json.loads(sys.argv[1]))
