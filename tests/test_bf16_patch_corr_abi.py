"""The bf16 correlation for shift_sz > 1 at the C-ABI, without a GPU: workspace sizes, the C % 64 refusal and the ABI version
that tells callers the bf16 entries now accept shift_sz > 1.

The fp32 queries (p = 1 and p = 3) and the bf16 query for p = 1 must return exactly what they returned before the bf16 window
path existed: those plans are unchanged byte for byte.  The values below were recorded from the library at ABI 14.
"""
import ctypes
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
IPSR_ERR_UNSUPPORTED = -2
IPSR_ERR_WORKSPACE = -3

# (B, C, h, w, M, patch, stride) -> (ipsr_forward_workspace_bytes, ipsr_forward_bf16corr_workspace_bytes or None = changed)
RECORDED = {
    (4, 512, 64, 64, 1024, 3, 1): (854921216, None),
    (8, 512, 32, 32, 256, 3, 1): (302708736, None),
    (2, 64, 12, 20, 40, 2, 1): (1371648, None),
    (8, 512, 32, 32, 256, 1, 1): (36283136, 53060352),
    (4, 512, 64, 64, 1024, 1, 1): (84624128, 118178560),
    (2, 64, 16, 16, 64, 1, 1): (310528, 441600),
}


@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as g
    g.build()
    from deepinpainting_amd import _lib
    return _lib


def test_abi_version_is_15(built):
    L = built.lib()
    assert built.ABI_VERSION == 15
    assert L.ipsr_abi_version() == 15


@pytest.mark.parametrize("shape", sorted(RECORDED))
def test_unchanged_plans_keep_their_workspace_sizes(built, shape):
    L = built.lib()
    fp32, bf16 = RECORDED[shape]
    assert L.ipsr_forward_workspace_bytes(*shape) == fp32
    if bf16 is not None:
        assert L.ipsr_forward_bf16corr_workspace_bytes(*shape) == bf16


@pytest.mark.parametrize("B,C,h,w,M,p", [(4, 512, 64, 64, 1024, 3), (8, 512, 32, 32, 256, 3), (2, 64, 12, 20, 40, 2), (1, 64, 5, 5, 1, 3)])
def test_bf16_window_query_covers_the_packed_operands(built, B, C, h, w, M, p):
    """p > 1 with the bf16 correlation: the workspace holds the two packed [C/8][ld][8] bf16 copies of the raw features
    (ld = h*w rounded up to 128) on top of everything the fp32 p > 1 plan holds (R [B][hw][hw], xT [B][N'][K], the un-folded
    result [B][K][N'], the stencil partials)."""
    L = built.lib()
    ld = (h * w + 127) // 128 * 128
    got = L.ipsr_forward_bf16corr_workspace_bytes(B, C, h, w, M, p, 1)
    assert got >= 2 * B * C * ld * 2 + B * (h * w) ** 2 * 4
    assert got >= L.ipsr_forward_workspace_bytes(B, C, h, w, M, p, 1) + 2 * B * C * ld * 2 - 4096


def _child():
    """Runs with every GPU hidden, on fake device pointers: the C = 24, p = 3 bf16 call (C not a multiple of 64), and what the bf16
    arg-max entry (whole 128-column tiles only) and the p = 1 bf16 layer refuse."""
    sys.path.insert(0, ROOT)
    from deepinpainting_amd import _lib
    L = _lib.lib()
    base = 1 << 40
    ptr = [base + i * (1 << 20) for i in range(8)]
    out = {}
    for name, args in (
            ("forward_bf16corr", lambda: L.ipsr_forward_bf16corr(ptr[0], ptr[1], ptr[2], 10, 2, 24, 16, 16, 3, 1, ptr[3], ptr[4], ptr[5],
                                                                  None, ptr[6], ptr[7], 1 << 40, None)),
            ("forward_masks", lambda: L.ipsr_forward_masks(ptr[0], ptr[1], ptr[2], 0, ptr[6], 10, 2, 24, 16, 16, 3, 1, ptr[3], ptr[4],
                                                            ptr[5], None, None, ptr[7], 1 << 40, None, 1)),
            ("corr_bf16_n100", lambda: L.ipsr_corr_argmax_bf16(ptr[0], ptr[1], 1, 64, 100, ptr[4], ptr[5], ptr[7], 1 << 40, None)),
            ("corr_bf16_c32", lambda: L.ipsr_corr_argmax_bf16(ptr[0], ptr[1], 1, 32, 128, ptr[4], ptr[5], ptr[7], 1 << 40, None)),
            ("corr_bf16_ws_short", lambda: L.ipsr_corr_argmax_bf16(ptr[0], ptr[1], 1, 64, 128, ptr[4], ptr[5], ptr[7],
                                                                    L.ipsr_corr_argmax_bf16_workspace_bytes(1, 64, 128) - 1, None)),
            ("forward_bf16corr_p1_n100", lambda: L.ipsr_forward_bf16corr(ptr[0], ptr[1], ptr[2], 10, 1, 64, 10, 10, 1, 1, ptr[3], ptr[4],
                                                                          ptr[5], None, ptr[6], ptr[7], 1 << 40, None))):
        rc = args()
        out[name] = (rc, L.ipsr_last_error().decode("utf-8", "replace"))
    print(json.dumps(out))


@pytest.fixture(scope="module")
def refusals(built):
    env = dict(os.environ, HIP_VISIBLE_DEVICES="-1", CUDA_VISIBLE_DEVICES="-1", ROCR_VISIBLE_DEVICES="-1")
    res = subprocess.run([sys.executable, os.path.abspath(__file__), "--child"], env=env, cwd=ROOT, capture_output=True, text=True, timeout=120)
    assert res.returncode == 0, res.stderr[-2000:]
    return json.loads(res.stdout.strip().splitlines()[-1])


@pytest.mark.parametrize("entry", ["forward_bf16corr", "forward_masks"])
def test_c_not_multiple_of_64_is_refused_before_any_hip_call(refusals, entry):
    rc, msg = refusals[entry]
    assert rc == IPSR_ERR_UNSUPPORTED, (rc, msg)
    assert "C % 64" in msg and "shift_sz > 1" in msg and "C=24" in msg, msg


def test_bf16_argmax_entry_refuses_ragged_n_before_any_hip_call(refusals):
    """(B, C, N) = (1, 64, 100): the arg-max entry takes whole 128-column tiles only (the ragged kernel belongs to the R entry)."""
    rc, msg = refusals["corr_bf16_n100"]
    assert rc == IPSR_ERR_UNSUPPORTED, (rc, msg)
    assert "100" in msg, msg


def test_bf16_argmax_entry_refuses_c_not_multiple_of_64_before_any_hip_call(refusals):
    rc, msg = refusals["corr_bf16_c32"]
    assert rc == IPSR_ERR_UNSUPPORTED, (rc, msg)
    assert "32" in msg, msg


def test_bf16_argmax_entry_refuses_a_workspace_one_byte_short(refusals):
    rc, msg = refusals["corr_bf16_ws_short"]
    assert rc == IPSR_ERR_WORKSPACE, (rc, msg)


def test_bf16_layer_at_patch_1_refuses_ragged_n_before_any_hip_call(refusals):
    """patch = 1, C = 64, 10 x 10: N = 100 is no multiple of 128."""
    rc, msg = refusals["forward_bf16corr_p1_n100"]
    assert rc == IPSR_ERR_UNSUPPORTED, (rc, msg)


if __name__ == "__main__" and sys.argv[1:] == ["--child"]:
    _child()
