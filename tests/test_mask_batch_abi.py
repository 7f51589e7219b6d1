"""The batched per-sample-mask entries without a GPU: ipsr_mask_index, ipsr_mask_index_workspace_bytes (csrc/mask_ops.hip),
innercos_loss_masks, innercos_loss_backward_masks (csrc/innercos.hip).  Header, exports and binding table; the ABI version stays 15
(entries were added, no signature changed); the workspace query; the refusals that come before any HIP call (on fake addresses, in a
child process with every GPU hidden); the front-ends refuse CPU tensors.  Nothing here launches a kernel.
"""
import ctypes
import os
import re

import pytest
import torch

from bf16x3_harness import ROOT, fake_pointers, lib, refused_calls  # noqa: F401  (fixtures by name)

IPSR_ERR_INVALID, IPSR_ERR_WORKSPACE = -1, -3
ENTRIES = ("ipsr_mask_index_workspace_bytes", "ipsr_mask_index", "innercos_loss_masks", "innercos_loss_backward_masks")


def test_header_exports_and_bindings_carry_the_entries(lib):
    from deepinpainting_amd import _lib
    header = open(os.path.join(ROOT, "include", "ipsr_hip.h")).read()
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for name in ENTRIES:
        assert re.search(r"\b%s\(" % name, header), name
        assert hasattr(raw, name), "libipsr_hip.so lacks %s" % name
        assert name in _lib.SIGNATURES and getattr(lib, name).argtypes == _lib.SIGNATURES[name][1]
    assert "layers == 0" in header and "mask_bstride" in header
    # the masks entries are the existing ones with ONE more argument
    for old, new in (("innercos_loss", "innercos_loss_masks"), ("innercos_loss_backward", "innercos_loss_backward_masks")):
        assert len(_lib.SIGNATURES[new][1]) == len(_lib.SIGNATURES[old][1]) + 1
    table = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert all("`%s`" % name in table for name in ENTRIES)


def test_abi_version_stays_15(lib):
    from deepinpainting_amd import _lib
    assert lib.ipsr_abi_version() == 15 == _lib.ABI_VERSION


def test_workspace_query(lib):
    q = lib.ipsr_mask_index_workspace_bytes
    for H, W, layers in ((256, 256, 3), (512, 512, 3), (67, 73, 1), (32, 32, 0), (1024, 1024, 3), (2048, 1024, 5)):
        sizes = [q(R, H, W, layers) for R in (1, 2, 5, 8, 64)]
        assert sizes[0] > 0 and sizes == sorted(sizes), (H, W, layers, sizes)
    # the two image sizes of the project keep their levels in LDS: nothing per row.  Past the LDS the rows get slices of the workspace
    assert q(8, 256, 256, 3) == q(1, 256, 256, 3) and q(4, 512, 512, 3) == q(1, 512, 512, 3)
    one, two = q(1, 1024, 1024, 3), q(2, 1024, 1024, 3)
    assert two - one >= 512 * 512 + 256 * 256 * 4 and q(3, 1024, 1024, 3) - two == two - one       # level 1 in bytes + level 2 in counts
    # what the entry refuses: 0
    for bad in ((0, 64, 64, 3), (2, 64, 64, -1), (2, 64, 64, 6), (2, 4, 64, 3), (2, 64, 1, 1), (2, 0, 8, 0)):
        assert q(*bad) == 0, bad


@pytest.fixture(scope="module")
def refusals(lib):
    p = fake_pointers([0] * 6)
    need = lib.ipsr_mask_index_workspace_bytes(3, 64, 64, 3)
    big = lib.ipsr_mask_index_workspace_bytes(2, 1024, 1024, 3)
    ic_need = lib.innercos_workspace_bytes(2, 8, 64)

    def mi(masks=p[0], R=3, H=64, W=64, layers=3, patch=1, stride=1, feat=p[1], flag=p[2], mpi=p[3], counts=p[4], ws=p[5], ws_bytes=need):
        return ("ipsr_mask_index", (masks, R, H, W, layers, 0.3125, patch, stride, 1, feat, flag, mpi, counts, ws, ws_bytes, None))

    def fwd(x=p[0], shape=(2, 8, 8, 64), mask=p[1], bstride=64, target=p[2], loss=p[3], ws=p[4], ws_bytes=ic_need):
        return ("innercos_loss_masks", (x,) + tuple(shape) + (mask, bstride, target, 0.5, loss, ws, ws_bytes, None))

    def bwd(x=p[0], shape=(2, 8, 8, 64), mask=p[1], bstride=64, target=p[2], gl=p[3], gx=p[4]):
        return ("innercos_loss_backward_masks", (x,) + tuple(shape) + (mask, bstride, target, 0.5, gl, gx, None))
    return refused_calls({
        "mi_null_masks": mi(masks=None), "mi_null_feat": mi(feat=None), "mi_null_flag": mi(flag=None), "mi_null_mpi": mi(mpi=None),
        "mi_null_counts": mi(counts=None), "mi_null_feat_l0_patch": mi(layers=0, feat=None, patch=65),
        "mi_r0": mi(R=0), "mi_layers_neg": mi(layers=-1), "mi_layers_6": mi(layers=6), "mi_h1": mi(H=1),
        "mi_too_small": mi(H=4, layers=3), "mi_too_small_w": mi(W=7, layers=4),
        "mi_patch_9": mi(patch=9), "mi_patch_0": mi(patch=0), "mi_stride_0": mi(stride=0),
        "mi_null_ws": mi(ws=None), "mi_ws_short": mi(ws_bytes=need - 1), "mi_ws_short_big": mi(R=2, H=1024, W=1024, ws_bytes=big - 1),
        "f_null_x": fwd(x=None), "f_null_mask": fwd(mask=None), "f_null_ws": fwd(ws=None), "f_b0": fwd(shape=(0, 8, 8, 64)),
        "f_cuse": fwd(shape=(2, 8, 9, 64)), "f_bstride_1": fwd(bstride=1), "f_bstride_2n": fwd(bstride=128), "f_bstride_neg": fwd(bstride=-64),
        "f_odd_mask": fwd(mask=p[1] + 4), "f_ws_short": fwd(ws_bytes=ic_need - 1), "f_ws_short_shared": fwd(bstride=0, ws_bytes=ic_need - 1),
        "b_null_gx": bwd(gx=None), "b_null_gl": bwd(gl=None), "b_n0": bwd(shape=(2, 8, 8, 0), bstride=0), "b_bstride_63": bwd(bstride=63),
    })


@pytest.mark.parametrize("case,rc,msg", [
    ("mi_null_masks", IPSR_ERR_INVALID, "null pointer"), ("mi_null_feat", IPSR_ERR_INVALID, "null pointer"),
    ("mi_null_flag", IPSR_ERR_INVALID, "null pointer"), ("mi_null_mpi", IPSR_ERR_INVALID, "null pointer"),
    ("mi_null_counts", IPSR_ERR_INVALID, "null pointer"),
    ("mi_null_feat_l0_patch", IPSR_ERR_INVALID, "does not fit"),          # layers == 0 takes a NULL feat: the refusal is the patch's
    ("mi_r0", IPSR_ERR_INVALID, "bad size"), ("mi_layers_neg", IPSR_ERR_INVALID, "bad size"), ("mi_layers_6", IPSR_ERR_INVALID, "bad size"),
    ("mi_h1", IPSR_ERR_INVALID, "bad size"), ("mi_too_small", IPSR_ERR_INVALID, "too small"), ("mi_too_small_w", IPSR_ERR_INVALID, "too small"),
    ("mi_patch_9", IPSR_ERR_INVALID, "does not fit"), ("mi_patch_0", IPSR_ERR_INVALID, "bad geometry"),
    ("mi_stride_0", IPSR_ERR_INVALID, "bad geometry"),
    ("mi_null_ws", IPSR_ERR_WORKSPACE, "workspace"), ("mi_ws_short", IPSR_ERR_WORKSPACE, "workspace"),
    ("mi_ws_short_big", IPSR_ERR_WORKSPACE, "workspace"),
    ("f_null_x", IPSR_ERR_INVALID, "null pointer"), ("f_null_mask", IPSR_ERR_INVALID, "null pointer"), ("f_null_ws", IPSR_ERR_INVALID, "null pointer"),
    ("f_b0", IPSR_ERR_INVALID, "bad size"), ("f_cuse", IPSR_ERR_INVALID, "bad size"),
    ("f_bstride_1", IPSR_ERR_INVALID, "mask_bstride"), ("f_bstride_2n", IPSR_ERR_INVALID, "mask_bstride"),
    ("f_bstride_neg", IPSR_ERR_INVALID, "mask_bstride"), ("f_odd_mask", IPSR_ERR_INVALID, "16-byte aligned"),
    ("f_ws_short", IPSR_ERR_WORKSPACE, "workspace"), ("f_ws_short_shared", IPSR_ERR_WORKSPACE, "workspace"),
    ("b_null_gx", IPSR_ERR_INVALID, "null pointer"), ("b_null_gl", IPSR_ERR_INVALID, "null pointer"), ("b_n0", IPSR_ERR_INVALID, "bad size"),
    ("b_bstride_63", IPSR_ERR_INVALID, "mask_bstride")])
def test_refused_before_any_hip_call(refusals, case, rc, msg):
    got, text = refusals[case]
    assert got == rc and msg in text, (got, text)


def test_ops_refuse_cpu_tensors(lib):
    from deepinpainting_amd import ops
    with pytest.raises(RuntimeError, match="CUDA/HIP tensor"):
        ops.mask_index(torch.zeros(2, 64, 64, dtype=torch.uint8), 3, 0.3125, 1, 1, 1)
    with pytest.raises(RuntimeError, match="CUDA/HIP tensor"):
        ops.mask_index(torch.zeros(8, 8, dtype=torch.bool), 0, 0.0, 1, 1, 1)
    x, t, m = torch.zeros(2, 8, 4, 4), torch.zeros(2, 8, 4, 4), torch.zeros(2, 4, 4)            # the B*N mask form
    with pytest.raises(RuntimeError, match="CUDA/HIP tensor"):
        ops.innercos_loss(x, 8, m, t, 1.0)
    with pytest.raises(RuntimeError, match="CUDA/HIP tensor"):
        ops.innercos_loss_backward(x, 8, m, t, 1.0, torch.ones(1))


def test_the_switch_and_the_cpu_route():
    """One class-level switch, on by default; a CPU mask batch never reaches the batched front-end (it fails in today's per-sample one)."""
    from deepinpainting_amd.models.IPSR_model import IPSR_model
    from deepinpainting_amd.util import util
    assert IPSR_model.batched_masks is True
    with pytest.raises(RuntimeError, match="^mask must be a CUDA/HIP tensor"):                   # ops.feat_mask's name for its operand
        util.cal_feat_mask_batch(torch.zeros(2, 1, 64, 64, dtype=torch.bool), 3, 0.3125)
