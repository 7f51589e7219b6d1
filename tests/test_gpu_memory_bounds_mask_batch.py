"""The guarded-memory rows of the batched per-sample-mask entries: ipsr_mask_index (csrc/mask_ops.hip), innercos_loss_masks and
innercos_loss_backward_masks (csrc/innercos.hip).

The rows are entered into the registry of tests/test_gpu_memory_bounds.py through its own `case` decorator, at import, so that its
`test_every_launching_entry_has_a_row` finds the entries covered, and they run here through that module's own harness (guard bands
around every buffer, a workspace of exactly the size asked, inputs untouched, the guarded result bit-identical to the normal one,
every element written).  ipsr_mask_index: ws="zero", its workspace holds integers; R = 5 at 100x140 with 3 layers (levels in LDS, a
12x17 feature mask, rows of different counts, an empty and a full one), R = 2 at 67x73 with 1 layer (N = 1188: two 1024-chunks of
the compaction), layers = 0, two row sets past the LDS (the levels in the workspace slices, whose size is then exact: 600x600 by
byte loads, 640x608 by the 16-byte loads of whole-vector rows) and 256x256, the 16-byte loads in LDS.
InnerCos: the scalar path with Cx > Cuse, and 5115 rows (two per workgroup, a workgroup astride every sample boundary).
"""
import pytest
import torch

import test_gpu_memory_bounds as M

MASK_INDEX = ("ipsr_mask_index",)
INNERCOS = ("innercos_loss_masks", "innercos_loss_backward_masks")
MI_ROWS = (("mask_index_r5_100x140_l3", 5, 100, 140, 3, 3), ("mask_index_r2_67x73_l1", 2, 67, 73, 1, 1), ("mask_index_r3_12x17_l0", 3, 12, 17, 0, 2),
           ("mask_index_r2_600x600_l3", 2, 600, 600, 3, 1), ("mask_index_r2_640x608_l3", 2, 640, 608, 3, 1), ("mask_index_r3_256x256_l3", 3, 256, 256, 3, 1))
IC_ROWS = ((3, 11, 8, 5, 7), (5, 1023, 1023, 4, 4))


def _iid(s):
    return "innercos_masks_" + "_".join(map(str, s))


def _masks(R, H, W):
    dens = (0.3, 0.0, 0.55, 1.0, 0.4)
    return torch.stack([(torch.rand(H, W, generator=M._gen(7 + r)) < dens[r % 5]).to(torch.uint8) for r in range(R)]).cuda()


for _cid, _R, _H, _W, _layers, _patch in MI_ROWS:
    if _cid not in {c[0] for c in M.CASES}:             # a second import of this file must not enter a row twice
        @M.case(_cid, MASK_INDEX, ws="zero")
        def _(mk, R=_R, H=_H, W=_W, layers=_layers, patch=_patch):
            from deepinpainting_amd import ops
            feat, flag, mpi, counts = ops.mask_index(mk("masks", _masks(R, H, W)), layers, 5 / 16.0, patch, 1, 1)
            assert (feat is None) == (layers == 0)
            res = dict(flag=flag, mpi=mpi, counts=counts)
            return res if feat is None else dict(res, feat=feat)

for _s in IC_ROWS:
    if _iid(_s) not in {c[0] for c in M.CASES}:
        @M.case(_iid(_s), INNERCOS)
        def _(mk, s=_s):
            from deepinpainting_amd import ops
            B, Cx, Cuse, h, w = s
            x = mk("x", M.rn(B, Cx, h, w, seed=1))
            m = torch.stack([M._mask(h, w, 20 + b, p=(0.4, 0.0, 1.0, 0.3, 0.6)[b % 5]).float() for b in range(B)])
            m, t = mk("mask", m), mk("target", M.rn(B, Cuse, h, w, seed=3))
            return dict(loss=ops.innercos_loss(x, Cuse, m, t, 0.5), gx=ops.innercos_loss_backward(x, Cuse, m, t, 0.5, mk("gl", M.rn(1, seed=4))))

IDS = [r[0] for r in MI_ROWS] + [_iid(s) for s in IC_ROWS]


def test_the_rows_are_in_the_registry():
    covered = {c[0]: c[1] for c in M.CASES}
    assert all(covered.get(r[0]) == MASK_INDEX for r in MI_ROWS) and all(covered.get(_iid(s)) == INNERCOS for s in IC_ROWS)
    for entry in MASK_INDEX + INNERCOS:
        assert entry in M._declared() and entry not in M.EXEMPT and entry not in M.ALIASES


@pytest.mark.gpu
@pytest.mark.parametrize("cid", IDS)
def test_guard_bands_and_poisoned_scratch(cid, monkeypatch):
    M.test_guard_bands_and_poisoned_scratch(cid, monkeypatch)
