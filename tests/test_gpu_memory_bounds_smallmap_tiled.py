"""The guarded-memory rows of the small-map engine's tiled regime (csrc/smallmap.hip, `ops.conv_smallmap(..., tiled=True)`).

As tests/test_gpu_memory_bounds_loss_head.py: the rows are entered into the registry of tests/test_gpu_memory_bounds.py through its own
`case` decorator at import and run here through that module's harness (guard bands around every buffer, a NaN-filled workspace of
exactly the size asked, inputs untouched, the guarded result bit-identical to the normal one, every element written).  The shapes are
those of tests/test_gpu_smallmap_tiled.py: 33 positions (most of a position tile and of a row tile empty), 1024 positions, the ragged
last split of either GEMM, 129 positions (a second position tile with one position), the dilated geometry with an odd fine grid.
"""
import pytest
import torch

import test_gpu_memory_bounds as M
import test_gpu_smallmap_tiled as T

ENTRY = ("ipsr_conv_smallmap",)
ROWS = (0, 2, 3, 5, 7, 8, 9)           # indices into T.CASES


def _cid(i):
    return "smallmap_tiled_" + T.IDS[i]


for _i in ROWS:
    if _cid(_i) not in {c[0] for c in M.CASES}:                 # a second import of this file must not enter a row twice
        @M.case(_cid(_i), list(ENTRY))
        def _(mk, case=T.CASES[_i]):
            from deepinpainting_amd import ops
            coarse, fine, w, _, _, _, geo = T._reference(case)
            c, f, wt = mk("coarse", coarse.cuda()), mk("fine", fine.cuda()), mk("w", w.cuda())
            return dict(fwd=ops.conv_smallmap(ops.SM_FWD, f, wt, *geo, tiled=True), data=ops.conv_smallmap(ops.SM_DATA, c, wt, *geo, tiled=True),
                        wrw=ops.conv_smallmap(ops.SM_WRW, c, f, *geo, tiled=True))

IDS = [_cid(i) for i in ROWS]


def test_the_rows_are_in_the_registry():
    covered = {c[0]: tuple(c[1]) for c in M.CASES}
    assert all(covered.get(cid) == ENTRY for cid in IDS)
    assert ENTRY[0] in M._declared() and ENTRY[0] not in M.EXEMPT and ENTRY[0] not in M.ALIASES


@pytest.mark.gpu
@pytest.mark.parametrize("cid", IDS)
def test_guard_bands_and_poisoned_scratch(cid, monkeypatch):
    M.test_guard_bands_and_poisoned_scratch(cid, monkeypatch)
