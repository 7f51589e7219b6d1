"""The guarded-memory rows of ipsr_conv4x4s2_bf16_dil_wrw (the direct bf16 weight gradient of the dilated k4 s2 p3 d2 layer).

The rows are entered into the registry of tests/test_gpu_memory_bounds.py through its own `case` decorator, at import, so that its
`test_every_launching_entry_has_a_row` finds the entry covered, and they run here through that module's own harness
(`test_guard_bands_and_poisoned_scratch`: guard bands around every buffer, a NaN-filled workspace of exactly the size asked, inputs
untouched, the guarded result bit-identical to the normal one, every element written).  That module's parametrisation is fixed when it
is imported, which is before these rows exist; hence the test function of this file (the pattern of tests/test_gpu_memory_bounds_bf16_dil.py).
"""
import pytest

import bf16_dil_wrw_plan as X
import test_gpu_memory_bounds as M

ENTRY = "ipsr_conv4x4s2_bf16_dil_wrw"
# one ragged tile, one stage; the 128-wide grid (half-row stages); 32 runs
SHAPES = tuple(X.CASES[cid][0] for cid in ("one", "w128", "cut"))


def _cid(B, Kc, Cf, nh, nw):
    return "bf16_dil_wrw_%d_%d_%dx%d_b%d" % (Kc, Cf, nh, nw, B)


for _shape in SHAPES:
    if _cid(*_shape) not in {c[0] for c in M.CASES}:           # a second import of this file must not enter a row twice
        @M.case(_cid(*_shape), [ENTRY])
        def _(mk, shape=_shape):
            from deepinpainting_amd import ops
            B, Kc, Cf, nh, nw = shape
            fine, coarse = mk("fine", M.rn(B, Cf, 2 * nh, 2 * nw, seed=1, dtype=M.BF16)), mk("coarse", M.rn(B, Kc, nh, nw, seed=2, dtype=M.BF16))
            return {"dw": ops.conv4x4s2_bf16_dil_wrw(fine, coarse, B, Kc, Cf, nh, nw)}


def test_the_rows_are_in_the_registry():
    covered = {c[0]: c[1] for c in M.CASES}
    assert all(covered.get(_cid(*s)) == (ENTRY,) for s in SHAPES)
    assert ENTRY in M._declared() and ENTRY not in M.EXEMPT and ENTRY not in M.ALIASES
    assert all(X.plan(*s) is not None for s in SHAPES)


@pytest.mark.gpu
@pytest.mark.parametrize("shape", SHAPES, ids=[_cid(*s) for s in SHAPES])
def test_guard_bands_and_poisoned_scratch(shape, monkeypatch):
    M.test_guard_bands_and_poisoned_scratch(_cid(*shape), monkeypatch)
