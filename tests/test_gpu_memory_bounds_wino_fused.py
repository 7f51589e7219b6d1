"""The guarded-memory rows of the one-launch Winograd kernel (csrc/wino_fused.hip, reached through `ops.conv3x3_winograd` under
`ipsr_debug_set_option(7, 2)`).

As tests/test_gpu_memory_bounds_smallmap_tiled.py: the rows are entered into the registry of tests/test_gpu_memory_bounds.py through
its own `case` decorator at import and run here through that module's harness (guard bands around every buffer, a NaN-filled
workspace of exactly the size asked, inputs untouched, the guarded result bit-identical to the normal one, every element written).
Shapes: 9x65 (one pixel over a block of 2 x 16 tiles in both directions: three of the four blocks hold one tile row or column) and
37x70 (ragged last tile row and column, rows that are no whole vectors), in the four ops, with the padded produced channels
(K = 40) beside the full 64, with and without the filter cache, and the pooled epilogue on 38x70.
"""
import pytest
import torch

import test_gpu_memory_bounds as M

ENTRY = ("ipsr_conv3x3_winograd_mp",)
FUSED_OPTION = 7

# (id, op, B, Cin, H, W, Cout, epilogue)
ROWS = [("conv_fwd_9x65", "CONV_FWD", 3, 48, 9, 65, 40, "relu"), ("conv_bwd_9x65", "CONV_BWD_DATA", 1, 64, 9, 65, 16, None),
        ("convT_fwd_37x70", "CONVT_FWD", 2, 16, 37, 70, 64, None), ("convT_bwd_37x70", "CONVT_BWD_DATA", 3, 40, 37, 70, 48, None),
        ("conv_fwd_pool_38x70", "CONV_FWD", 1, 16, 38, 70, 40, "relu_pool")]


def _cid(row):
    return "wino_fused_" + row[0]


for _row in ROWS:
    if _cid(_row) not in {c[0] for c in M.CASES}:                 # a second import of this file must not enter a row twice
        @M.case(_cid(_row), list(ENTRY))
        def _(mk, row=_row):
            from deepinpainting_amd import _lib, ops
            _, opname, B, Cin, H, W, Cout, epi = row
            op = getattr(ops, opname)
            fwd = opname.endswith("FWD")
            x = mk("x", M.rn(B, Cin if fwd else Cout, H, W, seed=B + Cin + H))
            w = mk("w", M.rn(*((Cin, Cout, 3, 3) if opname.startswith("CONVT") else (Cout, Cin, 3, 3)), seed=W, scale=0.1))
            bias = mk("bias", M.rn(Cout, seed=7)) if epi else None
            _lib.check(_lib.lib().ipsr_debug_set_option(FUSED_OPTION, 2), "ipsr_debug_set_option")
            try:
                y = ops.conv3x3_winograd(op, x, w, (B, Cin, H, W), Cout, bias=bias, epilogue=epi)
                cache = ops.winograd_filter_cache(op, Cin, Cout, x.device)
                yc = ops.conv3x3_winograd(op, x, w, (B, Cin, H, W), Cout, bias=bias, epilogue=epi, filter_cache=cache, filter_cache_valid=False)
                yv = ops.conv3x3_winograd(op, x, w, (B, Cin, H, W), Cout, bias=bias, epilogue=epi, filter_cache=cache, filter_cache_valid=True)
            finally:
                _lib.lib().ipsr_debug_set_option(FUSED_OPTION, 0)
            return dict(y=y, yc=yc, yv=yv, cache=cache)

IDS = [_cid(r) for r in ROWS]


def test_the_rows_are_in_the_registry():
    covered = {c[0]: tuple(c[1]) for c in M.CASES}
    assert all(covered.get(cid) == ENTRY for cid in IDS)
    assert ENTRY[0] in M._declared() and ENTRY[0] not in M.EXEMPT and ENTRY[0] not in M.ALIASES
    # every row is inside the fused kernel's envelope: at most 64 produced channels, the reduction in whole chunks of 16
    for _, opname, B, Cin, H, W, Cout, _ in ROWS:
        red, prod = (Cin, Cout) if opname.endswith("FWD") else (Cout, Cin)
        assert prod <= 64 and red % 16 == 0


@pytest.mark.gpu
@pytest.mark.parametrize("cid", IDS)
def test_guard_bands_and_poisoned_scratch(cid, monkeypatch):
    M.test_guard_bands_and_poisoned_scratch(cid, monkeypatch)
