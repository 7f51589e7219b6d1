"""The rows of tests/test_gpu_memory_bounds.py for the launching entry ipsr_conv4x4s2_bf16x3_wrw (the split-bf16 weight gradient of the k4 s2
p1 layers on fp32 tensors), kept in a file of their own: they are registered through that module's `case`, so that its
`test_every_launching_entry_has_a_row` finds them whenever the suite is collected, and run through its harness here (the parametrised test
there fixes its list of cases when that module is imported).
"""
import pytest

import test_gpu_memory_bounds as M

_IDS = []
# (B, Kc, Cf, nh, nw): one ragged tile, one stage; the widest grid, several runs per image; two stages per workgroup (the ring wraps)
for _B, _Kc, _Cf, _nh, _nw in ((1, 48, 16, 4, 16), (2, 64, 128, 3, 64), (2, 340, 380, 16, 16)):
    _IDS.append("bf16x3_s2_wrw_%d_%d_%dx%d_b%d" % (_Kc, _Cf, _nh, _nw, _B))

    @M.case(_IDS[-1], ["ipsr_conv4x4s2_bf16x3_wrw"])
    def _(mk, Kc=_Kc, Cf=_Cf, nh=_nh, nw=_nw, B=_B):
        from deepinpainting_amd import ops
        fine, coarse = mk("fine", M.rn(B, Cf, 2 * nh, 2 * nw, seed=1)), mk("coarse", M.rn(B, Kc, nh, nw, seed=2))
        return {"dw": ops.conv4x4s2_bf16x3_wrw(fine, coarse, B, Kc, Cf, nh, nw)}


def test_the_rows_are_registered():
    assert "ipsr_conv4x4s2_bf16x3_wrw" in {e for c in M.CASES for e in c[1]} and len({c[0] for c in M.CASES}) == len(M.CASES)


@pytest.mark.gpu
@pytest.mark.parametrize("cid", _IDS)
def test_guard_bands_and_poisoned_scratch(cid, monkeypatch):
    M.test_guard_bands_and_poisoned_scratch(cid, monkeypatch)
