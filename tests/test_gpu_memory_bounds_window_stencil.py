"""The guarded-memory rows of the LDS-tiled window stencil (csrc/window_stencil.hip, reached through `ops.forward(patch = p)` under
`ipsr_debug_set_option(8, 2)`).

As tests/test_gpu_memory_bounds_wino_fused.py: the rows are entered into the registry of tests/test_gpu_memory_bounds.py through its
own `case` decorator at import and run here through that module's harness (guard bands around every buffer, a workspace of exactly
the size the query reported, inputs untouched, the guarded result bit-identical to the normal one, every element written).  The
layer's workspace holds integers (arg-max indices), so it starts zero-filled, as in the other layer rows.  Shapes (from
tests/window_stencil_plan.py): the one-window case, the one wider than a wave (68 columns: two per thread, the second ragged) and
the one whose k' rows are split (partials in the window plan's slice, merged by a second launch).  Each row also asks the plan query
(`ipsr_window_corr_plan`, which launches nothing) that the tiled kernel is what ran.
"""
import pytest
import torch

import test_gpu_memory_bounds as M
import window_stencil_plan as W

ENTRY = ("ipsr_forward", "ipsr_window_corr_plan")
OPTION = 8
ROWS = ("one_window", "wider_than_a_wave", "many_per_thread_split")


def _cid(name):
    return "window_stencil_" + name


for _name in ROWS:
    if _cid(_name) not in {c[0] for c in M.CASES}:                 # a second import of this file must not enter a row twice
        @M.case(_cid(_name), list(ENTRY), ws="zero")
        def _(mk, name=_name):
            from deepinpainting_amd import _lib, ops
            B, C, h, w, p = W.GPU_CASES[name]
            x = mk("x", M.rn(B, C, h, w, seed=h + w, pos=True))
            ref = mk("ref", M.rn(B, C, h, w, seed=h + w + 1, pos=True))
            feat = torch.zeros(h, w, dtype=torch.uint8)
            feat[h // 2:h // 2 + 2, w // 2:w // 2 + 2] = 1
            _, mpi, cnt = ops.index_prep(mk("feat", feat.cuda()), p, 1, 1)
            n = int(cnt.item())
            assert n > 0
            _lib.check(_lib.lib().ipsr_debug_set_option(OPTION, 2), "ipsr_debug_set_option")
            try:
                assert ops.window_corr_plan(B, h, w, p)["variant"] == W.LDS_TILED
                f = ops.forward(x, ref, mk("mpi", mpi[:n].contiguous()), patch=p, want_attn=True)
            finally:
                _lib.lib().ipsr_debug_set_option(OPTION, 0)
            return dict(out=f.out, ind=f.ind, vmax=f.vmax, attn=f.attn_rows, bidx=f.bwd_index)

IDS = [_cid(n) for n in ROWS]


def test_the_rows_are_in_the_registry():
    covered = {c[0]: tuple(c[1]) for c in M.CASES}
    assert all(covered.get(cid) == ENTRY for cid in IDS)
    assert all(e in M._declared() and e not in M.EXEMPT and e not in M.ALIASES for e in ENTRY)
    plans = {n: W.plan(W.GPU_CASES[n][0], *W.GPU_CASES[n][2:], 2) for n in ROWS}
    assert all(pl["variant"] == W.LDS_TILED for pl in plans.values())
    assert plans["one_window"]["workgroups"] == 1 and plans["many_per_thread_split"]["split"] > 1


@pytest.mark.gpu
@pytest.mark.parametrize("cid", IDS)
def test_guard_bands_and_poisoned_scratch(cid, monkeypatch):
    M.test_guard_bands_and_poisoned_scratch(cid, monkeypatch)
