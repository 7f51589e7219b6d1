"""The guarded-memory rows of the fused loss heads (csrc/loss_head.hip): ipsr_ragan_loss, ipsr_l1_pair_loss and their backward
ipsr_loss_grad_scale.

The rows are entered into the registry of tests/test_gpu_memory_bounds.py through its own `case` decorator, at import, so that its
`test_every_launching_entry_has_a_row` finds the entries covered, and they run here through that module's own harness
(`test_guard_bands_and_poisoned_scratch`: guard bands around every buffer, a NaN-filled workspace of exactly the size asked, inputs
untouched, the guarded result bit-identical to the normal one, every element written).  That module's parametrisation is fixed when it
is imported, which is before these rows exist; hence the test function of this file.  The shapes are the ragged ones of
tests/test_gpu_loss_head.py: one element, one past a wave / a workgroup, unequal sizes, a last workgroup that is not full, a count
that is no multiple of the 4-element vectors.
"""
import pytest

import test_gpu_memory_bounds as M

RAGAN = ("ipsr_ragan_loss", "ipsr_loss_grad_scale")
L1 = ("ipsr_l1_pair_loss", "ipsr_loss_grad_scale")
RAGAN_SHAPES = ((1, 1), (65, 63), (1025, 1023), (900, 1800), (7200, 7200), (4097, 8195), (65536, 65536))      # the last two: 3 and 16 workgroups
L1_SHAPES = (1, 257, 2 * 2048 + 1027, 2 * 3 * 64 * 64)


def _rid(nf, nr):
    return "ragan_loss_%d_%d" % (nf, nr)


def _lid(n):
    return "l1_pair_loss_%d" % n


for _nf, _nr in RAGAN_SHAPES:
    if _rid(_nf, _nr) not in {c[0] for c in M.CASES}:           # a second import of this file must not enter a row twice
        @M.case(_rid(_nf, _nr), RAGAN)
        def _(mk, nf=_nf, nr=_nr):
            from deepinpainting_amd import ops
            fake, real = mk("fake", M.rn(nf, seed=1)), mk("real", M.rn(nr, seed=2))
            gl = mk("gl", M.rn(1, seed=3))
            loss, gf, gr = ops.ragan_loss(fake, real, -1.0)
            loss_f, gf_only, none = ops.ragan_loss(fake, real, 1.0, want_real=False)
            assert none is None
            loss_j, joined = ops.ragan_loss(fake, real, -1.0, joined=True)
            bf, br = ops.loss_grad_scale(gl, gf, gr)
            bj, _ = ops.loss_grad_scale(gl, joined)
            return dict(loss=loss, gf=gf, gr=gr, loss_f=loss_f, gf_only=gf_only, loss_j=loss_j, joined=joined, bf=bf, br=br, bj=bj)

for _n in L1_SHAPES:
    if _lid(_n) not in {c[0] for c in M.CASES}:
        @M.case(_lid(_n), L1)
        def _(mk, n=_n):
            from deepinpainting_amd import ops
            a1, a2, t = mk("a1", M.rn(n, seed=1)), mk("a2", M.rn(n, seed=2)), mk("t", M.rn(n, seed=3))
            gl = mk("gl", M.rn(1, seed=4))
            loss, g1, g2 = ops.l1_pair_loss(a1, a2, t, 100.0)
            loss_v, none1, none2 = ops.l1_pair_loss(a1, a2, t, 100.0, want1=False, want2=False)
            assert none1 is None and none2 is None
            b1, b2 = ops.loss_grad_scale(gl, g1, g2)
            res = dict(loss=loss, g1=g1, g2=g2, loss_v=loss_v, b1=b1, b2=b2)
            if n > 1:
                # operands 4 bytes off a 16-byte boundary (a contiguous view x[1:]): the element-by-element path of both kernels
                res["loss_s"], res["g1_s"], res["g2_s"] = ops.l1_pair_loss(a1[1:], a2[1:], t[1:], 100.0)
                res["b_s"], _ = ops.loss_grad_scale(gl, g1[1:])
            return res

IDS = [_rid(*s) for s in RAGAN_SHAPES] + [_lid(n) for n in L1_SHAPES]


def test_the_rows_are_in_the_registry():
    covered = {c[0]: c[1] for c in M.CASES}
    assert all(covered.get(_rid(*s)) == RAGAN for s in RAGAN_SHAPES) and all(covered.get(_lid(n)) == L1 for n in L1_SHAPES)
    for entry in set(RAGAN + L1):
        assert entry in M._declared() and entry not in M.EXEMPT and entry not in M.ALIASES


@pytest.mark.gpu
@pytest.mark.parametrize("cid", IDS)
def test_guard_bands_and_poisoned_scratch(cid, monkeypatch):
    M.test_guard_bands_and_poisoned_scratch(cid, monkeypatch)
