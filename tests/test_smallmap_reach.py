"""The reach of the small-map engine's tiled regime (models/hipconv.py `select(..., reach=)` / `select_wrw(..., reach=)`): pure host logic
plus workspace probes, no kernel is launched.  Over the axes of tests/test_abi.py's recorded grid:
  * reach None (and 0) answers what the call without the keyword answers;
  * reach 1024 moves an answer only from "miopen" to "smallmap", never under bf16 activations, a forced engine or IPSR_NO_SMALLMAP=1;
  * the passes of the training step that were measured ahead of MIOpen move (`_reach_regime`), the others stay;
  * the reach lives on the trainer's modules: building a trainer changes no answer of `select` / `select_wrw` in the process.
"""
import pytest

import test_abi as A
from test_abi import built  # noqa: F401  (fixture)


def _grid(hipconv, ops, reach, use_keyword=True):
    kw = {"reach": reach} if use_keyword else {}
    out = []
    for B, bf16 in A._SEL_AXES["batch_bf16"]:
        for k, stride, pad, dil in A._SEL_AXES["k_stride_pad_dil"]:
            for Cin in A._SEL_AXES["channels"]:
                for Cout in A._SEL_AXES["channels"]:
                    for H in A._SEL_AXES["extent"]:
                        lay = (B, Cin, H, H, Cout, k, stride, pad, dil)
                        for op in (ops.CONV_FWD, ops.CONV_BWD_DATA, ops.CONVT_FWD, ops.CONVT_BWD_DATA):
                            out.append(((op,) + lay + (bf16,), hipconv.select(op, *lay, bf16, **kw)))
                        for transposed in (False, True):
                            out.append((("wrw", transposed) + lay + (bf16,), hipconv.select_wrw(transposed, *lay, bf16, **kw)))
    return out


@pytest.fixture()
def dispatcher(built, monkeypatch):  # noqa: F811
    from deepinpainting_amd import ops
    from deepinpainting_amd.models import hipconv
    monkeypatch.setattr(hipconv, "_FORCE", None)
    for var in A._SEL_SWITCHES:
        monkeypatch.delenv(var, raising=False)
    hipconv.reload_env()
    yield hipconv, ops
    monkeypatch.undo()
    hipconv.reload_env()


def test_no_reach_is_todays_answer(dispatcher):
    hipconv, ops = dispatcher
    base = _grid(hipconv, ops, None, use_keyword=False)
    assert _grid(hipconv, ops, None) == base and _grid(hipconv, ops, 0) == base
    assert _grid(hipconv, ops, None, use_keyword=False) == base          # and asking with a reach in between moved nothing in the memo
    _grid(hipconv, ops, 1024)
    assert _grid(hipconv, ops, None, use_keyword=False) == base


def test_reach_moves_miopen_to_smallmap_only(dispatcher, monkeypatch):
    hipconv, ops = dispatcher
    base, far = _grid(hipconv, ops, None), _grid(hipconv, ops, 1024)
    moved = [(p, b, f) for (p, b), (_, f) in zip(base, far) if b != f]
    assert moved, "the reach moves nothing"
    for p, b, f in moved:
        assert (b, f) == ("miopen", "smallmap") and p[-1] is False and p[0] != "wrw", (p, b, f)
        Cin, Cout, k = p[2], p[5], p[6]
        assert k == 4 and min(Cin, Cout) >= 256, p
    # a smaller reach moves a subset; the switches that switch the engine off win
    near = _grid(hipconv, ops, 128)
    assert 0 < sum(b != n for (_, b), (_, n) in zip(base, near)) < len(moved)
    assert all(n in (b, f) for (_, b), (_, n), (_, f) in zip(base, near, far))
    for var, val in (("IPSR_NO_SMALLMAP", "1"), ("IPSR_CONV_ENGINE", "miopen"), ("IPSR_CONV_ENGINE", "direct")):
        monkeypatch.setenv(var, val)
        hipconv.reload_env()
        assert _grid(hipconv, ops, 1024) == _grid(hipconv, ops, None), (var, val)
        monkeypatch.delenv(var)
    hipconv.reload_env()
    monkeypatch.setattr(hipconv, "_FORCE", "miopen")
    assert _grid(hipconv, ops, 1024) == _grid(hipconv, ops, None)


# the step's 512 / 1024-channel layers on 2x2 .. 16x16 maps, as (module, Cin, Cout, (k, stride, pad, dil), input extent, batches, the passes
# that move): the rows of profiles/smallmap_tiled_layers.txt that won.  The passes not named stay where they were.
STEP_PASSES = (
    ("conv", 512, 512, (4, 2, 1, 1), 16, (8, 16), ("fwd",)),             # netP / netF: dx is checked per batch below
    ("conv", 512, 512, (4, 2, 1, 1), 8, (8, 16), ("fwd", "dx")),
    ("convT", 1024, 512, (4, 2, 1, 1), 4, (8,), ("fwd", "dx")),
    ("convT", 1024, 512, (4, 2, 1, 1), 8, (8,), ("fwd",)),               # its input gradient is level with MIOpen, stays
    ("conv", 512, 512, (4, 2, 3, 2), 16, (8,), ("fwd",)),                # netG, dilated: its input gradient @16 is "direct"'s
    ("conv", 512, 512, (4, 2, 3, 2), 8, (8,), ("fwd", "dx")),
    ("conv", 512, 512, (3, 1, 1, 1), 8, (8,), ()),                       # k3 stays (`_reach_regime`)
    ("conv", 512, 512, (3, 1, 1, 1), 4, (8,), ()),
    ("conv", 512, 512, (3, 1, 1, 1), 2, (8,), ()),                       # (its data passes are the chain's own "smallmap")
    ("convT", 1024, 512, (3, 1, 1, 1), 2, (8,), ()),
    ("convT", 1024, 512, (3, 1, 1, 1), 4, (8,), ()),
    ("convT", 1024, 512, (3, 1, 1, 1), 8, (8,), ()),
    ("convT", 512, 512, (4, 2, 1, 1), 4, (8,), ("fwd", "dx")),
    ("convT", 512, 512, (4, 2, 1, 1), 8, (8,), ("fwd", "dx")),
)


def test_the_steps_passes_move(dispatcher):
    hipconv, ops = dispatcher
    for kind, Cin, Cout, geom, H, batches, passes in STEP_PASSES:
        tr = kind == "convT"
        for B in batches:
            lay = (B, Cin, H, H, Cout) + geom
            for name in ("fwd", "dx"):
                op = {("fwd", False): ops.CONV_FWD, ("dx", False): ops.CONV_BWD_DATA, ("fwd", True): ops.CONVT_FWD, ("dx", True): ops.CONVT_BWD_DATA}[name, tr]
                if name in passes:
                    assert hipconv.select(op, *lay) == "miopen", (kind, lay, name)
                    assert hipconv.select(op, *lay, reach=1024) == "smallmap", (kind, lay, name)
                elif (kind, H, B, name) != ("conv", 16, 8, "dx"):
                    assert hipconv.select(op, *lay, reach=1024) == hipconv.select(op, *lay), (kind, lay, name)
                assert hipconv.select(op, *lay, True, reach=1024) == hipconv.select(op, *lay, True), "bf16 activations moved"
            assert hipconv.select_wrw(tr, *lay, reach=1024) == hipconv.select_wrw(tr, *lay), (kind, lay)      # no weight gradient moves
            assert hipconv.select_wrw(tr, *lay, True, reach=1024) == hipconv.select_wrw(tr, *lay, True), "bf16 activations moved"
    # netP / netF 512 -> 512 k4 s2 @16: the input gradient moves at batch 8 and stays with "wino_s2" at batch 16
    lay = (512, 16, 16, 512, 4, 2, 1, 1)
    assert hipconv.select(ops.CONV_BWD_DATA, 8, *lay, reach=1024) == "smallmap"
    assert hipconv.select(ops.CONV_BWD_DATA, 16, *lay) == hipconv.select(ops.CONV_BWD_DATA, 16, *lay, reach=1024) == "wino_s2"
    # beyond the reach, and below the regime's first position count, nothing moves
    assert hipconv.select(ops.CONV_FWD, 8, 512, 32, 32, 512, 4, 2, 1, 1, reach=1024) == hipconv.select(ops.CONV_FWD, 8, 512, 32, 32, 512, 4, 2, 1, 1)
    assert hipconv.select(ops.CONV_FWD, 8, 512, 16, 16, 512, 4, 2, 1, 1, reach=256) == "miopen"


def test_building_a_trainer_moves_no_answer(dispatcher, tmp_path):
    """The reach is stamped on the trainer's modules (`smallmap_reach`), not kept in the process: the dispatcher's answers to everybody else
    are the same before and after a trainer exists, and `smallmap_reach=0` / bf16 activations stamp none."""
    import contextlib
    import io
    import torch
    from deepinpainting_amd.options import Option
    from oracle import cpu_model                # the CPU twin of the trainer: the same IPSR.initialize on oracle layers
    hipconv, ops = dispatcher
    before = _grid(hipconv, ops, None, use_keyword=False)
    for kw, want in ((dict(), 1024), (dict(smallmap_reach=256), 256), (dict(smallmap_reach=0), None), (dict(amp_bf16=True), None)):
        opt = Option(gpu_ids=[], batchSize=1, quiet=True, allow_random_vgg=True, checkpoints_dir=str(tmp_path), **kw)
        with contextlib.redirect_stdout(io.StringIO()):
            m = cpu_model.create_cpu_model(opt)
        convs = [mod for net in (m.netG, m.netP, m.netD, m.netF) for mod in net.modules() if isinstance(mod, (torch.nn.Conv2d, torch.nn.ConvTranspose2d))]
        assert len(convs) > 40 and all(getattr(mod, "smallmap_reach", "unset") == want for mod in convs), kw
        assert not any(hasattr(mod, "smallmap_reach") for mod in m.vgg.modules())
        assert _grid(hipconv, ops, None, use_keyword=False) == before, kw
