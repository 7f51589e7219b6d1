"""`fused.match`: the steps a module list is turned into, as literals.  No tensor, no GPU, no library."""
import torch.nn as nn

from deepinpainting_amd.models import networks
from deepinpainting_amd.models.fused import FusedSequential, Step, match

LEAKY, RELU, NONE = ("leaky", 0.2), ("relu", 0.0), ("none", 0.0)
INSTANCE = networks.get_norm_layer('instance')


def module(n=1):
    return [Step("module", None, None, None, None, None, False, None, 1)] * n


def test_runs_within_one_level():
    conv, convT, norm = nn.Conv2d(4, 4, 3), nn.ConvTranspose2d(4, 4, 3), nn.InstanceNorm2d(4)
    assert match([conv, nn.LeakyReLU(0.2, True)]) == [Step("bias", conv, None, LEAKY, "level", None, False, None, 2)]
    assert match([convT, norm, nn.ReLU()]) == [Step("norm", convT, norm, RELU, "level", None, False, None, 3)]
    assert match([conv, norm]) == [Step("norm", conv, norm, NONE, None, None, False, None, 2)]
    assert match([norm, nn.LeakyReLU(0.1)]) == [Step("norm", None, norm, ("leaky", 0.1), "level", None, False, None, 2)]
    assert match([conv, nn.Tanh()]) == [Step("bias", conv, None, NONE, None, None, False, None, 1)] + module()
    assert match([conv, norm, nn.Dropout(0.5)]) == [Step("norm", conv, norm, NONE, None, None, False, None, 2)] + module()
    # two runs, and an activation in the middle that belongs to neither
    assert match([conv, nn.ReLU(), nn.ReLU(True), convT, norm]) == [Step("bias", conv, None, RELU, "level", None, False, None, 2)] + module() + [
        Step("norm", convT, norm, NONE, None, None, False, None, 2)]
    assert match([]) == []


def test_what_is_no_plain_conv_or_norm_runs_as_a_module():
    nobias, norm, act = nn.Conv2d(4, 4, 3, bias=False), nn.InstanceNorm2d(4), nn.LeakyReLU(0.2, True)
    # the convolution is called as it is; the norm behind it is a norm step without a convolution
    assert match([nobias, norm, act]) == module() + [Step("norm", None, norm, LEAKY, "level", None, False, None, 2)]
    reflect, conv = nn.Conv2d(4, 4, 3, padding=1, padding_mode="reflect"), nn.Conv2d(4, 4, 3)
    assert match([reflect, act]) == module(2)
    running = nn.InstanceNorm2d(4, track_running_stats=True)
    assert match([conv, running, act]) == [Step("bias", conv, None, NONE, None, None, False, None, 1)] + module(2)
    assert match([conv, nn.BatchNorm2d(4), act]) == [Step("bias", conv, None, NONE, None, None, False, None, 1)] + module(2)


def test_head_activation_of_a_level():
    conv = nn.Conv2d(4, 4, 3)
    for act, a in ((nn.LeakyReLU(0.2, True), LEAKY), (nn.ReLU(True), RELU)):
        assert match([act, conv, act]) == [Step("head_act", None, None, a, None, None, False, None, 1), Step("bias", conv, None, a, "level", None, False, None, 2)]
    assert match([nn.LeakyReLU(0.2), conv])[0] == module()[0]        # not in place: nobody may absorb it
    assert match([nn.Tanh(), conv])[0] == module()[0]


def _levels():
    B = networks.UnetSkipConnectionBlock
    inner = B(8, 8, None, innermost=True, norm_layer=INSTANCE)                               # ends in a norm of 8 channels
    dropout = B(8, 8, None, submodule=inner, norm_layer=INSTANCE, use_dropout=True)          # ends in Dropout: no tail norm
    return inner, dropout


def test_child_level_behind_a_conv_or_a_norm():
    inner, dropout = _levels()
    conv, norm, relu = nn.Conv2d(3, 8, 4, 2, 1), nn.InstanceNorm2d(8), nn.ReLU(True)
    up = nn.ConvTranspose2d(16, 3, 4, 2, 1)
    assert match([conv, inner, relu, up]) == [Step("bias", conv, None, LEAKY, "child", inner, True, 8, 3),
                                              Step("bias", up, None, NONE, None, None, False, None, 1)]
    assert match([conv, norm, inner, relu, up])[0] == Step("norm", conv, norm, LEAKY, "child", inner, True, 8, 4)
    assert match([conv, dropout, relu, up])[0] == Step("bias", conv, None, LEAKY, "child", dropout, True, None, 3)
    assert match([conv, norm, dropout, relu])[0] == Step("norm", conv, norm, LEAKY, "child", dropout, True, None, 4)
    # no in-place ReLU behind the child: the child's concatenation stays plain, and the ReLU is a module of its own
    assert match([conv, inner, nn.ReLU(), up])[:2] == [Step("bias", conv, None, LEAKY, "child", inner, False, 8, 2)] + module()
    assert match([conv, norm, inner]) == [Step("norm", conv, norm, LEAKY, "child", inner, False, 8, 3)]
    # the steps do not depend on the class-wide switches: skip_source is read when the step runs
    saved = FusedSequential.skip_source
    try:
        FusedSequential.skip_source = False
        assert match([conv, inner, relu, up])[0].c1 == 8
    finally:
        FusedSequential.skip_source = saved


def test_what_is_no_child_level():
    conv, relu = nn.Conv2d(3, 8, 4, 2, 1), nn.ReLU(True)
    outermost = networks.UnetSkipConnectionBlock(3, 8, 3, submodule=_levels()[0], outermost=True, norm_layer=INSTANCE)   # starts with a conv
    assert match([conv, outermost, relu]) == [Step("bias", conv, None, NONE, None, None, False, None, 1)] + module(2)
    plain_seq = nn.Sequential(nn.LeakyReLU(0.2, True), nn.Conv2d(8, 8, 3))      # no `.model` that is a FusedSequential
    assert match([conv, plain_seq, relu]) == [Step("bias", conv, None, NONE, None, None, False, None, 1)] + module(2)


def test_steps_of_the_nets_cover_every_module_once():
    netP = networks.UnetGenerator(3, 3, 6, 8, norm_layer=INSTANCE, use_dropout=True)
    seqs = [m for m in netP.modules() if isinstance(m, FusedSequential)]
    assert len(seqs) == 6
    for seq in seqs:
        steps = match(list(seq))
        assert sum(st.n for st in steps) == len(seq)
        assert [st.kind for st in steps].count("head_act") == (0 if seq is netP.model.model else 1)


def test_a_replaced_child_is_matched_anew():
    """The steps are matched per call and nothing is kept: a sequence whose child was replaced runs the new child."""
    import torch
    import test_fused_trace as ft           # the executor on CPU memory: FakeCuda inputs, the nodes and hipconv replaced by recorders
    seq = FusedSequential(nn.Conv2d(2, 2, 3, padding=1), nn.Tanh())
    x = torch.randn(1, 2, 4, 4)
    before, out = ft.trace(seq, x, engine=True)
    assert [e[0] for e in before] == ["any_engine:Conv2d", "conv_nobias:Conv2d", "_BiasAct", "module:Tanh"] and before[2][2] == "none"
    assert out.min() < 0
    seq[1] = nn.ReLU()
    after, out = ft.trace(seq, x, engine=True)
    assert [e[0] for e in after] == ["conv_nobias:Conv2d", "_BiasAct"] and after[1][2] == "relu" and out.min() == 0
    assert match(list(seq)) == [Step("bias", seq[0], None, RELU, "level", None, False, None, 2)]
