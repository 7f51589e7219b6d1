"""The node sequence of `models/fused.py` on the real kernels equals what the CPU technique of tests/test_fused_trace.py gives
for the same nets: the fakes of that file hide no path that only real CUDA tensors take."""
import contextlib

import pytest
import torch

import test_fused_trace as ft
from deepinpainting_amd.models import fused, hipconv, networks

pytestmark = pytest.mark.gpu


@contextlib.contextmanager
def recorded_nodes(log, answers):
    """`apply` of the seven node classes records [class name, act, c1] and calls through to the real node; `answers`: what the real
    `hipconv.any_engine` said, in order (the CPU trace is then given the same answers)."""
    def recorder(cls):
        real = cls.apply
        where = {"_InstNormAct": (5, None), "_BiasAct": (2, None), "_BiasActSkip": (2, 4), "_InstNormActSkip": (5, 7)}.get(cls.__name__, (None, None))

        def apply(*args):
            act, c1 = (None if i is None else args[i] for i in where)
            log.append([cls.__name__, act, args[0].shape[1] if where == (None, None) else c1])
            return real(*args)
        return apply
    real_any_engine = hipconv.any_engine

    def any_engine(m, x):
        answers.append(real_any_engine(m, x))
        return answers[-1]
    try:
        for n in ft.NODES:
            setattr(getattr(fused, n), "apply", recorder(getattr(fused, n)))
        hipconv.any_engine = any_engine
        yield
    finally:
        hipconv.any_engine = real_any_engine
        for n in ft.NODES:
            delattr(getattr(fused, n), "apply")


@pytest.mark.parametrize("skip_source", [True, False])
def test_real_nodes_follow_the_cpu_trace(skip_source):
    norm = networks.get_norm_layer('instance')
    torch.manual_seed(11)
    nets = [networks.UnetGenerator(3, 3, 5, 16, norm_layer=norm, use_dropout=False), networks.NLayerDiscriminator(3, 16, 3, norm_layer=norm)]
    x = torch.rand(2, 3, 64, 64) * 2 - 1
    for net in nets:
        net.eval()
        gpu, answers = [], []
        net.cuda()
        with torch.no_grad(), ft.switches(True, skip_source), recorded_nodes(gpu, answers):
            net(x.cuda())
        torch.cuda.synchronize()
        net.cpu()
        cpu = [[e[0], e[2], e[4]] for e in ft.trace(net, x, skip_source, engine=answers)[0] if e[0] in ft.NODES]
        assert len(gpu) >= 4 and gpu == cpu and answers == []
