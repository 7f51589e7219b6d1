"""Which fused node every level of the four nets gets: the call sequence of `models/fused.py`, pinned on the CPU.

`FusedSequential` decides per level which HIP node runs between the convolutions.  The value tests (`test_gpu_model.py`) would
still pass if a level silently fell back to the plain modules or lost its skip-source node, so this file pins the DECISIONS:
the ordered list of node applications, bias-free convolution calls, `any_engine` questions, plain-module calls and plain
`torch.cat` / `torch.relu_` calls of a forward pass equals `tests/golden/fused_trace.json`, for every net, with `skip_source`
on and off, with `any_engine` answering no and yes, and for the run-time fallbacks.

How it runs without a GPU or the library: the inputs are a `torch.Tensor` subclass whose `is_cuda` is True (so the fused path
is taken on CPU memory); `apply` of the seven node classes, `hipconv.conv_nobias` and `hipconv.any_engine` are replaced by
recorders that return the same expression by plain torch.  So the traced output must also EQUAL the plain-module output of
the same net (`FusedSequential.enabled = False`): a lost activation, a lost norm or a doubled ReLU moves it by 1e-1, the
fakes' rounding by 1e-6; the bound is 1e-5.

    python tests/test_fused_trace.py --record      # rewrites the fixture from the tree it runs in; states that tree's commit
"""
import contextlib
import io
import json
import os
import sys

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from deepinpainting_amd.models import fused, hipconv, networks  # noqa: E402
from deepinpainting_amd.models.fused import FusedSequential  # noqa: E402
from deepinpainting_amd.options import Option  # noqa: E402

FIXTURE = os.path.join(ROOT, "tests", "golden", "fused_trace.json")
NODES = ("_InstNormAct", "_BiasAct", "_BiasActSkip", "_CatReLU", "_InstNormReLUCat", "_InstNormActSkip", "_InstNormReLUCatInto")
INSTANCE = networks.get_norm_layer('instance')
_cat, _relu_ = torch.cat, torch.relu_


class FakeCuda(torch.Tensor):
    """CPU memory that says it is on the GPU; every torch function of one returns one."""
    is_cuda = property(lambda self: True)


def fake(t):
    return t.as_subclass(FakeCuda)


def _act(v, act, slope):
    return {"none": lambda: v, "relu": lambda: torch.relu(v), "leaky": lambda: F.leaky_relu(v, slope)}[act]()


def _norm(y, bias, gamma, beta, eps):
    v = y.float() if bias is None else y.float() + bias.float().view(1, -1, 1, 1)
    return F.instance_norm(v, weight=gamma, bias=beta, eps=eps)


def _skip_buf(v, c1):
    buf = v.new_zeros((v.shape[0], c1 + v.shape[1]) + tuple(v.shape[2:]))
    buf[:, c1:] = torch.relu(v)
    return buf


class Tracer:
    """Replaces the nodes and the two hipconv entry points by recorders while active; `log` is the trace."""

    def __init__(self, engine=False, noncontig_conv=False):
        self.log, self.engine, self.noncontig_conv = [], engine, noncontig_conv

    def rec(self, name, tensors, act=None, slope=None, c1=None):
        self.log.append([name, [list(t.shape) for t in tensors], act, slope, c1])

    # --- the seven nodes: [class name, input shapes, act, slope, c1] and the plain-torch value ---
    def _InstNormAct(self, x, bias, gamma, beta, eps, act, slope):
        self.rec("_InstNormAct", [x], act, slope)
        return fake(_act(_norm(x, bias, gamma, beta, eps), act, slope).to(x.dtype))

    def _BiasAct(self, x, bias, act, slope):
        self.rec("_BiasAct", [x], act, slope)
        return fake(_act(x + bias.view(1, -1, 1, 1).to(x.dtype), act, slope))

    def _BiasActSkip(self, x, bias, act, slope, c1):
        self.rec("_BiasActSkip", [x], act, slope, c1)
        v = x + bias.view(1, -1, 1, 1).to(x.dtype)
        return fake(_act(v, act, slope)), fake(_skip_buf(v, c1))

    def _CatReLU(self, y, x):
        self.rec("_CatReLU", [y, x], c1=y.shape[1])
        return fake(torch.relu(_cat([y, x], 1)))

    def _InstNormReLUCat(self, y, bias, gamma, beta, eps, x):
        self.rec("_InstNormReLUCat", [y, x], c1=y.shape[1])
        return fake(torch.relu(_cat([_norm(y, bias, gamma, beta, eps).to(y.dtype), x], 1)))

    def _InstNormActSkip(self, y, bias, gamma, beta, eps, act, slope, c1):
        self.rec("_InstNormActSkip", [y], act, slope, c1)
        v = _norm(y, bias, gamma, beta, eps).to(y.dtype)
        return fake(_act(v, act, slope)), fake(_skip_buf(v, c1))

    def _InstNormReLUCatInto(self, y, bias, gamma, beta, eps, buf):
        self.rec("_InstNormReLUCatInto", [y, buf], c1=y.shape[1])
        out = buf.clone()
        out[:, :y.shape[1]] = torch.relu(_norm(y, bias, gamma, beta, eps).to(y.dtype))
        return fake(out)

    # --- hipconv ---
    def conv_nobias(self, m, x, weight=None):
        self.rec("conv_nobias:" + type(m).__name__, [x, m.weight])
        w = m.weight if weight is None else weight
        if isinstance(m, nn.ConvTranspose2d):
            y = F.conv_transpose2d(x, w, None, m.stride, m.padding, m.output_padding, m.groups, m.dilation)
        else:
            y = F.conv2d(x, w, None, m.stride, m.padding, m.dilation, m.groups)
        if self.noncontig_conv:
            y = y.contiguous(memory_format=torch.channels_last)
            assert not y.is_contiguous()
        return fake(y)

    def any_engine(self, m, x):
        self.rec("any_engine:" + type(m).__name__, [x, m.weight])
        return self.engine.pop(0) if isinstance(self.engine, list) else self.engine      # a list: one answer per question

    # --- everything that is not a node: leaf-module calls, torch.cat, torch.relu_ ---
    def _module_hook(self, mod, inp, out):
        self.rec("module:" + type(mod).__name__, [t for t in inp if torch.is_tensor(t)])

    def _torch_cat(self, tensors, dim=0):
        self.rec("torch.cat", tensors)
        return _cat(tensors, dim)

    def _torch_relu_(self, t):
        self.rec("torch.relu_", [t])
        return _relu_(t)

    @contextlib.contextmanager
    def on(self, net):
        saved_conv = (hipconv.conv_nobias, hipconv.any_engine)
        hooks = [m.register_forward_hook(self._module_hook) for m in net.modules() if not list(m.children())]
        try:
            for n in NODES:
                getattr(fused, n).apply = getattr(self, n)
            hipconv.conv_nobias, hipconv.any_engine = self.conv_nobias, self.any_engine
            torch.cat, torch.relu_ = self._torch_cat, self._torch_relu_
            yield self
        finally:
            torch.cat, torch.relu_ = _cat, _relu_
            hipconv.conv_nobias, hipconv.any_engine = saved_conv
            for n in NODES:
                delattr(getattr(fused, n), "apply")      # back to the inherited Function.apply
            for h in hooks:
                h.remove()


@contextlib.contextmanager
def switches(enabled=True, skip_source=True):
    saved = FusedSequential.enabled, FusedSequential.skip_source
    FusedSequential.enabled, FusedSequential.skip_source = enabled, skip_source
    try:
        yield
    finally:
        FusedSequential.enabled, FusedSequential.skip_source = saved


def trace(net, x, skip_source=True, engine=False, call=None, raises=None, **tracer_args):
    """(trace, output) of one forward pass of `net` (or of `call(net, x)`) on a FakeCuda copy of x.  `raises`: the exception the
    pass must end in (the trace then ends in a "raises:" entry and the output is None); any other exception is an error."""
    t = Tracer(engine, **tracer_args)
    with torch.no_grad(), switches(True, skip_source), t.on(net):
        if raises is None:
            return t.log, (call or (lambda n, v: n(v)))(net, fake(x.clone())).as_subclass(torch.Tensor)
        with pytest.raises(raises):
            net(fake(x.clone()))
    t.log.append(["raises:" + raises.__name__, [], None, None, None])
    return t.log, None


def plain(net, x, call=None):
    with torch.no_grad(), switches(enabled=False):
        return (call or (lambda n, v: n(v)))(net, x.clone())


# ---------------------------------------------------------------------------------------------------------------------
# the nets
# ---------------------------------------------------------------------------------------------------------------------
def _seeded(build, seed):
    torch.manual_seed(seed)
    with contextlib.redirect_stdout(io.StringIO()):
        net = build()
    return net.eval()


def build_netG():
    """netG at ngf 8 on 64x64 with the attention layer and the two loss taps stubbed to pass their input through (they are
    recorded as plain-module calls)."""
    from oracle import cpu_model
    mask = torch.zeros(1, 1, 64, 64, dtype=torch.bool)
    mask[:, :, 16:48, 16:48] = 1
    with cpu_model.oracle_layers():
        net = networks.UnetGeneratorIPSR(6, 3, 5, Option(fineSize=64), mask, [], [], [], ngf=8, norm_layer=INSTANCE, use_dropout=True)
    for m in net.modules():
        if isinstance(m, (cpu_model.OracleIPSRModel, cpu_model.OracleInnerCos)):
            m.forward = lambda x: x
    return net


def nets():
    """name -> (net, input).  Built once per process (`NETS`)."""
    g = torch.Generator().manual_seed(11)
    x3 = torch.rand(2, 3, 64, 64, generator=g) * 2 - 1
    return {
        "netP_dropout": (_seeded(lambda: networks.UnetGenerator(3, 3, 6, 8, norm_layer=INSTANCE, use_dropout=True), 1), x3),
        "netP": (_seeded(lambda: networks.UnetGenerator(3, 3, 6, 8, norm_layer=INSTANCE, use_dropout=False), 2), x3),
        "netD": (_seeded(lambda: networks.NLayerDiscriminator(3, 8, 3, norm_layer=INSTANCE), 3), x3),
        "netF": (_seeded(networks.PFDiscriminator, 4), torch.rand(1, 256, 16, 16, generator=g) * 2 - 1),
        "netG": (_seeded(build_netG, 5), torch.rand(2, 6, 64, 64, generator=g) * 2 - 1),
    }


# ---------------------------------------------------------------------------------------------------------------------
# the run-time fallbacks, as small sequences
# ---------------------------------------------------------------------------------------------------------------------
def _level(x, cat_buf):
    return lambda blk, v: blk(v, head_act_done=True, tail_relu=True, cat_buf=None if cat_buf is None else fake(cat_buf))


def fallbacks():
    """name -> (module, input, call or None, tracer arguments)."""
    g = torch.Generator().manual_seed(12)
    rnd = lambda *s: torch.rand(*s, generator=g) * 2 - 1  # noqa: E731
    conv_norm_act = lambda c: FusedSequential(nn.Conv2d(c, c, 3, padding=1), nn.InstanceNorm2d(c), nn.LeakyReLU(0.2, True))  # noqa: E731
    innermost = _seeded(lambda: networks.UnetSkipConnectionBlock(4, 6, None, innermost=True, norm_layer=INSTANCE), 21)
    x_in = torch.relu(rnd(2, 4, 8, 8))
    cases = {
        "plane_above_limit": (conv_norm_act(4), rnd(1, 4, 260, 256), None, {}),
        "plane_above_16384_not_x4": (conv_norm_act(2), rnd(1, 2, 130, 127), None, {}),
        # torch's own refusal of a one-element plane, which the fused path must leave to torch
        "plane_of_one": (conv_norm_act(3), rnd(2, 3, 1, 1), None, dict(raises=ValueError)),
        "bf16": (conv_norm_act(4).bfloat16(), rnd(2, 4, 8, 8).bfloat16(), None, {}),
        "float64": (conv_norm_act(4).double(), rnd(2, 4, 8, 8).double(), None, {}),
        "noncontig_conv_norm": (conv_norm_act(4), rnd(2, 4, 8, 8), None, dict(noncontig_conv=True)),
        "noncontig_conv_act": (FusedSequential(nn.Conv2d(4, 4, 3, padding=1), nn.LeakyReLU(0.2, True)), rnd(2, 4, 8, 8), None,
                               dict(noncontig_conv=True)),
        "noncontig_conv_alone": (FusedSequential(nn.Conv2d(4, 4, 3, padding=1), nn.Tanh()), rnd(2, 4, 8, 8), None,
                                 dict(noncontig_conv=True, engine=True)),
        # a level that ends in a norm, entered the way its producer enters it: with the concatenated tensor ...
        "cat_buf_fits": (innermost, x_in, _level(x_in, _skip_buf(x_in, 4)), {}),
        # ... with one of the wrong channel count (the level then concatenates by itself), and with none
        "cat_buf_wrong_channels": (innermost, x_in, _level(x_in, _skip_buf(x_in, 5)), {}),
        "cat_buf_none": (innermost, x_in, _level(x_in, None), {}),
    }
    for seed, (m, _, _, _) in enumerate(cases.values()):
        torch.manual_seed(40 + seed)
        for p in m.parameters():
            nn.init.normal_(p, 0.0, 0.3)
        m.eval()
    return cases


def _plain_level(blk, v):
    """What the producer's absorbed activation and the consumer's ReLU amount to for a level entered with head_act_done /
    tail_relu: the plain block runs its own leading activation (an in-place LeakyReLU; the input is >= 0, so it changes nothing)."""
    return torch.relu(blk(v))


def all_traces():
    """name -> trace, and name -> (traced output, plain output), over every net, switch setting and fallback."""
    traces, outputs = {}, {}
    for name, (net, x) in NETS().items():
        ref = plain(net, x)
        for skip_source in (True, False):
            for engine in (False, True):
                key = "%s/skip_source=%d/any_engine=%d" % (name, skip_source, engine)
                traces[key], out = trace(net, x, skip_source, engine)
                outputs[key] = (out, ref)
    for name, (m, x, call, targs) in fallbacks().items():
        traces["fallback/" + name], out = trace(m, x, call=call, **targs)
        if out is None:
            with pytest.raises(ValueError):
                plain(m, x)
        elif out.dtype != torch.bfloat16:     # bf16: the plain modules round after every module, the nodes once; only the trace is pinned
            outputs["fallback/" + name] = (out, plain(m, x, _plain_level if call else None))
    return traces, outputs


_NETS = None


def NETS():
    global _NETS
    if _NETS is None:
        _NETS = nets()
    return _NETS


@pytest.fixture(scope="module")
def traced():
    return all_traces()


def names_of(trace_, prefix="_"):
    names = [e if isinstance(e, str) else e[0] for e in trace_]
    return [n for n in names if n.startswith(prefix)]


def test_trace_equals_the_recorded_fixture(traced):
    with open(FIXTURE) as f:
        golden = json.load(f)
    assert golden["recorded_at_commit"]
    traces = json.loads(json.dumps(traced[0]))
    assert sorted(traces) == sorted(golden["traces"])
    for key in golden["traces"]:
        assert traces[key] == golden["traces"][key], "the call sequence of %s changed" % key


def test_traced_output_equals_plain_modules(traced):
    for key, (out, ref) in traced[1].items():
        err = (out.double() - ref.double()).abs().max().item()
        print("%-48s max |traced - plain| = %.3g" % (key, err))
        assert out.shape == ref.shape and err <= 1e-5, (key, err)


def test_trace_holds_the_nodes_the_design_names(traced):
    """The fixture is only worth something if the nets reach the interesting nodes at these sizes."""
    t = traced[0]
    P, G = t["netP_dropout/skip_source=1/any_engine=0"], t["netG/skip_source=1/any_engine=0"]
    assert names_of(P)[0] == "_BiasActSkip" and names_of(G)[0] == "_BiasActSkip"
    assert names_of(P).count("_InstNormActSkip") == 3 and names_of(P).count("_InstNormReLUCatInto") == 4
    assert names_of(G).count("_InstNormActSkip") == 3 and names_of(G).count("_InstNormReLUCatInto") == 4
    # the dropout level: its norm without activation, the dropout, then the concatenation (netG's: plain, below the attention level)
    for T, cat in ((P, "_CatReLU"), (G, "torch.cat")):
        i = [e[0:1] + e[2:3] for e in T].index(["_InstNormAct", "none"])
        assert [e[0] for e in T[i + 1:i + 3]] == ["module:Dropout", cat]
    assert [e[0] for e in G if e[0].startswith("any_engine")] == ["any_engine:Conv2d", "any_engine:ConvTranspose2d"]
    assert G[[e[0] for e in G].index("any_engine:Conv2d") + 2][0] == "module:OracleIPSRModel"          # the conv in front of the attention layer
    for n in ("netP", "netD", "netF", "netG"):                                                         # the last conv of each net
        names = [e[0] for e in t[n + "/skip_source=1/any_engine=0"]]
        assert names.index(names_of(names, "any_engine")[-1]) > max(i for i, v in enumerate(names) if v.startswith("conv_nobias"))
        assert names_of(t[n + "/skip_source=1/any_engine=1"])[-1:] == ["_BiasAct"]
    off = t["netP_dropout/skip_source=0/any_engine=0"]
    assert not {"_BiasActSkip", "_InstNormActSkip", "_InstNormReLUCatInto"} & set(names_of(off)) and "_InstNormReLUCat" in names_of(off)
    assert names_of(t["fallback/cat_buf_fits"]) == ["_BiasAct", "_InstNormReLUCatInto"]
    assert names_of(t["fallback/cat_buf_wrong_channels"]) == names_of(t["fallback/cat_buf_none"]) == ["_BiasAct", "_InstNormReLUCat"]
    for k in ("plane_above_limit", "plane_above_16384_not_x4", "plane_of_one", "float64", "noncontig_conv_norm"):
        assert names_of(t["fallback/" + k]) == [], k
    assert names_of(t["fallback/bf16"]) == ["_InstNormAct"]


if __name__ == "__main__":
    if sys.argv[1:] != ["--record"]:
        sys.exit(__doc__)
    import subprocess
    commit = subprocess.check_output(["git", "-C", ROOT, "rev-parse", "HEAD"], text=True).strip()
    dirty = subprocess.check_output(["git", "-C", ROOT, "status", "--porcelain", "--", "deepinpainting_amd"], text=True).strip()
    assert not dirty, "record from a tree whose product code is the commit's:\n" + dirty
    with open(FIXTURE, "w") as f:      # one trace entry per line
        f.write('{"recorded_at_commit": "%s",\n"traces": {\n' % commit)
        f.write(",\n".join('"%s": [\n%s\n]' % (k, ",\n".join(json.dumps(e) for e in t)) for k, t in all_traces()[0].items()))
        f.write("\n}}\n")
    print("recorded %s at %s" % (FIXTURE, commit))
