"""Fused conv-bias + InstanceNorm2d + activation for the U-Nets and discriminators (HIP kernels of csrc/instnorm.hip).

The reference builds every level as  Conv2d/ConvTranspose2d(bias) -> InstanceNorm2d -> LeakyReLU(0.2, True) / ReLU(True)
(models/networks.py:220-259, 404-432, 470-497, 507-514), the activation often being the FIRST module of the next
(child) level, applied in place.  On MIOpen that chain is a bias add, a 2-3 pass norm and an activation pass (and as
many again backward, plus a bias-gradient reduction).  `FusedSequential` keeps the module tree — children, names and
therefore state_dict keys are exactly those of nn.Sequential — and only changes HOW a run of such modules is executed:

    conv (called without bias) -> ONE kernel: bias + instance norm + affine + activation      (_InstNormAct)
    conv (called without bias) -> ONE kernel: bias + activation, in place                     (_BiasAct)

The in-place activation at the head of a child level is absorbed into the parent's kernel (the child is then told to skip
it), which is value-identical: the reference's in-place LeakyReLU rewrites the very tensor the parent's norm produced,
so nobody ever sees the un-activated values (that is also why the skip connection carries the activated tensor).

Activations may be fp32 or bf16 (BASELINE config 5 runs the convolutions under bf16 autocast; the kernels then read and
write bf16 and compute in fp32).  CPU tensors, other dtypes, planes above 256x256 (ops.INSTNORM_MAX_PLANE) or above 16384 elements
and not a multiple of 4, and `FusedSequential.enabled = False` take the plain module-by-module path.
"""
from typing import NamedTuple, Optional

import torch
import torch.nn as nn

from .. import ops
from . import hipconv      # conv_nobias / any_engine are looked up on the module at call time (tests replace them there)


def _ticket_words(x, bias):
    """The per-channel arrival counters of the backward's in-launch bias-gradient sum: C words owned by THIS autograd node, zeroed by
    the node's forward launch (csrc/instnorm.hip: the library keeps no device state)."""
    if bias is None or not bias.requires_grad:
        return None
    return torch.empty(x.shape[1], dtype=torch.int32, device=x.device)


def _norm_backward(ctx, dy, act, slope, **dy2):
    """The backward the four norm nodes share -> (dx, dbias, dgamma, dbeta), the gradients of their first four inputs.  Each saves
    (x, bias, gamma, y, mean, rstd, tickets); dy and y may be the wide concatenated tensors, read in place; dy2 / dy2_at: the
    gradient of a second, relu'd output."""
    x, bias, gamma, y, mean, rstd, tickets = ctx.saved_tensors
    need_bias = bias is not None and ctx.needs_input_grad[1]
    need_affine = ctx.has_affine and (ctx.needs_input_grad[2] or ctx.needs_input_grad[3])
    dx, dg, db, dbias = ops.instnorm_act_backward(dy, y, x, bias, gamma, mean, rstd, act, slope, need_affine, need_bias, tickets=tickets, **dy2)
    return dx, dbias, dg, db


class _InstNormAct(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, bias, gamma, beta, eps, act, slope):
        y, mean, rstd, tickets = ops.instnorm_act_forward(x, bias, gamma, beta, eps, act, slope, return_tickets=True)
        ctx.save_for_backward(x, bias, gamma, y, mean, rstd, tickets)
        ctx.act, ctx.slope = act, slope
        ctx.has_affine = gamma is not None
        return y

    @staticmethod
    def backward(ctx, dy):
        return _norm_backward(ctx, dy, ctx.act, ctx.slope) + (None, None, None)


class _BiasAct(torch.autograd.Function):
    """act(x + bias[c]) in place on x (a fresh convolution output nobody else holds)."""

    @staticmethod
    def forward(ctx, x, bias, act, slope):
        tickets = _ticket_words(x, bias)
        ops.bias_act_(x, bias, act, slope, tickets=tickets)
        ctx.mark_dirty(x)
        ctx.save_for_backward(x, tickets)
        ctx.act, ctx.slope = act, slope
        ctx.has_bias = bias is not None
        return x

    @staticmethod
    def backward(ctx, dy):
        y, tickets = ctx.saved_tensors
        dx, dbias = ops.bias_act_backward(dy, y, ctx.act, ctx.slope, ctx.has_bias and ctx.needs_input_grad[1], tickets=tickets)
        return dx, dbias, None, None


class _BiasActSkip(torch.autograd.Function):
    """_BiasAct with a second output: relu(x + bias) written into the skip half of the child level's concatenated tensor (allocated
    here); backward dx = dy * act'(y) + dbuf[:, c1:] * relu'(y).  The level-1 blocks, whose input comes from a convolution alone."""

    @staticmethod
    def forward(ctx, x, bias, act, slope, c1):
        B, C2 = x.shape[0], x.shape[1]
        buf = torch.empty((B, c1 + C2) + tuple(x.shape[2:]), dtype=x.dtype, device=x.device)
        tickets = _ticket_words(x, bias)
        ops.bias_act_(x, bias, act, slope, relu_into=buf, relu_at=c1, tickets=tickets)
        ctx.mark_dirty(x)
        ctx.save_for_backward(x, tickets)
        ctx.act, ctx.slope, ctx.c1 = act, slope, c1
        ctx.has_bias = bias is not None
        return x, buf

    @staticmethod
    def backward(ctx, dy, dbuf):
        y, tickets = ctx.saved_tensors
        if dy is None:
            dy = torch.zeros_like(y)
        dx, dbias = ops.bias_act_backward(dy.contiguous(), y, ctx.act, ctx.slope, ctx.has_bias and ctx.needs_input_grad[1],
                                          dy2=None if dbuf is None else dbuf.contiguous(), dy2_at=ctx.c1, tickets=tickets)
        return dx, dbias, None, None, None


class _CatReLU(torch.autograd.Function):
    """relu(cat([y, x], 1)): the skip concatenation of a level followed by the parent's in-place ReLU."""

    @staticmethod
    def forward(ctx, y, x):
        out = ops.cat_relu_forward(y, x)
        ctx.save_for_backward(out)
        ctx.c1 = y.size(1)
        return out

    @staticmethod
    def backward(ctx, g):
        (out,) = ctx.saved_tensors
        return ops.cat_relu_backward(g, out, ctx.c1)


class _InstNormReLUCat(torch.autograd.Function):
    """relu(cat([InstanceNorm(y + bias) * gamma + beta, x], 1)) — a level's last norm, its skip concatenation and the parent's in-place
    ReLU as ONE node: the norm kernel writes its half straight into the concatenated tensor (and its backward reads the gradient's
    slice in place); only the skip half is left to the concatenation kernels."""

    @staticmethod
    def forward(ctx, y, bias, gamma, beta, eps, x):
        B, C1, C2 = y.shape[0], y.shape[1], x.shape[1]
        out = torch.empty((B, C1 + C2) + tuple(y.shape[2:]), dtype=y.dtype, device=y.device)
        _, mean, rstd, tickets = ops.instnorm_act_forward(y, bias, gamma, beta, eps, "relu", 0.0, into=out, return_tickets=True)
        ops.cat_relu_skip_half_(out, x)
        ctx.save_for_backward(y, bias, gamma, out, mean, rstd, tickets)
        ctx.c1 = C1
        ctx.has_affine = gamma is not None
        return out

    @staticmethod
    def backward(ctx, g):
        g = g.contiguous()
        grads = _norm_backward(ctx, g, "relu", 0.0)
        _, dx = ops.cat_relu_backward(g, ctx.saved_tensors[3], ctx.c1, skip_half_only=True)
        return grads + (None, dx)


class _InstNormActSkip(torch.autograd.Function):
    """The norm that produces a level's input, with TWO outputs: act(norm) for the level's down path and relu(norm) written straight
    into the skip half of the level's concatenated tensor (allocated here, completed by _InstNormReLUCatInto at the level's end).
    Backward: the two consumers' gradients meet inside the norm's backward kernel (no add kernel, no slice copy)."""

    @staticmethod
    def forward(ctx, y, bias, gamma, beta, eps, act, slope, c1):
        B, C2 = y.shape[0], y.shape[1]
        buf = torch.empty((B, c1 + C2) + tuple(y.shape[2:]), dtype=y.dtype, device=y.device)
        x_act, mean, rstd, tickets = ops.instnorm_act_forward(y, bias, gamma, beta, eps, act, slope, relu_into=buf, relu_at=c1, return_tickets=True)
        ctx.save_for_backward(y, bias, gamma, x_act, mean, rstd, tickets)
        ctx.act, ctx.slope, ctx.c1 = act, slope, c1
        ctx.has_affine = gamma is not None
        return x_act, buf

    @staticmethod
    def backward(ctx, g_x, g_buf):
        if g_x is None:
            g_x = torch.zeros_like(ctx.saved_tensors[3])
        return _norm_backward(ctx, g_x.contiguous(), ctx.act, ctx.slope, dy2=None if g_buf is None else g_buf.contiguous(),
                              dy2_at=ctx.c1) + (None, None, None, None)


class _InstNormReLUCatInto(torch.autograd.Function):
    """_InstNormReLUCat into a concatenated tensor whose skip half is already there (written by _InstNormActSkip): the first C1
    channels of `buf` receive relu(norm(y)); the gradient of `buf` is handed back whole (its producer reads the skip half in place)."""

    @staticmethod
    def forward(ctx, y, bias, gamma, beta, eps, buf):
        _, mean, rstd, tickets = ops.instnorm_act_forward(y, bias, gamma, beta, eps, "relu", 0.0, into=buf, into_at=0, return_tickets=True)
        ctx.mark_dirty(buf)
        ctx.save_for_backward(y, bias, gamma, buf, mean, rstd, tickets)
        ctx.has_affine = gamma is not None
        return buf

    @staticmethod
    def backward(ctx, g):
        g = g.contiguous()
        return _norm_backward(ctx, g, "relu", 0.0) + (None, g)


def _fusable(*tensors):
    """What the kernels read and write: contiguous fp32 / bf16 (not e.g. channels_last)."""
    return all(t.is_contiguous() and t.dtype in (torch.float32, torch.bfloat16) for t in tensors)


def cat_skip(y, x, tail_relu):
    """torch.cat([y, x], 1), with the consumer's in-place ReLU folded in when it asked for that."""
    if tail_relu and y.is_cuda and _fusable(y, x) and y.dtype == x.dtype and y.shape[2:] == x.shape[2:]:
        return _CatReLU.apply(y, x)
    out = torch.cat([y, x], 1)
    return torch.relu_(out) if tail_relu else out


# ----------------------------------------------------------------------------------------------------
# matching: what the module list alone decides
# ----------------------------------------------------------------------------------------------------
def _act_of(m):
    """(name, slope) when m is an activation the kernels implement."""
    if isinstance(m, nn.LeakyReLU):
        return "leaky", float(m.negative_slope)
    if isinstance(m, nn.ReLU):
        return "relu", 0.0
    return None


def _plain_conv(m):
    return type(m) in (nn.Conv2d, nn.ConvTranspose2d) and m.bias is not None and getattr(m, "padding_mode", "zeros") == "zeros"


def _plain_inorm(m):
    return isinstance(m, nn.InstanceNorm2d) and not m.track_running_stats


def _head_act_of_child(m):
    """A skip level whose first module is an in-place activation can have it absorbed by the producer."""
    inner = getattr(m, "model", None)
    if isinstance(inner, FusedSequential) and len(inner) > 0 and getattr(inner[0], "inplace", False):
        return _act_of(inner[0])
    return None


def _tail_norm_channels(block):
    """Output channels of a skip level whose sequence ends in a plain InstanceNorm (then the level can complete a concatenated tensor
    its producer allocated), else None."""
    inner = getattr(block, "model", None)
    if getattr(block, "outermost", True) or not isinstance(inner, FusedSequential) or len(inner) == 0 or not _plain_inorm(inner[-1]):
        return None
    return int(inner[-1].num_features)


class Step(NamedTuple):
    """One step of a sequence: `n` consecutive modules and how they run."""
    kind: str                   # "bias": conv -> bias kernel | "norm": [conv ->] norm kernel | "module": the module itself |
                                # "head_act": the leading in-place activation, the module itself unless the producer absorbed it
    conv: Optional[nn.Module]   # the convolution called without its bias (a norm step may have none)
    norm: Optional[nn.Module]
    act: Optional[tuple]        # (name, slope) the kernel applies; ("none", 0.0) where nothing fusable follows
    act_of: Optional[str]       # whose activation that is: "level" (the next module), "child" (the head of the child level), None
    child: Optional[nn.Module]  # the skip block entered with its head activation done
    tail_relu: bool             # the in-place ReLU behind the child is applied by the child's concatenation
    c1: Optional[int]           # _tail_norm_channels(child): the child can complete a concatenated tensor this step allocates
    n: int


def match(mods):
    """The steps of a module list; a pure function of the modules (no tensor is looked at)."""
    steps, i = [], 0
    while i < len(mods):
        m = mods[i]
        conv = m if _plain_conv(m) else None
        j = i + (conv is not None)
        norm = mods[j] if j < len(mods) and _plain_inorm(mods[j]) else None
        j += norm is not None
        if j == i:
            head = i == 0 and getattr(m, "inplace", False) and _act_of(m) is not None
            step = Step("head_act", None, None, _act_of(m), None, None, False, None, 1) if head else Step("module", None, None, None, None, None, False, None, 1)
        else:
            nxt = mods[j] if j < len(mods) else None            # what follows the conv / norm: this level's activation, a child level, or neither
            act, act_of, child, tail, c1 = _act_of(nxt), "level", None, False, None
            if act is None:
                act, act_of = _head_act_of_child(nxt), "child"
            if act is None:
                act, act_of = ("none", 0.0), None
            elif act_of == "child":
                # the in-place ReLU a skip level's concatenated output runs into (models/networks.py:229,408)
                tail = j + 1 < len(mods) and type(mods[j + 1]) is nn.ReLU and mods[j + 1].inplace
                child, c1 = nxt, _tail_norm_channels(nxt)
            step = Step("bias" if norm is None else "norm", conv, norm, act, act_of, child, tail, c1, j - i + (act_of is not None) + tail)
        steps.append(step)
        i += step.n
    return steps


# ----------------------------------------------------------------------------------------------------
# execution: what the tensors decide
# ----------------------------------------------------------------------------------------------------
def _fits_norm_kernel(y):
    hw = y.size(2) * y.size(3)
    return 2 <= hw <= ops.INSTNORM_MAX_PLANE and not (hw > 16384 and hw % 4)


def _plain_modules(st, y, rest):
    """The step by torch where the kernels cannot take y (e.g. channels_last, too large for the plane-in-registers kernel)."""
    dt = y.dtype
    if st.norm is None:
        x = y + st.conv.bias.view(1, -1, 1, 1).to(dt)
    else:
        if st.conv is not None:
            y = y + st.conv.bias.view(1, -1, 1, 1)
        # torch's own kernels, not MIOpen's batch norm (its backward put dx 30 % and dgamma 2 % off on 145x113 planes),
        # and in fp32: bf16 activations are normalised in fp32 and stay bf16
        with torch.backends.cudnn.flags(enabled=False):
            x = st.norm(y.float()).to(dt) if dt == torch.bfloat16 else st.norm(y)
    for m in rest:
        x = m(x)
    return x


def _into_child(st, node, skip_node, *args):
    """Hand node(*args) to the child level: with FusedSequential.skip_source, and where the child can complete it, the skip-source form
    of the node also writes the skip half of the child's concatenated tensor."""
    if st.tail_relu and FusedSequential.skip_source and st.c1:
        x, buf = skip_node.apply(*args, st.c1)
    else:
        x, buf = node.apply(*args), None
    return st.child(x, head_act_done=True, tail_relu=st.tail_relu, cat_buf=buf)


class FusedSequential(nn.Sequential):
    enabled = True          # class-wide switch (Option.fused_norm_act); False = behave exactly like nn.Sequential
    skip_source = True      # A/B switch (tests): False = a level's producer does NOT write the skip half of the child's concatenated tensor
                            # (no _InstNormActSkip / _BiasActSkip nodes: the child concatenates, autograd adds the two input gradients)

    def _get_name(self):    # prints like the reference's module tree (train.ipynb cell 1 output)
        return 'Sequential'

    def forward(self, x, level=None):
        """seq(x): the tensor, as nn.Sequential.  seq(x, level=(head_act_done, cat_with, cat_buf)), the call of the skip blocks
        (networks._SkipBlock): always (tensor, concatenated).  head_act_done: the producer of x applied this level's leading in-place
        activation; cat_with: the level's input, when the caller wants relu(cat([this(x), cat_with], 1)) — a sequence that ends in a
        norm produces it itself and says so; cat_buf: that concatenated tensor with its skip half already written."""
        if level is None:
            return self._run(x, False, None, None)[0]
        return self._run(x, *level)

    def _run(self, x, head_act_done, cat_with, cat_buf):
        mods = list(self)
        i = 0
        if head_act_done:                       # the producer already applied this level's leading in-place activation
            assert mods and _act_of(mods[0]) is not None
            i = 1
        if not (FusedSequential.enabled and x.is_cuda and x.dtype in (torch.float32, torch.bfloat16)):
            for m in mods[i:]:
                x = m(x)
            return x, False
        for st in match(mods)[i:]:              # an activation at the head is a step of its own
            first, i = i, i + st.n
            conv, norm = st.conv, st.norm
            if conv is None and norm is None:
                x = mods[first](x)
                continue
            if conv is None:
                y = x
            elif st.kind == "bias" and st.act_of is None and not hipconv.any_engine(conv, x):
                # conv -> something the kernels do not fuse (Tanh of the outermost level, a loss): the plain module, unless a HIP
                # engine takes one of its passes (netG's last ConvTranspose2d 128 -> 3 @256x256: 0.13 vs 0.24 ms forward) — then
                # the bias is split off and added (with its gradient as a by-product) by the bias kernel
                x = conv(x)
                continue
            else:
                y = hipconv.conv_nobias(conv, x)
            if not _fusable(y) or (norm is not None and not _fits_norm_kernel(y)):
                x = _plain_modules(st, y, mods[first + (conv is not None) + (norm is not None):i])
                continue
            if norm is None:
                node, skip_node, args = _BiasAct, _BiasActSkip, (y, conv.bias)
            else:
                node, skip_node, args = _InstNormAct, _InstNormActSkip, (y, conv.bias if conv is not None else None, norm.weight, norm.bias, norm.eps)
                if i == len(mods) and st.act_of is None and cat_with is not None and cat_with.is_contiguous() and cat_with.dtype == y.dtype \
                        and cat_with.shape[0] == y.shape[0] and cat_with.shape[2:] == y.shape[2:]:
                    # the level ends here: norm + skip concatenation + the parent's ReLU in one node
                    if cat_buf is not None and cat_buf.dtype == y.dtype and cat_buf.shape[0] == y.shape[0] and cat_buf.shape[2:] == y.shape[2:] \
                            and cat_buf.shape[1] == y.shape[1] + cat_with.shape[1]:
                        return _InstNormReLUCatInto.apply(*args, cat_buf), True
                    return _InstNormReLUCat.apply(*args, cat_with), True
            x = node.apply(*args, *st.act) if st.child is None else _into_child(st, node, skip_node, *args, *st.act)
        return x, False
