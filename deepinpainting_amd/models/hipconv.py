"""Convolutions of the four nets and of VGG16 on the hand-written HIP kernels, behind nn.Conv2d /
nn.ConvTranspose2d modules whose parameters, names and state_dict keys are untouched (models/networks.py:220-259,
404-432, 470-495, 510-515; models/vgg16.py:9-21).

One engine per (operation, geometry), chosen by `select()` / `select_wrw()` from measurements on MI355X at the step's shapes
(tools/bench_hipconv.py -> profiles/r02_hipconv_*.txt).  The engines are the records of `_ENGINES` below — the call that runs each
pass, the support query that says which layers the engine accepts (`takes`), and what the engine needs.  A new engine is one record
there (its passes, its `takes`, its flags) plus its rule in `_select` / `_select_wrw`; a new direct opt-in, for fp32 or for bf16
activations, is one row of `_DIRECT_OPT_INS` (and, where it reaches a new entry point, one entry of `_DIRECT_ENTRIES`).  A rule asks the
record before it answers, and a last guard in `_select_any` / `_select_wrw_any` turns any answer its engine does not take into "miopen":
no rule, and no forced mode, can hand an engine a layer it raises on.

  "winograd"  csrc/winograd.hip   k3 s1 p1 forward / backward-data of Conv2d and ConvTranspose2d, F(4x4,3x3) on fp32 MFMA:
                                  2.0-2.4x MIOpen's F(2x2,3x3) assembly from 16x16 maps and 128 channels up
  "wino_dil"  csrc/winograd.hip   netG's dilated down convolution Conv2d(k4 s2 p3 d2) and netD's Conv2d(k4 s1 p1) by F(3x3,4x4) —
                                  forward, input and weight gradient, 1.4-2.0x MIOpen at 128..512 channels on 32x32..128x128 inputs
  "wino_s2"   csrc/winograd.hip   the 4x4 stride-2 pad-1 layers (Conv2d of netP/netD/netF, ConvTranspose2d of netP/netG) by F(5x5,2x2) on
                                  the polyphase components — forward, input and weight gradient, 5-30 % faster than MIOpen at
                                  >= 128 / 64 channels on coarse grids of 16..64
  "thin"      csrc/thin_conv.hip  3x3 stride-1 layers with a 3- or 6-channel side at full resolution (VGG conv1_1, netG's last ConvTranspose2d):
                                  one pass over the wide tensor on the vector ALUs, 1.3-3x MIOpen
  "thin_f2m"  csrc/thin_conv.hip  Conv2d 3 -> K, k4 s2 p1, forward under bf16 activations: the window gather on the bf16 matrix cores, one launch
  "thin_mfma" csrc/thin_conv.hip  weight gradient of the layers with 3 or 6 channels on the narrow side (k3 s1 p1, k4 s2 p1) under bf16
                                  activations: the pixel reduction on the bf16 matrix cores straight from NCHW, two launches
  "smallmap"  csrc/smallmap.hip   the innermost levels: the weight tensor streamed once, 16 bytes per lane straight into MFMA operands —
                                  weight gradients of the 4x4 stride-2 layers up to 256 positions per batch (dW written in its native
                                  layout), forward and input gradient of the 3x3 / 4x4 layers up to 32 positions.  For a caller that sets a
                                  reach (`select(..., reach=)`, the trainer's `opt.smallmap_reach`): forward and input gradient of the
                                  512 / 1024-channel 4x4 stride-2 layers (pad 1 and the dilated pad 3) on 4x4 .. 16x16 maps (128 .. 1024
                                  positions per batch) that MIOpen had and loses (`_reach_regime`): the 4x4 maps (128 positions) on the
                                  streaming kernels, the 8x8 / 16x16 maps as LDS-tiled split-K GEMMs on the weights in place (the engine's
                                  tiled regime).  The 3x3 layers and every weight gradient of those levels stay on MIOpen.
  "direct"    csrc/conv_gemm.hip  one-launch implicit GEMM, NCHW in/out (every k3/k4, stride 1/2, dilated and transposed
                                  geometry of the nets, forward and backward-data): at parity with MIOpen (~100 TF), used
                                  where it measured >= 7 % faster
  "one"       csrc/thin_conv.hip  Conv2d with ONE output channel, stride 1 (netD's last layer, 512 -> 1 on 31x31): forward and weight
                                  gradient as one pass over the input
  "bf16d"     csrc/conv_bf16.hip  bf16 activations (BASELINE config 5): the direct bf16 implicit GEMM, forward / input gradient / weight
                                  gradient of the k3 s1 p1 and k4 s2 p1 layers where the split-bf16 Winograd engines do not win
                                  — and, by a switch of its own (`set_direct_dilated_bf16`, the "bf16_dil_data" row of `_DIRECT_OPT_INS`),
                                  forward / input gradient of netG's dilated down convolution Conv2d(k4 s2 p3 d2) as a 16-tap correlation
                                  on the odd / odd quarter of the input (ops.conv4x4s2_bf16_dil), instead of "wino_dil" / MIOpen — and, by
                                  another switch of its own (`set_direct_dilated_bf16_dw`, the "bf16_dil_wrw" row), that layer's weight
                                  gradient as the pixel reduction over the same quarter (ops.conv4x4s2_bf16_dil_wrw), instead of
                                  "wino_dil" / MIOpen.  The engine takes a pass of that layer only while the pass's switch is on
                                  (`_DIRECT_TAKES_SWITCH`)
  "bf16x3d"   csrc/conv_bf16.hip  fp32 activations, opt-in (`set_conv_math(fp32=...)`, the four direct names of ops.DIRECT_PASSES): forward / input gradient on split-bf16 operands
                                  — and, by a switch of its own (`set_direct_dilated`), forward / input gradient of netG's dilated down convolution
                                  Conv2d(k4 s2 p3 d2) as a 16-tap correlation on the odd / odd quarter of the input, instead of "wino_dil"
  "bf16x3w"   csrc/conv_bf16.hip  fp32 activations, opt-in (the same names): the weight gradient as a pixel reduction on split-bf16 operands, two launches
                                  — and, by a switch of its own (`set_direct_dilated_dw`), the weight gradient of the dilated down convolution as
                                  the same reduction over the odd / odd quarter of the input, instead of "wino_dil"
  "miopen"    torch               everything else
Weight gradients: Winograd F(3x3,4x4) (csrc/winograd.hip) for the 3x3 stride-1 layers with >= 256 channels on 16x16..64x64
maps (2.0-2.4x MIOpen), MIOpen otherwise (`select_wrw`).

`IPSR_CONV_ENGINE=miopen|direct|winograd|auto` (default auto) forces one engine wherever it is implemented — for the
per-engine parity tests and for A/B timing.  Non-contiguous inputs and other dtypes take MIOpen.
"""
import os
from collections import namedtuple
from functools import partial

import torch
import torch.nn as nn
import torch.nn.functional as F

from .. import _lib, ops
from .. import dist as ipsr_dist

_FORCE = None          # test hook: overrides the environment
# Arithmetic of the Winograd GEMMs (ops.MATH_CODE): "fp32" for fp32 activations (the reference's arithmetic; "bf16x6" / "bf16x3" are
# opt-in, models/IPSR.py `opt.conv_math`), "bf16x3" for bf16 activations / under bf16 autocast (BASELINE config 5).  The four direct names
# for fp32 activations are no Winograd arithmetic: see ops.DIRECT_PASSES for the passes each moves to "bf16x3d" / "bf16x3w".
_MATH = {"fp32": "fp32", "bf16": "bf16x3"}


def set_conv_math(fp32=None, bf16=None):
    """Choose the arithmetic of the Winograd engines for fp32 activations and for bf16 activations (autocast).  fp32 may also be one of the
    four direct names of ops.DIRECT_PASSES (the table says which passes each moves to the direct split-bf16 kernels); they are for fp32
    activations only."""
    from .. import ops as _ops
    for key, val in (("fp32", fp32), ("bf16", bf16)):
        if val is not None:
            if val not in _ops.MATH_CODE or (key == "bf16" and val in _ops.DIRECT_PASSES):
                raise ValueError("conv math must be one of %s" % sorted(k for k in _ops.MATH_CODE if k))
            _MATH[key] = val
    _SEL.clear()           # `select` memoises without the arithmetic


# The four opt-in switches of netG's dilated down convolution, by the key of the row of `_DIRECT_OPT_INS` each one switches on: fp32 activations
# on the direct split-bf16 kernels (data passes, weight gradient), bf16 activations on the direct bf16 kernels (the same two).
_DIRECT_SWITCHES = {"dil_data": False, "dil_wrw": False, "bf16_dil_data": False, "bf16_dil_wrw": False}


def _set_direct_switch(key, on):
    _DIRECT_SWITCHES[key] = bool(on)
    _SEL.clear()           # `select` memoises without the switches


def _direct_passes_on():
    """-> the keys of `_DIRECT_OPT_INS` that are switched on: the passes the fp32 arithmetic name moves (ops.DIRECT_PASSES) and the
    `_DIRECT_SWITCHES` that are set.  The one place the switches are read."""
    return ops.DIRECT_PASSES.get(_MATH["fp32"], frozenset()) | {key for key, on in _DIRECT_SWITCHES.items() if on}


def set_direct_dilated(on):
    """Opt-in, default off, independent of `set_conv_math`: under fp32 activations, forward and input gradient of the dilated down
    convolution Conv2d(k4, stride 2, pad 3, dilation 2) that "wino_dil" has go to the direct split-bf16 kernel ("bf16x3d",
    ops.conv4x4s2_bf16x3 with ops.S2_DILATED) on every shape it takes.  Weight gradients, bf16 activations, forced engines and the
    k4 s1 p1 layer stay where they are."""
    _set_direct_switch("dil_data", on)


def direct_dilated():
    """Whether `set_direct_dilated` is on."""
    return "dil_data" in _direct_passes_on()


def set_direct_dilated_dw(on):
    """Opt-in, default off, independent of `set_conv_math` and of `set_direct_dilated`: under fp32 activations, the weight gradient of the
    dilated down convolution Conv2d(k4, stride 2, pad 3, dilation 2) that "wino_dil" has goes to the direct split-bf16 kernel ("bf16x3w",
    ops.conv4x4s2_bf16x3_dil_wrw) on every shape it takes (the "dil_wrw" row of `_DIRECT_OPT_INS`).  The data passes, bf16 activations,
    forced engines, the k4 s1 p1 layer and "smallmap" grids stay where they are."""
    _set_direct_switch("dil_wrw", on)


def direct_dilated_dw():
    """Whether `set_direct_dilated_dw` is on."""
    return "dil_wrw" in _direct_passes_on()


def set_direct_dilated_bf16(on):
    """Opt-in, default off, independent of `set_conv_math`, `set_direct_dilated` and `set_direct_dilated_dw`: under bf16 activations, forward
    and input gradient of the dilated down convolution Conv2d(k4, stride 2, pad 3, dilation 2) that "wino_dil" or MIOpen has go to the direct
    bf16 kernel ("bf16d", ops.conv4x4s2_bf16_dil) on every shape it takes (the "bf16_dil_data" row of `_DIRECT_OPT_INS`).  Weight gradients,
    fp32 activations, forced engines, "smallmap" grids and the k4 s1 p1 layer stay where they are."""
    _set_direct_switch("bf16_dil_data", on)


def direct_dilated_bf16():
    """Whether `set_direct_dilated_bf16` is on."""
    return "bf16_dil_data" in _direct_passes_on()


def set_direct_dilated_bf16_dw(on):
    """Opt-in, default off, independent of `set_conv_math` and of the three other dilated switches: under bf16 activations, the weight gradient
    of the dilated down convolution Conv2d(k4, stride 2, pad 3, dilation 2) that "wino_dil" or MIOpen has goes to the direct bf16 kernel
    ("bf16d", ops.conv4x4s2_bf16_dil_wrw) on every shape it takes (the "bf16_dil_wrw" row of `_DIRECT_OPT_INS`).  The data passes, fp32
    activations, forced engines, "smallmap" grids and the k4 s1 p1 layer stay where they are."""
    _set_direct_switch("bf16_dil_wrw", on)


def direct_dilated_bf16_dw():
    """Whether `set_direct_dilated_bf16_dw` is on."""
    return "bf16_dil_wrw" in _direct_passes_on()


def _amp_bf16():
    return torch.is_autocast_enabled() and torch.get_autocast_dtype("cuda") == torch.bfloat16
_check_hook = None     # test hook: callable(kind, engine, geometry, operands, result) after every engine call of _HipConv


# The A/B switches (IPSR_CONV_ENGINE, IPSR_NO_SMALLMAP, IPSR_NO_THIN, IPSR_BF16_ENGINES) are read from the environment ONCE, at first use:
# a training step asks `select` ~250 times, and each os.environ.get costs ~0.8 us of a host that is the step's bound under bf16
# (tools/profile_host.py: 2000 look-ups, 1.6 ms per step).  `reload_env()` re-reads them (a tool that flips one in-process).
_ENV = {}
_SEL = {}


def _env(name, default):
    v = _ENV.get(name)
    if v is None:
        v = _ENV[name] = os.environ.get(name, default)
    return v


def reload_env():
    _ENV.clear()
    _SEL.clear()


def _mode():
    return _FORCE or _env("IPSR_CONV_ENGINE", "auto")


def select(op, B, Cin, H, W, Cout, k, stride, pad, dil, bf16=False, reach=None):
    """-> the engine for one convolution call.  (Cin, H, W) = the module's input, as in ipsr_conv2d.  Memoised per (mode, shape):
    the rules query the library (workspace probes), ~150 convolution calls per training step ask.
    bf16: the activations are bf16 tensors — only the Winograd engines read / write those; every other shape takes MIOpen.
    reach: the caller's reach of the small-map engine's tiled regime in positions per batch (`_reached`); None or 0 = none."""
    key = (0, _FORCE, op, B, Cin, H, W, Cout, k, stride, pad, dil, bf16)
    eng = _SEL.get(key)
    if eng is None:
        eng = _SEL[key] = _select_any(op, (op in (ops.CONVT_FWD, ops.CONVT_BWD_DATA), B, Cin, H, W, Cout, k, stride, pad, dil), bf16)
    return _reached("data", key, eng, op, bf16, reach) if reach else eng


# The reach.  "smallmap" beyond the chain's own rules — its tiled regime (ops.conv_smallmap(..., tiled=True)) and the streaming kernels on the
# 4x4 levels — is no rule of the chain: a caller asks for it, per module, by the
# number of positions per batch up to which it wants MIOpen's passes of the 3x3 / 4x4 layers with >= 256 channels moved to "smallmap" — the
# trainer stamps `opt.smallmap_reach` on the conv modules of its nets as the attribute `smallmap_reach`, `conv_nobias` reads it.  It is applied
# to the FINAL answer of the chain and moves "miopen" only: never a pass another engine has, no bf16 activations (the wider reach lost there,
# `_bf16_direct`), no forced engine, not under IPSR_NO_SMALLMAP=1.  Inside the reach `_reach_regime` says which passes move, and to which of
# the engine's two regimes.


def _reach_regime(kind, op, lay):
    """-> "stream" | "tiled" | None: the regime of "smallmap" that beats MIOpen on this pass, by the rule of profiles/smallmap_tiled_layers.txt
    (the engine's median below MIOpen's minimum by more than MIOpen's spread), measured at the step's shapes — 512 / 1024 channels, batch 8
    and netF's batch 16 — and applied to the position counts between them:
      forward / input gradient   the k4 layers (stride 2, pad 1 and the dilated pad 3):
                                 33 .. 128 positions: the streaming kernels (every row, 1.1-2.7x MIOpen; the tiled GEMM has one position
                                 tile there and nothing to share);  129 .. 256: SM_FWD tiled, SM_DATA streaming;  257 .. 512: tiled
                                 (1.05-1.4x), except SM_FWD with 1024 weight rows (netP's ConvTranspose2d 1024 -> 512 @8 input gradient:
                                 91 us against MIOpen's 96.7-102.6, level by the rule);  513 .. 1024: SM_FWD tiled (1.3x).  SM_DATA at
                                 1024 positions was measured on one pass only, netF's batch-16 input gradient @16 (102 us against
                                 MIOpen's 170), which the chain gives to "wino_s2": nothing of MIOpen's was measured there, none moves
                                 k3 stays.  At 512 positions its rows are level or lose.  At 128 positions the streaming kernels win all
                                 four rows by 6-12 us a call, the smallest gains of the table (~40 us a step) — but MIOpen's 3x3 kernels on
                                 those maps are what makes a batch-2 step differ between identical runs, and tests/test_gpu_loss_head.py
                                 takes its tolerance from that difference: without them the step repeats bit for bit and the tolerance
                                 falls below what the loss heads' own rounding moves netG's gradient by (5.5e-5 of its norm).  They move
                                 with a change that can re-derive that tolerance.
      weight gradient            none moves.  The engine has no tiled weight gradient; the streaming kernel loses from 512 positions up (k4 s2
                                 beyond the chain's own 256 included) and is ahead only on the 3x3 layers at 32 positions (3x) and at 128 with
                                 <= 512 channels (1.4x).  Those two stay as well: MIOpen's 3x3 weight gradient there is a transform
                                 algorithm whose own error is several times the bound of an fp32 fma chain (and nonzero where the exact
                                 value is zero), so the in-step comparison with MIOpen that guards every pass moved here
                                 (tests/test_gpu_smallmap_reach_step.py) cannot hold for them, though the kernel is within 0.4 of that
                                 bound against float64."""
    transposed, B, Cin, H, W, Cout, k, stride, pad, dil = lay
    g = _smallmap_geometry(lay)
    pos = g[0] * g[3] * g[4] if g[3] >= 1 and g[4] >= 1 else 0
    if pos < 1:
        return None
    if kind == "wrw":
        return None
    if pos <= 32:
        return None              # the chain's own rule (`_smallmap_data_wins`)
    if k != 4:
        return None
    if pos <= 128:
        return "stream"
    fwd = _smallmap_op(op) == ops.SM_FWD
    if pos <= 256:
        return "tiled" if fwd else "stream"
    if pos <= 512:
        return None if fwd and g[1] > 512 else "tiled"
    return "tiled" if fwd else None


def _reached(kind, key, eng, op, bf16, reach):
    """-> "smallmap" where the pass of `key` (the memo key of `select` / `select_wrw`), answered `eng` by the chain, is inside `reach`."""
    if eng != "miopen" or bf16:
        return eng
    rkey = key + (int(reach),)
    hit = _SEL.get(rkey)
    if hit is None:
        lay = ((op in (ops.CONVT_FWD, ops.CONVT_BWD_DATA),) if kind == "data" else ()) + key[3 if kind == "data" else 2:-1]
        transposed, B, Cin, H, W, Cout, k, stride, pad, dil = lay
        g = _smallmap_geometry(lay)
        regime = _reach_regime(kind, op, lay)
        ok = _mode() == "auto" and _env("IPSR_NO_SMALLMAP", "0") != "1" and regime is not None and k in (3, 4) and min(Cin, Cout) >= 256 \
            and g[0] * g[3] * g[4] <= int(reach) and bool(_ENGINES["smallmap"].takes(kind, op, lay, False, tiled=regime == "tiled"))
        hit = _SEL[rkey] = "smallmap" if ok else eng
    return hit


def _via_reach(kind, op, lay, bf16, reach):
    """Whether this pass runs on "smallmap" only because of the caller's reach, and in the tiled regime: those calls carry `tiled=True`."""
    if not reach or _reach_regime(kind, op, lay) != "tiled":
        return False
    if kind == "data":
        return select(op, *lay[1:], bf16) != "smallmap" and select(op, *lay[1:], bf16, reach=reach) == "smallmap"
    return select_wrw(*lay, bf16) != "smallmap" and select_wrw(*lay, bf16, reach=reach) == "smallmap"


# Below `select` / `select_wrw` a layer travels as ONE tuple, `lay` = (transposed, B, Cin, H, W, Cout, k, stride, pad, dil): (Cin, H, W) =
# the module's input whatever the operation.  The rule functions read the switches through `_mode()` / `_env()`; `_SEL` is the only memo.
def _select_any(op, lay, bf16):
    eng = _select(op, lay)
    transposed, B, Cin, H, W, Cout, k, stride, pad, dil = lay
    if bf16 and not (_bf16_wins(eng, Cin, H, W, Cout) or _ENGINES[eng].fp32_copies):
        if _mode() == "auto" and _thin_wins(op, lay, True):
            eng = "thin"         # the vector-ALU stream kernels read / write bf16 tensors themselves (ipsr_conv3x3_thin_io)
        elif _mode() == "auto" and _env("IPSR_NO_THIN", "0") != "1" and op == ops.CONV_FWD and Cin == 3 and (k, stride, pad, dil) == (4, 2, 1, 1) and H * W >= 4096 \
                and engine_takes("thin_f2m", "data", op, lay, True):
            # the first Conv2d of netP / netD (3 -> 64, k4 s2): the window gather on the matrix cores, 0.041-0.045 vs MIOpen's 0.059 ms and one
            # launch instead of four (profiles/r04_thin_bf16.txt; for the 3x3 thin layers the vector-ALU kernels and MIOpen stay ahead or level)
            eng = "thin_f2m"
        else:
            eng = _bf16_direct(op, lay)
    eng = _direct_opt_in("data", eng, op, lay, bf16)         # after the bf16 chain: the opt-ins replace its answer
    # the final guard: the rules and forced modes that probe nothing ("winograd", "wino_dil", IPSR_CONV_ENGINE=winograd) answer "miopen"
    # where their engine refuses the layer, instead of raising in `conv_nobias` on a layer torch computes
    return eng if engine_takes(eng, "data", op, lay, bf16) else "miopen"


def _bf16_direct(op, lay):
    """bf16 activations, and the split-bf16 Winograd engines do not win this shape: the DIRECT bf16 implicit GEMM (csrc/conv_bf16.hip,
    ops.conv3x3_bf16: one launch, NCHW in and out) where it is implemented — k3 s1 p1 on maps of 16..128 pixels width — else MIOpen.
    Measured at batch 16 (profiles/r04_conv_bf16_layers.txt): 700-870 TF against MIOpen's 350-570 incl. its layout transposes on
    every map from 32x32 up; on 16x16 maps MIOpen ties (and the Winograd engines win from 512 channels)."""
    transposed, B, Cin, H, W, Cout, k, stride, pad, dil = lay
    if _env("IPSR_BF16_ENGINES", "") == "none" or _mode() in ("miopen", "winograd", "direct"):
        return "miopen"
    if k == 3 and stride == 1 and pad == 1 and dil == 1 and H * W >= 256 and engine_takes("bf16d", "data", op, lay, True):
        return "bf16d"           # 16x16 maps too since the reduction is cut over workgroups there (0.041-0.063 vs 0.056-0.081 split-Winograd, 0.070-0.122 MIOpen)
    # (measured and not kept: the small-map engine on fp32 copies for the innermost levels beyond 32 positions per batch — 708 images/s at
    # 32, 706 at 64, 696 at 256, 658 at 1024: MIOpen's tiny bf16 convolutions cost 45-60 us per CALL but far less device time)
    g = _s2_geometry(lay)
    if g is not None and engine_takes("bf16d", "data", op, lay, True):
        # the 4x4 stride-2 family (profiles/r04_conv_bf16_layers.txt, batch 16): 1.3-2x MIOpen wherever the launch has enough tiles;
        # a 16x16 coarse grid gives one pixel tile per image (64 workgroups at 512 channels) and MIOpen ties or wins
        Kc, Cf, nh, nw = g
        if _s2_mode(op) == ops.S2_FINE_TO_COARSE:
            if nw == 16:                 # one pixel tile per image: the split reduction fills the chip up to 512 produced channels (0.048-0.078 vs MIOpen's
                return "bf16d" if Kc <= 512 else "miopen"      # 0.083-0.106); 1024 produced channels leave no room to split: 0.098 vs 0.087
            return "bf16d" if nw >= 32 and ((Kc + 127) // 128) * B * nh * nw // 256 >= 128 else "miopen"
        return "bf16d"
    return "miopen"


def _bf16_wins(eng, Cin, H, W, Cout, wrw=False):
    """bf16 activations (BASELINE config 5).  MIOpen's bf16 implicit GEMMs run ~490 TF and need no transform passes; the Winograd
    engines here must SPLIT their operands (F(4x4,3x3) amplifies rounding ~100x), so their intermediates stay fp32-wide: 4.5x the
    bf16 activation bytes each way.  They win where the channel count amortises that (profiles/r03_bf16_layers.txt, batch 16, forward
    + both gradients against MIOpen incl. its layout transposes and weight casts): the 3x3 layers with >= 512 channels on one side at
    <= 32x32 (0.72-0.79x), the dilated 4x4 layers with >= 256 channels at <= 64x64 (0.70-0.90x), netD's 4x4 stride-1 layer (0.95x);
    they lose on larger maps and on the whole 4x4 stride-2 family (1.1-1.7x) — those stay on MIOpen.  IPSR_BF16_ENGINES=all|none
    overrides (A/B timing)."""
    force = _env("IPSR_BF16_ENGINES", "")
    if not _ENGINES[eng].bf16_io or force == "none":
        return False
    if force == "all":
        return True
    if eng == "winograd":
        # round 4: against the DIRECT bf16 kernel (csrc/conv_bf16.hip, profiles/r04_conv_bf16_layers.txt) the split engines keep the WEIGHT
        # GRADIENTS of the 16x16 maps (0.060-0.084 vs 0.076-0.159 ms); forward / input gradient went to the direct kernel when its reduction
        # was cut over workgroups; at 32x32 the direct weight gradient ties or wins since its runs were halved (0.068-0.131 vs 0.084-0.126)
        return wrw and H * W <= 256 and max(Cin, Cout) >= 512
    if eng == "wino_dil":
        return H * W <= 4096 and min(Cin, Cout) >= 256
    return False


def _select(op, lay):
    transposed, B, Cin, H, W, Cout, k, stride, pad, dil = lay
    mode = _mode()
    fwd = op in (ops.CONV_FWD, ops.CONVT_FWD)
    cred, kout = (Cin, Cout) if fwd else (Cout, Cin)            # reduction / produced channels of this operation
    wino_ok = k == 3 and stride == 1 and pad == 1 and dil == 1 and cred % 16 == 0
    if mode == "miopen":
        return "miopen"
    if mode == "winograd":
        return "winograd" if wino_ok else "miopen"
    if mode == "direct":
        return "direct" if engine_takes("direct", "data", op, lay, False) else "miopen"
    if mode == "auto" and _is_dilated4(k, stride, pad, dil) and op in (ops.CONV_FWD, ops.CONV_BWD_DATA) \
            and cred % 16 == 0 and min(Cin, Cout) >= 64 and 32 <= H <= 256 and H % 2 == 0 and W % 2 == 0:
        # netG's dilated down convolution: F(3x3,4x4), 1.4-2.0x MIOpen (profiles/r02_hipconv_k3_v3.txt); since the GEMM has a
        # 64-row tile also the outermost 64 -> 64 @256x256 level (0.171 / 0.193 vs 0.230 / 0.261 ms, profiles/r03_hipconv_k3.txt)
        return "wino_dil"
    if mode == "auto" and _is_k4s1(k, stride, pad, dil) and op in (ops.CONV_FWD, ops.CONV_BWD_DATA) \
            and cred % 16 == 0 and min(Cin, Cout) >= 128 and 16 <= H <= 128 and W >= 4:
        return "wino_dil"        # netD's 4x4 stride-1 convolution: the same F(3x3,4x4) pipeline on the image itself (which refuses extents below the kernel)
    if mode == "auto" and op == ops.CONV_FWD and Cout == 1 and Cin >= 64 and engine_takes("one", "data", op, lay, False):
        return "one"             # netD's last layer (512 -> 1): a single pass over the input, 15 vs 80-143 us
    if mode == "auto" and _thin_wins(op, lay):
        return "thin"            # 3/6-channel side at full resolution: one pass over the wide tensor on the vector ALUs
    if mode == "auto" and _smallmap_data_wins(op, lay):
        return "smallmap"        # innermost levels (<= 32 positions per batch): the weight tensor streamed once into MFMA operands
    if mode == "auto":
        g = _s2_geometry(lay)
        if g is not None and _s2_wins(g, _s2_mode(op), B) and engine_takes("wino_s2", "data", op, lay, False):
            return "wino_s2"     # 4x4 stride-2 layers: polyphase Winograd F(5x5,2x2)
    # auto: measured rules (MI355X, batch 8; profiles/r03_hipconv_k3.txt).  64 produced channels run on the GEMM's 64-row tile:
    # 64 -> 64 @256x256 (VGG conv1_2, forward and input gradient) 0.311 vs MIOpen's 0.378 ms
    if wino_ok and H * W >= 256 and min(cred, kout) >= 64 and (max(cred, kout) >= 128 or kout == 64):
        return "winograd"
    if k == 4 and stride == 2 and dil == 2 and op == ops.CONV_BWD_DATA and Cin >= 128 and 16 <= H <= 128 \
            and engine_takes("direct", "data", op, lay, False):
        return "direct"          # dilated 4x4 stride-2 input gradient: 8-12 % faster than MIOpen's f3x2_dilation2 + transposes
    return "miopen"


def _is_dilated4(k, stride, pad, dil):
    return k == 4 and stride == 2 and pad == 3 and dil == 2


def _s2_geometry(lay):
    """(Kc, Cf, nh, nw) of a k4 s2 p1 layer in the coarse / fine terms of ipsr_conv4x4s2_winograd, or None."""
    transposed, B, Cin, H, W, Cout, k, stride, pad, dil = lay
    if not (k == 4 and stride == 2 and pad == 1 and dil == 1):
        return None
    if transposed:
        return Cin, Cout, H, W
    if H % 2 or W % 2:
        return None
    return Cout, Cin, H // 2, W // 2


def _s2_wins(geom, mode=None, B=8):
    """Measured (profiles/r03_hipconv_k4s2.txt, batch 8): F(5x5,2x2) beats MIOpen by 5-35 % from 128 coarse / 64 fine channels up
    on coarse grids of 16..64; it loses on 8x8 and below (too few tiles).  The 64-channel 128x128 layer is transform bound: only
    its coarse-to-fine pass (ConvTranspose2d forward), whose output transform writes whole rows, is ahead (0.210 vs 0.226 ms)."""
    Kc, Cf, nh, nw = geom
    if mode == ops.S2_COARSE_TO_FINE and Kc >= 64 and Cf >= 64 and 16 <= min(nh, nw) and max(nh, nw) <= 128:
        return True
    if mode == ops.S2_COARSE_TO_FINE and B >= 16 and Kc >= 512 and Cf >= 512 and min(nh, nw) == 8 and max(nh, nw) == 8:
        return True          # netF's 512 -> 512 @16 -> 8 input gradient at batch 16 (the batched discriminator pass): 0.141 vs 0.188 ms
    return Kc >= 128 and Cf >= 64 and 16 <= min(nh, nw) and max(nh, nw) <= 64


def _s2_mode(op):
    return ops.S2_FINE_TO_COARSE if op in (ops.CONV_FWD, ops.CONVT_BWD_DATA) else ops.S2_COARSE_TO_FINE


def _smallmap_geometry(lay):
    """(B, R, Cq, Ho, Wo, Hf, Wf, k, stride, pad, dil) of ipsr_conv_smallmap for this module call: R / (Ho, Wo) = the weight's first
    channel dimension and its grid, Cq / (Hf, Wf) = the second."""
    transposed, B, Cin, H, W, Cout, k, stride, pad, dil = lay
    if transposed:
        Hy, Wy = (H - 1) * stride - 2 * pad + dil * (k - 1) + 1, (W - 1) * stride - 2 * pad + dil * (k - 1) + 1
        return B, Cin, Cout, H, W, Hy, Wy, k, stride, pad, dil
    Hy, Wy = (H + 2 * pad - dil * (k - 1) - 1) // stride + 1, (W + 2 * pad - dil * (k - 1) - 1) // stride + 1
    return B, Cout, Cin, Hy, Wy, H, W, k, stride, pad, dil


def _thin_wins(op, lay, bf16=False):
    """3x3 stride-1 layers with a 3- or 6-channel side on maps of >= 64x64 (profiles/r02_thin.txt, device time at 256x256, batch 8):
    many -> few (VGG conv1_1 input gradient 185 -> 61 us, netG's last ConvTranspose2d forward 217 -> 130 us) and 3 -> many
    (VGG conv1_1 forward 70 -> 52 us, and the bias + ReLU pass goes into the kernel); 6 -> 64 forward and the weight gradients
    stay on MIOpen (87 vs 99 us; 134 vs 296 us).  bf16 activations (batch 16, profiles/r04_thin_bf16.txt): 3 -> many wins by 2x and
    1.5x (VGG conv1_1 forward 90 vs 182 us, bias + ReLU included; the last ConvTranspose2d's input gradient 172 vs 261 us); 6 -> 64 stays
    on MIOpen (175 vs 156 us) and many -> 3 on the direct MFMA kernel (252 vs 300 us)."""
    if _env("IPSR_NO_THIN", "0") == "1":           # A/B switch
        return False
    transposed, B, Cin, H, W, Cout, k, stride, pad, dil = lay
    if not (k == 3 and stride == 1 and pad == 1 and dil == 1) or H * W < 4096 or not engine_takes("thin", "data", op, lay, bf16):
        return False
    fwd = op in (ops.CONV_FWD, ops.CONVT_FWD)
    i, o = (Cin, Cout) if fwd else (Cout, Cin)
    if bf16:
        return i == 3
    return o in (3, 6) or i == 3


def _smallmap_op(op):
    """Conv2d forward / ConvTranspose2d backward-data contract the weight's second dimension (SM_FWD); the other two its first."""
    return ops.SM_FWD if op in (ops.CONV_FWD, ops.CONVT_BWD_DATA) else ops.SM_DATA


def _smallmap_data_wins(op, lay):
    """Forward / input gradient on grids of <= 32 positions per batch (2x2 and 1x1 at batch 8): 15-20 us on the device against
    MIOpen's 40-50 (profiles/r02_hipconv_small.txt); from 128 positions up the op is a real GEMM and MIOpen ties."""
    transposed, B, Cin, H, W, Cout, k, stride, pad, dil = lay
    if _env("IPSR_NO_SMALLMAP", "0") == "1" or k not in (3, 4) or min(Cin, Cout) < 256:
        return False
    g = _smallmap_geometry(lay)
    return g[3] >= 1 and g[4] >= 1 and g[0] * g[3] * g[4] <= int(_env("IPSR_SMALLMAP_MAX_POS", "32")) and engine_takes("smallmap", "data", op, lay, False)


def _smallmap_wrw_wins(lay):
    """Weight gradients of the 4x4 layers on grids of <= 256 positions per batch (the four innermost levels at batch 8): the GEMM
    writes dW in place, 27-39 us against MIOpen's 41-57 (profiles/r02_hipconv_small.txt)."""
    transposed, B, Cin, H, W, Cout, k, stride, pad, dil = lay
    if k != 4 or stride != 2 or _env("IPSR_NO_SMALLMAP", "0") == "1":        # the switch is for A/B timing
        return False
    g = _smallmap_geometry(lay)
    return g[3] >= 1 and g[4] >= 1 and g[0] * g[3] * g[4] <= 256 and min(Cin, Cout) >= 256 and engine_takes("smallmap", "wrw", None, lay, False)


def _is_k4s1(k, stride, pad, dil):
    return k == 4 and stride == 1 and pad == 1 and dil == 1


def select_wrw(transposed, B, Cin, H, W, Cout, k, stride, pad, dil, bf16=False, reach=None):
    """-> the engine for the weight gradient of one layer (profiles/r02_hipconv_k3_wrw.txt: F(3x3,4x4) is 2.0-2.4x
    MIOpen from 256 channels up on maps of 16x16..64x64; on larger maps its tile-major transforms lose to MIOpen).
    reach: as in `select`."""
    key = (1, _FORCE, transposed, B, Cin, H, W, Cout, k, stride, pad, dil, bf16)
    eng = _SEL.get(key)
    if eng is None:
        eng = _SEL[key] = _select_wrw_any((transposed, B, Cin, H, W, Cout, k, stride, pad, dil), bf16)
    return _reached("wrw", key, eng, None, bf16, reach) if reach else eng


def _select_wrw_any(lay, bf16):
    transposed, B, Cin, H, W, Cout, k, stride, pad, dil = lay
    eng = _select_wrw(lay)
    thin = _mode() == "auto" and _env("IPSR_NO_THIN", "0") != "1" and pad == 1 and dil == 1 and (k, stride) in ((3, 1), (4, 2)) and H * W >= 4096 \
        and engine_takes("thin_mfma", "wrw", None, lay, bf16)
    if not bf16:
        # fp32 activations: the same pixel reduction on v_mfma_f32_32x32x2_f32 (profiles/r04_thin_fp32.txt, batch 8).  It wins over the opt-ins:
        # no row of `_DIRECT_OPT_INS` replaces "thin_mfma"
        if thin and eng == "miopen":
            eng = "thin_mfma"
    elif not (_bf16_wins(eng, Cin, H, W, Cout, True) or _ENGINES[eng].fp32_copies):
        # 3 / 6 channels on the narrow side: the pixel reduction on the bf16 matrix cores straight from NCHW (profiles/r04_thin_bf16.txt, batch 16:
        # 3 -> 64 k4 s2 0.033 vs MIOpen's 0.057 ms, ConvT 128 -> 3 k3 0.152 vs 0.202, k4 s2 0.052 vs 0.063, 6 -> 64 0.118 vs 0.125 — and 2
        # launches instead of MIOpen's 5-6)
        eng = "thin_mfma" if thin else _bf16_direct_wrw(lay)
    eng = _direct_opt_in("wrw", eng, None, lay, bf16)        # after the bf16 chain, as in `_select_any`
    # the final guard, as in `_select_any`: "winograd", "wino_dil" and "wino_s2" weight gradients are answered without a probe
    return eng if engine_takes(eng, "wrw", None, lay, bf16) else "miopen"


def _bf16_direct_wrw(lay):
    """Weight gradient on bf16 activations by the direct kernel (ops.conv3x3_bf16_wrw): 1.1-2.0x MIOpen on every map from 32x32 up (one
    run per CU: the partial-sum slabs are what it costs)."""
    transposed, B, Cin, H, W, Cout, k, stride, pad, dil = lay
    if _env("IPSR_BF16_ENGINES", "") == "none" or _mode() in ("miopen", "winograd", "direct"):
        return "miopen"
    if k == 3 and stride == 1 and pad == 1 and dil == 1 and H * W >= 1024 and engine_takes("bf16d", "wrw", None, lay, True):
        return "bf16d"
    g = _s2_geometry(lay)
    if g is not None and g[3] >= 32 and ((g[0] + 127) // 128) * ((g[1] + 31) // 32) >= 4 and engine_takes("bf16d", "wrw", None, lay, True):
        return "bf16d"           # 1.2-1.4x MIOpen from four 128 x 32 output tiles up on coarse grids >= 32 wide; 16-wide grids and single tiles lose
    return "miopen"


def _dil_geometry(lay):
    """(Kc, Cf, nh, nw) of a Conv2d(k4 s2 p3 d2) layer on an even map in the coarse / fine terms of ipsr_conv4x4s2_bf16x3, or None."""
    transposed, B, Cin, H, W, Cout, k, stride, pad, dil = lay
    if transposed or not _is_dilated4(k, stride, pad, dil) or H % 2 or W % 2:
        return None
    return Cout, Cin, H // 2, W // 2


def _dil_mode(op):
    return ops.S2_DILATED | (ops.S2_FINE_TO_COARSE if op == ops.CONV_FWD else ops.S2_COARSE_TO_FINE)


# MIOpen's one dilated weight gradient of the step, netG's outermost 64 -> 64 @256x256 (coarse grid 128 wide), as (Kc, Cf, nh, nw)
_DIL_WRW_MIOPEN_ROW = (64, 64, 128, 128)


# ---- the direct opt-ins: one row per pass a switch moves to "bf16x3d" / "bf16x3w" (fp32 activations) or to "bf16d" (bf16 activations) --------
# key:      what switches the row on (`_direct_passes_on`): a pass name of ops.DIRECT_PASSES, or a key of `_DIRECT_SWITCHES`
# bf16:     the activation dtype the row is for: False fp32, True bf16
# replaces: the answers of the chain before it (`_select` / `_select_wrw`, then the bf16 chain of `_select_any` / `_select_wrw_any`) the row
#           may replace;  when(base, op, lay): what else must hold (op None for "wrw")
# `_direct_opt_in` adds what every row shares: mode "auto" only (a forced engine is never overridden), for the bf16 rows IPSR_BF16_ENGINES unset
# as well (the A/B values "all" / "none" are not overridden either), and the engine must take the layer.
_DirectOptIn = namedtuple("_DirectOptIn", "key kind engine bf16 replaces when")
_DIRECT_OPT_INS = (
    # the k3 s1 p1 forward / input gradient of "winograd": every shape the kernel takes, won or lost (profiles/direct_bf16x3_layers.txt)
    _DirectOptIn("k3_data", "data", "bf16x3d", False, ("winograd",), lambda base, op, lay: True),
    # "direct_bf16x3_s2" / "direct_bf16x3_s2_dw": the k4 s2 p1 forward / input-gradient passes that "wino_s2" has go to the direct split-bf16
    # kernel (ops.conv4x4s2_bf16x3) where it takes the shape.  Measured at batch 8 on every such row of the step
    # (profiles/direct_bf16x3_s2_layers.txt): 1.23-2.51x "wino_s2" (0.037-0.106 vs 0.079-0.197 ms), every row's slowest round of the kernel
    # faster than the fastest of "wino_s2", no row loses — so the rule is every "wino_s2" data pass the kernel takes; other batches and
    # channel counts inside it were not measured.  Of MIOpen's k4 s2 p1 rows the kernel takes one in the step, netG's outermost
    # ConvTranspose2d 64 -> 64 @128 input gradient (0.072 vs 0.197 ms, 2.72x): that shape moves too, at any batch though only batch 8 was
    # measured; nothing else of MIOpen's does.
    _DirectOptIn("s2_data", "data", "bf16x3d", False, ("wino_s2", "miopen"), lambda base, op, lay: _s2_geometry(lay) is not None and (
        base != "miopen" or (_s2_mode(op) == ops.S2_FINE_TO_COARSE and _s2_geometry(lay) == (64, 64, 128, 128)))),
    # `set_direct_dilated(True)`: the forward / input-gradient passes of the dilated down convolution that "wino_dil" has go to the direct
    # split-bf16 kernel wherever it takes the shape (coarse grids 16 .. 128 wide) — every such shape, won or lost.  Measured at batch 8 on the
    # step's four shapes (profiles/direct_bf16x3_dil_layers.txt, vs "wino_dil", forward / input gradient): 64 @256 wins 2.16x / 2.61x,
    # 128 @128 wins 1.55x / 1.72x, 512 @32 wins 1.47x / 1.30x, 256 @64 LOSES 0.82x / 0.93x; the switch moves all four, the step gains 1.5 %.
    # netD's k4 s1 p1 and the weight gradient stay on "wino_dil".
    _DirectOptIn("dil_data", "data", "bf16x3d", False, ("wino_dil",),
                 lambda base, op, lay: op in (ops.CONV_FWD, ops.CONV_BWD_DATA) and _dil_geometry(lay) is not None),
    # "direct_bf16x3_dw" / "direct_bf16x3_s2" / "direct_bf16x3_s2_dw": the k3 s1 p1 weight gradients that "winograd" / "miopen" have go to
    # the direct split-bf16 kernel (ops.conv3x3_bf16x3_wrw) on the shapes it takes from 32x32 maps up (`_bf16_direct_wrw`'s floor).  Measured
    # at batch 8 (profiles/direct_bf16x3_wrw_layers.txt): 2.6x MIOpen on 128 -> 128 @128x128, 1.2x / 1.5x the fp32 Winograd weight gradient
    # on 256 -> 256 / 512 -> 128 @64x64; 512 -> 512 @32x32 loses to it (0.136 vs 0.119 ms: the F(3x3,4x4) GEMM does 4x fewer
    # multiplications and its transforms are small there), so maps below 64x64 with >= 512 channels on both sides stay where they are.
    _DirectOptIn("k3_wrw", "wrw", "bf16x3w", False, ("winograd", "miopen"), lambda base, op, lay: lay[6:] == (3, 1, 1, 1) and lay[3] * lay[4] >= 1024
                 and not (lay[3] * lay[4] < 4096 and min(lay[2], lay[5]) >= 512)),
    # "direct_bf16x3_s2_dw": the k4 s2 p1 weight gradients that "wino_s2" has go to the direct split-bf16 kernel (ops.conv4x4s2_bf16x3_wrw)
    # where it takes the shape (coarse grids 16, 32 or 64 wide).  Measured at batch 8 on every such row of the step
    # (profiles/direct_bf16x3_s2_wrw_layers.txt): 1.21-1.87x "wino_s2" (0.050-0.091 vs 0.079-0.145 ms), every row's slowest round of the
    # kernel faster than the fastest of "wino_s2" (the closest: Conv2d 64 -> 128 on a 64-wide coarse grid, 0.0823 vs 0.0947), no row loses —
    # so the rule is every "wino_s2" weight gradient the kernel takes; other batches and the channel counts / grids `_s2_wins` admits beyond
    # the step's were not measured.  MIOpen's rows ("thin_mfma"'s 3-channel ends, netG's outermost 64 -> 64 on a 128-wide coarse grid, which
    # the kernel refuses), "smallmap", "one", the dilated family and grids below 16 wide stay where they are.
    _DirectOptIn("s2_wrw", "wrw", "bf16x3w", False, ("wino_s2",), lambda base, op, lay: _s2_geometry(lay) is not None),
    # `set_direct_dilated_dw(True)`: the weight gradients of the dilated down convolution that "wino_dil" has go to the direct split-bf16
    # kernel (ops.conv4x4s2_bf16x3_dil_wrw) wherever it takes the shape (coarse grids 16 .. 128 wide) — every such shape, won or lost.
    # Measured at batch 8 on the step's shapes (profiles/direct_bf16x3_dil_wrw_layers.txt): 1.84x "wino_dil" on 128 @128 (0.079 vs
    # 0.146 ms), 1.30x on 256 @64, 1.13x on 512 @32, the ranges apart in every row.  Of MIOpen's rows exactly one moves, at any batch though
    # only batch 8 was measured: 64 -> 64 @256x256, where the kernel's slowest round (0.1412 ms) is faster than MIOpen's fastest
    # (0.2164 ms), 1.68x on the medians.  The step gains 0.8-1.0 %.  netD's k4 s1 p1, "smallmap" grids and bf16 activations stay where they are.
    _DirectOptIn("dil_wrw", "wrw", "bf16x3w", False, ("wino_dil", "miopen"), lambda base, op, lay: _dil_geometry(lay) is not None and (
        base != "miopen" or _dil_geometry(lay) == _DIL_WRW_MIOPEN_ROW)),
    # bf16 activations under `set_direct_dilated_bf16(True)`: the forward / input-gradient passes of the dilated down convolution that the
    # chain answers "wino_dil" (kept by `_bf16_wins`: >= 256 channels up to 64x64) or "miopen" (the rest) go to the direct bf16 kernel
    # wherever it takes the shape (coarse grids 16 .. 128 wide) — every such shape, won or lost, the rule `set_direct_dilated` follows for
    # fp32.  Mode "auto" with IPSR_BF16_ENGINES unset only; "smallmap" grids, the weight gradient and netD's k4 s1 p1 stay.
    # Against the switch-off answer at batch 16 on the step's four shapes (profiles/direct_bf16_dil_layers.txt, forward / input gradient):
    # 64 -> 64 @256 against MIOpen 1.93x / 2.53x (0.077 / 0.073 vs 0.149 / 0.186 ms), 128 -> 128 @128 against MIOpen 1.75x / 2.47x, 256 -> 256 @64
    # against "wino_dil" 0.93x (LOSES, 0.086 vs 0.081 ms) / 1.13x, 512 -> 512 @32 against "wino_dil" 1.05x / 0.84x (LOSES, 0.091 vs 0.076 ms); every
    # row's ranges apart.  The switch moves all eight passes; the config-5 step rate goes from 821.3 to 834.4 images/s (+1.6 %, five alternated
    # rounds, the ranges apart).  Other batches and channel counts inside the kernel's limits were not measured.
    _DirectOptIn("bf16_dil_data", "data", "bf16d", True, ("wino_dil", "miopen"),
                 lambda base, op, lay: op in (ops.CONV_FWD, ops.CONV_BWD_DATA) and _dil_geometry(lay) is not None),
    # bf16 activations under `set_direct_dilated_bf16_dw(True)`: the weight gradient of the dilated down convolution that the chain answers
    # "wino_dil" (kept by `_bf16_wins`: >= 256 channels up to 64x64) or "miopen" (the rest) goes to the direct bf16 kernel wherever it takes the
    # shape (coarse grids 16 .. 128 wide) — every such shape, won or lost, the rule `set_direct_dilated_bf16` follows for the data passes.  Mode
    # "auto" with IPSR_BF16_ENGINES unset only; "smallmap" grids (answered before this), netD's k4 s1 p1 and transposed layers stay.
    # Against the switch-off answer at batch 16 on the step's four shapes (profiles/direct_bf16_dil_wrw_layers.txt): 64 -> 64 @256 against MIOpen
    # 1.37x (0.117 vs 0.160 ms), 128 -> 128 @128 against MIOpen 1.62x, 256 -> 256 @64 against "wino_dil" 1.50x, 512 -> 512 @32 against "wino_dil"
    # 0.64x (LOSES, 0.131 vs 0.084 ms: 16 runs of 16.8 MB slabs); every row's ranges apart.  The switch moves all four; the config-5 step rate
    # goes from 829.5 to 833.2 images/s with `set_direct_dilated_bf16` on in both columns (+0.4 %, five alternated rounds, the ranges apart).
    # Other batches and channel counts inside the kernel's limits were not measured.
    _DirectOptIn("bf16_dil_wrw", "wrw", "bf16d", True, ("wino_dil", "miopen"), lambda base, op, lay: _dil_geometry(lay) is not None),
)


def _direct_opt_in(kind, base, op, lay, bf16):
    """-> the engine of the first row of `_DIRECT_OPT_INS` for this activation dtype that moves this pass off its base answer, else `base`."""
    if _mode() != "auto" or (bf16 and _env("IPSR_BF16_ENGINES", "") != ""):
        return base
    on = _direct_passes_on()
    for row in _DIRECT_OPT_INS:
        if row.kind == kind and row.bf16 == bool(bf16) and row.key in on and base in row.replaces and row.when(base, op, lay) \
                and engine_takes(row.engine, kind, op, lay, bf16):
            return row.engine
    return base


def _select_wrw(lay):
    transposed, B, Cin, H, W, Cout, k, stride, pad, dil = lay
    mode = _mode()
    if mode == "auto" and not transposed and Cout == 1 and Cin >= 64 and engine_takes("one", "wrw", None, lay, False):
        return "one"
    if mode == "auto" and not transposed and _is_dilated4(k, stride, pad, dil) and min(Cin, Cout) >= 128 and 32 <= H <= 128 \
            and H % 2 == 0 and W % 2 == 0:
        return "wino_dil"
    if mode == "auto" and not transposed and _is_k4s1(k, stride, pad, dil) and min(Cin, Cout) >= 128 and 16 <= H <= 128 and W >= 4:
        return "wino_dil"
    if mode == "auto":
        g = _s2_geometry(lay)
        if g is not None and _s2_wins(g):
            return "wino_s2"
    if mode == "auto" and _smallmap_wrw_wins(lay):
        return "smallmap"
    ok = k == 3 and stride == 1 and pad == 1 and dil == 1
    if mode in ("miopen", "direct") or not ok:
        return "miopen"
    if mode == "winograd":
        return "winograd"
    if 256 <= H * W <= 4096 and max(Cin, Cout) >= 256 and min(Cin, Cout) >= 128:
        return "winograd"
    if transposed and Cout == 64 and Cin >= 256 and H * W <= 16384:
        return "winograd"        # netG upconv_1 (256 -> 64 @128x128): the one large-map weight gradient that is ahead, 0.365 vs 0.409 ms
    return "miopen"


# ---- the engines: one record each, the source of the list in the module docstring -----------------------------------------------------
# data:  (op, inp, w, lay, math, out_dtype, param) -> y / dx: forward (inp = x) and input gradient (inp = dy) share the call
# wrw:   (x, dy, lay, math, sink) -> dW (fp32, the module's layout); None: the engine has no such pass
#        ("miopen" has neither: it runs through _miopen_forward / _miopen_backward).  lay[1:5] = (B, Cin, H, W), lay[5] = Cout, lay[6:] = (k, stride, pad, dil)
# takes: (kind, op, lay, bf16) -> whether the engine accepts this pass of this layer: kind "data" (op = the ops.* code of the forward / input-
#        gradient pass) or "wrw" (op ignored); bf16 = the activations are bf16.  The support query of the entry point the `data` / `wrw` call
#        reaches, with the arguments that call builds; False for a pass the engine has not, or a geometry its call cannot express.  Ask
#        through `engine_takes`.  (tests/dispatch_envelope.py restates the mapping on its own.)
# bf16_io:    reads / writes bf16 activation tensors in competition with MIOpen's bf16 kernels: the engines `_bf16_wins` rules on (the thin
#              engines read bf16 too, by rules of their own in `_select_any` / `_select_wrw_any`)
# fp32_copies: an fp32 engine whose operands are small next to its weight stream / single pass (the innermost levels, netD's one-channel
#              head): under bf16 activations it runs on fp32 copies of the activations (a cast of a few hundred KB) instead of falling
#              back to MIOpen's transposes + 40-160 us kernels
# sink:        data parallel: may write the weight gradient straight into its slice of the armed gradient bucket (dist.py)
# wrw_x_as_dy: a weight gradient that reads both operands in one dtype: x is cast to dy's
_Engine = namedtuple("_Engine", "data wrw takes bf16_io fp32_copies sink wrw_x_as_dy", defaults=(None, None, None, False, False, False, False))
_K3 = (3, 1, 1, 1)         # (k, stride, pad, dil)


def engine_takes(eng, kind, op, lay, bf16):
    """Whether the engine accepts one pass of one layer (`_Engine.takes`); "miopen" takes everything."""
    return eng == "miopen" or bool(_ENGINES[eng].takes(kind, op, lay, bf16))


def _frozen_pack(w, param):
    """-> the keep_packed / pack_key arguments of the direct 3x3 data passes.  param: the module's weight Parameter when `w` is a detached
    view of it (the no-grad path).  Frozen weights (a leaf Parameter with requires_grad False, outside autograd) keep their packed image,
    cached under the Parameter."""
    param = w if param is None else param
    return dict(keep_packed=isinstance(param, nn.Parameter) and not param.requires_grad and not torch.is_grad_enabled(), pack_key=param)


def _fine_coarse(x, dy, lay):
    """(fine, coarse, B, Kc, Cf, nh, nw): the operands of a k4 s2 p1 weight gradient in the terms of the coarse / fine entries."""
    return ((dy, x) if lay[0] else (x, dy)) + (lay[1],) + _s2_geometry(lay)


def _direct_case(lay):
    """-> (case, g): which entry points of csrc/conv_bf16.hip a layer reaches on the direct bf16 / split-bf16 engines, from its geometry alone —
    "k3" (k3 s1 p1), "s2" (k4 s2 p1, g = `_s2_geometry`), "dil" (the dilated down convolution, g = `_dil_geometry`) — or (None, None) where
    their calls cannot express the layer.  The run calls and the `takes` of "bf16d" / "bf16x3d" / "bf16x3w" look `_DIRECT_ENTRIES` up by it."""
    if lay[6:] == _K3:
        return "k3", None
    dilated = _is_dilated4(*lay[6:])
    g = _dil_geometry(lay) if dilated else _s2_geometry(lay)
    return (None if g is None else "dil" if dilated else "s2"), g


# What the direct engines reach: (x3, case, kind) -> the ops.* call that runs the pass, its support query, and the mode argument of the k4 data
# entries as a function of the pass's op.  x3: False = the bf16 kernels ("bf16d"), True = the split-bf16 ones on fp32 tensors ("bf16x3d" data,
# "bf16x3w" weight gradient); case: `_direct_case`.  Names, not functions: looked up in `ops` at the call.  The split-bf16 dilated data pass is
# the k4 s2 entry with ops.S2_DILATED or-ed into the mode; the bf16 one is an entry of its own that takes the plain mode.
_DirectEntry = namedtuple("_DirectEntry", "run supported mode", defaults=(None,))
_DIRECT_ENTRIES = {
    (False, "k3", "data"): _DirectEntry("conv3x3_bf16", "conv3x3_bf16_supported"),
    (False, "k3", "wrw"): _DirectEntry("conv3x3_bf16_wrw", "conv3x3_bf16_wrw_supported"),
    (False, "s2", "data"): _DirectEntry("conv4x4s2_bf16", "conv4x4s2_bf16_supported", _s2_mode),
    (False, "s2", "wrw"): _DirectEntry("conv4x4s2_bf16_wrw", "conv4x4s2_bf16_wrw_supported"),
    (False, "dil", "data"): _DirectEntry("conv4x4s2_bf16_dil", "conv4x4s2_bf16_dil_supported", lambda op: _dil_mode(op) & ~ops.S2_DILATED),
    (False, "dil", "wrw"): _DirectEntry("conv4x4s2_bf16_dil_wrw", "conv4x4s2_bf16_dil_wrw_supported"),
    (True, "k3", "data"): _DirectEntry("conv3x3_bf16x3", "conv3x3_bf16x3_supported"),
    (True, "k3", "wrw"): _DirectEntry("conv3x3_bf16x3_wrw", "conv3x3_bf16x3_wrw_supported"),
    (True, "s2", "data"): _DirectEntry("conv4x4s2_bf16x3", "conv4x4s2_bf16x3_supported", _s2_mode),
    (True, "s2", "wrw"): _DirectEntry("conv4x4s2_bf16x3_wrw", "conv4x4s2_bf16x3_wrw_supported"),
    (True, "dil", "data"): _DirectEntry("conv4x4s2_bf16x3", "conv4x4s2_bf16x3_supported", _dil_mode),
    (True, "dil", "wrw"): _DirectEntry("conv4x4s2_bf16x3_dil_wrw", "conv4x4s2_bf16x3_dil_wrw_supported"),
}
# The one place an engine's `takes` asks a switch: "bf16d" takes a pass of the dilated layer only while that pass's switch is on, so
# `engine_takes("bf16d", ...)` follows `set_direct_dilated_bf16` / `set_direct_dilated_bf16_dw`.  "bf16x3d" / "bf16x3w" do NOT follow
# `set_direct_dilated` / `set_direct_dilated_dw`: they take the dilated layer whatever the switches say, and only their rows of
# `_DIRECT_OPT_INS` ask.  The asymmetry is how the two pairs were written; levelling it would change what `engine_takes` answers.
_DIRECT_TAKES_SWITCH = {(False, "dil", "data"): "bf16_dil_data", (False, "dil", "wrw"): "bf16_dil_wrw"}


def _direct_data(x3, op, inp, w, lay, math, out_dtype, param):
    """One pass of a module on the direct kernels (csrc/conv_bf16.hip): k3 s1 p1, or k4 s2 p1 / the dilated k4 s2 p3 d2 in their coarse / fine
    form.  The bf16 kernels read bf16 tensors and write `out_dtype`; the split-bf16 ones read and write fp32."""
    case, g = _direct_case(lay)
    e = _DIRECT_ENTRIES[x3, case, "data"]
    kw = {}
    if not x3:
        kw["out_dtype"] = out_dtype
        if inp.dtype != torch.bfloat16:
            inp = inp.to(torch.bfloat16)
    if case == "k3":
        return getattr(ops, e.run)(op, inp, w, lay[1:5], lay[5], **kw, **_frozen_pack(w, param))
    return getattr(ops, e.run)(e.mode(op), inp, w, lay[1], *g, **kw)


def _direct_wrw(x3, x, dy, lay, math, sink):
    case, g = _direct_case(lay)
    run = getattr(ops, _DIRECT_ENTRIES[x3, case, "wrw"].run)
    if case == "k3":
        return run(lay[0], x, dy, lay[5], out=sink)
    return run(*((dy, x) if lay[0] else (x, dy)), lay[1], *g, out=sink)      # (fine, coarse) as in `_fine_coarse`; the dilated layer is Conv2d only


def _direct_takes(x3, kind, op, lay, bf16):
    case, g = _direct_case(lay)
    e = _DIRECT_ENTRIES.get((x3, case, kind))
    switch = _DIRECT_TAKES_SWITCH.get((x3, case, kind))
    if e is None or bool(bf16) == x3 or (switch is not None and switch not in _direct_passes_on()):      # "bf16d" reads bf16 activations, the
        return False                                                                                     # split-bf16 pair fp32 ones
    supported = getattr(ops, e.supported)
    if case == "k3":
        return supported(op, *lay[1:6]) if kind == "data" else supported(*lay[:6])
    return supported(e.mode(op), lay[1], *g) if kind == "data" else supported(lay[1], *g)


def _thin_mfma_wrw(x, dy, lay, math, sink):
    if lay[0] and dy.dtype == torch.bfloat16 and x.dtype != torch.bfloat16:
        x = x.to(torch.bfloat16)                 # the WIDE tensor decides the arithmetic
    return ops.conv_thin_wrw_mfma(lay[0], x, dy, lay[6], lay[7], out=sink)


def _winograd_takes(kind, op, lay, bf16):
    if lay[6:] != _K3:
        return False
    if kind == "data":
        return ops.winograd_supported(op, *lay[1:6])
    return _lib.lib().ipsr_conv3x3_winograd_wrw_workspace_bytes(int(lay[0]), *lay[1:6]) > 0      # (ops has no *_supported for it)


def _wino_dil_mode(kind, op):
    """Mode of ops.conv4x4_dilated_winograd: 0 forward, 1 input gradient, 2 weight gradient."""
    return 2 if kind == "wrw" else int(op != ops.CONV_FWD)


def _wino_dil_takes(kind, op, lay, bf16):
    g = ops.conv4x4_geometry(*lay[6:])
    return g is not None and not lay[0] and ops.dilated_winograd_supported(_wino_dil_mode(kind, op), *lay[1:6], geom=g)


def _wino_s2_takes(kind, op, lay, bf16):
    g = _s2_geometry(lay)
    return g is not None and ops.s2_winograd_supported(_s2_mode(op) if kind == "data" else ops.S2_WEIGHT_GRAD, lay[1], *g)


_ENGINES = {
    "winograd": _Engine(
        lambda op, inp, w, lay, math, out_dtype, param: ops.conv3x3_winograd(op, inp, w, lay[1:5], lay[5], math=math, out_dtype=out_dtype),
        lambda x, dy, lay, math, sink: ops.conv3x3_winograd_wrw(lay[0], x, dy, lay[5], out=sink, math=math),
        _winograd_takes, bf16_io=True, sink=True, wrw_x_as_dy=True),
    "wino_dil": _Engine(
        lambda op, inp, w, lay, math, out_dtype, param: ops.conv4x4_dilated_winograd(
            _wino_dil_mode("data", op), inp, w, lay[1:5], lay[5], geom=ops.conv4x4_geometry(*lay[6:]), math=math, out_dtype=out_dtype),
        lambda x, dy, lay, math, sink: ops.conv4x4_dilated_winograd(
            _wino_dil_mode("wrw", None), x, dy, lay[1:5], lay[5], out=sink, geom=ops.conv4x4_geometry(*lay[6:]), math=math),
        _wino_dil_takes, bf16_io=True, sink=True, wrw_x_as_dy=True),
    "wino_s2": _Engine(          # the weight gradient takes (fine, coarse)
        lambda op, inp, w, lay, math, out_dtype, param: ops.conv4x4s2_winograd(_s2_mode(op), inp, w, lay[1], *_s2_geometry(lay), math=math, out_dtype=out_dtype),
        lambda x, dy, lay, math, sink: ops.conv4x4s2_winograd(ops.S2_WEIGHT_GRAD, *_fine_coarse(x, dy, lay), out=sink, math=math),
        _wino_s2_takes, bf16_io=True, sink=True, wrw_x_as_dy=True),
    "thin": _Engine(
        lambda op, inp, w, lay, math, out_dtype, param: ops.conv3x3_thin(op, inp, w, lay[1:5], lay[5], out_dtype=out_dtype),
        takes=lambda kind, op, lay, bf16: kind == "data" and lay[6:] == _K3 and ops.thin_supported(op, *lay[2:6])),
    "thin_f2m": _Engine(
        lambda op, inp, w, lay, math, out_dtype, param: ops.conv_thin_f2m_mfma(op, inp, w, lay[1:5], lay[5], lay[6], lay[7], out_dtype=out_dtype),
        takes=lambda kind, op, lay, bf16: kind == "data" and lay[8:] == (1, 1) and ops.thin_f2m_mfma_supported(op, *lay[1:8])),
    "thin_mfma": _Engine(
        None, _thin_mfma_wrw, sink=True,
        takes=lambda kind, op, lay, bf16: kind == "wrw" and lay[8:] == (1, 1) and ops.thin_wrw_mfma_supported(*lay[:8])),
    "smallmap": _Engine(         # the weight gradient takes (coarse, fine); tiled: the pass was admitted through the caller's reach
        lambda op, inp, w, lay, math, out_dtype, param, tiled=False: ops.conv_smallmap(_smallmap_op(op), inp, w, *_smallmap_geometry(lay), tiled=tiled),
        lambda x, dy, lay, math, sink, tiled=False: ops.conv_smallmap(ops.SM_WRW, *((x, dy) if lay[0] else (dy, x)), *_smallmap_geometry(lay), out=sink,
                                                                       tiled=tiled),
        lambda kind, op, lay, bf16, tiled=False: ops.smallmap_supported(_smallmap_op(op) if kind == "data" else ops.SM_WRW, *_smallmap_geometry(lay),
                                                                         tiled=tiled),
        fp32_copies=True, sink=True),
    "direct": _Engine(
        lambda op, inp, w, lay, math, out_dtype, param: ops.conv2d(op, inp, w, lay[1:5], *lay[5:]),
        takes=lambda kind, op, lay, bf16: kind == "data" and ops.conv2d_supported(op, *lay[1:])),
    "one": _Engine(              # Conv2d forward and weight gradient only
        lambda op, inp, w, lay, math, out_dtype, param: ops.conv_to_one(inp, w, lay[8]),
        lambda x, dy, lay, math, sink: ops.conv_to_one_wrw(x, dy, lay[6], lay[8], out=sink),
        lambda kind, op, lay, bf16: not lay[0] and lay[5] == 1 and (kind == "wrw" or op == ops.CONV_FWD) and ops.conv_to_one_supported(*lay[1:5], *lay[6:]),
        fp32_copies=True, sink=True),
    "bf16d": _Engine(partial(_direct_data, False), partial(_direct_wrw, False), partial(_direct_takes, False), bf16_io=True, sink=True, wrw_x_as_dy=True),
    "bf16x3d": _Engine(partial(_direct_data, True), takes=lambda kind, op, lay, bf16: kind == "data" and _direct_takes(True, kind, op, lay, bf16)),
    "bf16x3w": _Engine(None, partial(_direct_wrw, True), lambda kind, op, lay, bf16: kind == "wrw" and _direct_takes(True, kind, op, lay, bf16), sink=True),
    "miopen": _Engine(),
}


def _run_data(eng, op, inp, w, lay, math, out_dtype, param=None, tiled=False):
    """Forward (inp = x) or input gradient (inp = dy) of one layer on a HIP engine; `inp` contiguous.  tiled: `_via_reach` ("smallmap" only)."""
    e = _ENGINES[eng]
    kw = {"tiled": True} if tiled else {}
    if e.fp32_copies:
        return e.data(op, inp.float(), w, lay, math, torch.float32, param, **kw).to(out_dtype)
    return e.data(op, inp, w, lay, math, out_dtype, param, **kw)


def _run_wrw(eng, x, dy, w, lay, math, tiled=False):
    """Weight gradient of one layer on a HIP engine (fp32, the module's layout); x, dy contiguous.  tiled: as in `_run_data`."""
    e = _ENGINES[eng]
    sink = ipsr_dist.grad_sink_for(w.data_ptr(), w.shape) if e.sink else None
    if e.fp32_copies:
        x, dy = x.float(), dy.float()
    elif e.wrw_x_as_dy and x.dtype != dy.dtype:
        x = x.to(dy.dtype)
    return e.wrw(x, dy, lay, math, sink, **({"tiled": True} if tiled else {}))


def _miopen_forward(x, w, transposed, stride, pad, dil):
    if x.dtype != w.dtype and not torch.is_autocast_enabled():
        w = w.to(x.dtype)
    return F.conv_transpose2d(x, w, None, stride, pad, 0, 1, dil) if transposed else F.conv2d(x, w, None, stride, pad, dil)


def _miopen_backward(dy, x, w, transposed, stride, pad, dil, which):
    """aten.convolution_backward on operands of ONE dtype (bf16 activations: the fp32 weight is cast, its gradient cast back)."""
    dt = dy.dtype
    out = torch.ops.aten.convolution_backward(dy, x if x.dtype == dt else x.to(dt), w if w.dtype == dt else w.to(dt), None, [stride, stride],
                                              [pad, pad], [dil, dil], transposed, [0, 0], 1, which)
    return out[0], (out[1].to(w.dtype) if out[1] is not None else None)


class _HipConv(torch.autograd.Function):
    """Bias-free Conv2d / ConvTranspose2d: forward, input gradient and weight gradient each on the engine `select` names for it
    (MIOpen where none is faster).  `math` = the Winograd engines' arithmetic, `act` = dtype of the activation tensors produced."""

    @staticmethod
    def forward(ctx, x, w, lay, eng_fwd, math, act, reach=None):
        transposed, B, Cin, H, W, Cout, k, stride, pad, dil = lay
        xc = x.contiguous()
        if eng_fwd == "miopen":
            y = _miopen_forward(xc, w, transposed, stride, pad, dil)
        else:
            fop = ops.CONVT_FWD if transposed else ops.CONV_FWD
            y = _run_data(eng_fwd, fop, xc, w, lay, math, act, tiled=eng_fwd == "smallmap" and _via_reach("data", fop, lay, act == torch.bfloat16, reach))
        ctx.save_for_backward(xc, w)
        ctx.lay, ctx.geom = lay, (transposed, k, stride, pad, dil, Cout)
        ctx.math, ctx.bf16, ctx.reach = math, act == torch.bfloat16, reach
        if _check_hook is not None:
            _check_hook("forward", eng_fwd, ctx.geom, (xc, w), y)
        return y

    @staticmethod
    def backward(ctx, dy):
        x, w = ctx.saved_tensors
        lay, math, bf16, reach = ctx.lay, ctx.math, ctx.bf16, ctx.reach
        transposed, B, Cin, H, W, Cout, k, stride, pad, dil = lay
        dy = dy.contiguous()
        if bf16 and dy.dtype != torch.bfloat16:
            dy = dy.to(torch.bfloat16)
        dx = dw = None
        if ctx.needs_input_grad[0]:
            op = ops.CONVT_BWD_DATA if transposed else ops.CONV_BWD_DATA
            eng = select(op, B, Cin, H, W, Cout, k, stride, pad, dil, bf16, reach=reach)
            if eng == "miopen":
                dx = _miopen_backward(dy, x, w, transposed, stride, pad, dil, [True, False, False])[0]
                if dx.dtype != x.dtype:
                    dx = dx.to(x.dtype)
            else:
                dx = _run_data(eng, op, dy, w, lay, math, x.dtype, tiled=eng == "smallmap" and _via_reach("data", op, lay, bf16, reach))
            if _check_hook is not None:
                _check_hook("input_grad", eng, ctx.geom, (dy, x, w), dx)
        if ctx.needs_input_grad[1]:
            weng = select_wrw(transposed, B, Cin, H, W, Cout, k, stride, pad, dil, bf16, reach=reach)
            if weng == "miopen":
                dw = _miopen_backward(dy, x, w, transposed, stride, pad, dil, [False, True, False])[1]
            else:
                dw = _run_wrw(weng, x, dy, w, lay, math, tiled=weng == "smallmap" and _via_reach("wrw", None, lay, bf16, reach))
            if _check_hook is not None:
                _check_hook("weight_grad", weng, ctx.geom, (dy, x, w), dw)
        return dx, dw, None, None, None, None, None


def _geometry(m):
    """(k, stride, pad, dil) of a module the kernels can express (square, symmetric, groups 1, no output padding) or None."""
    ks, st, pd, dl = m.kernel_size, m.stride, m.padding, m.dilation
    if m.groups != 1 or ks[0] != ks[1] or st[0] != st[1] or pd[0] != pd[1] or dl[0] != dl[1] or isinstance(pd, str):
        return None
    if isinstance(m, nn.ConvTranspose2d) and tuple(m.output_padding) != (0, 0):
        return None
    if getattr(m, "padding_mode", "zeros") != "zeros":
        return None
    return ks[0], st[0], pd[0], dl[0]


def _layer_of(m, x, w):
    """-> (lay, bf16) when the call m(x) with the weight w is one the engines can take (a 4-d fp32 / bf16 GPU tensor, fp32 weights, no
    autocast other than bf16), else None.  bf16: the activations are bf16 (a bf16 tensor, or any input under bf16 autocast)."""
    g = _geometry(m)
    if g is None or not x.is_cuda or x.dim() != 4 or w.dtype != torch.float32 or x.dtype not in (torch.float32, torch.bfloat16):
        return None
    amp = _amp_bf16()
    if not amp and torch.is_autocast_enabled():
        return None
    transposed = isinstance(m, nn.ConvTranspose2d)
    B, Cin, H, W = x.shape
    return (transposed, B, Cin, H, W, w.shape[1] if transposed else w.shape[0]) + g, amp or x.dtype == torch.bfloat16


def conv_math(bf16):
    """The arithmetic (ops.MATH_CODE) the Winograd engines run under fp32 (False) / bf16 (True) activations: see `set_conv_math`."""
    return _MATH["bf16" if bf16 else "fp32"]


def _engines_of(lay, bf16, dx=True, dw=True, reach=None):
    """-> the engines of (forward, input gradient, weight gradient) of one layer; a gradient nobody needs (dx / dw False) is not asked for
    and reads "miopen".  reach: the module's `smallmap_reach` (`select`)."""
    transposed, B, Cin, H, W, Cout, k, stride, pad, dil = lay
    fop, bop = (ops.CONVT_FWD, ops.CONVT_BWD_DATA) if transposed else (ops.CONV_FWD, ops.CONV_BWD_DATA)
    return (select(fop, B, Cin, H, W, Cout, k, stride, pad, dil, bf16, reach=reach),
            select(bop, B, Cin, H, W, Cout, k, stride, pad, dil, bf16, reach=reach) if dx else "miopen",
            select_wrw(transposed, B, Cin, H, W, Cout, k, stride, pad, dil, bf16, reach=reach) if dw else "miopen")


def any_engine(m, x):
    """True when at least one pass of m(x) would run on a HIP engine (so the caller should split the bias off and come through
    conv_nobias); False = all three passes are MIOpen's and the plain module call loses nothing."""
    lb = _layer_of(m, x, m.weight)
    if lb is None:
        return False
    return _engines_of(*lb, reach=getattr(m, "smallmap_reach", None)) != ("miopen",) * 3


def conv_nobias(m, x, weight=None):
    """m(x) without the bias (the fused epilogue kernels add it): HIP engine where `select` says so, else MIOpen.  fp32 activations:
    every engine; bf16 activations (a bf16 tensor, or any input under bf16 autocast — BASELINE config 5): the engines that read / write
    bf16 or run on fp32 copies (`_ENGINES`), the Winograd ones on split-bf16 operands (`_MATH`); the weights stay fp32 parameters."""
    w = m.weight if weight is None else weight
    lb = _layer_of(m, x, w)
    if lb is not None:
        lay, bf16 = lb
        act = torch.bfloat16 if bf16 else torch.float32
        math = _MATH["bf16" if bf16 else "fp32"]
        grad = torch.is_grad_enabled()
        reach = getattr(m, "smallmap_reach", None)       # stamped by the trainer (models/IPSR.py); a bare module has none
        engs = _engines_of(lay, bf16, grad and x.requires_grad, grad and w.requires_grad, reach)
        if grad and (x.requires_grad or w.requires_grad):
            # the backward may use a HIP engine even where the forward stays on MIOpen
            if engs != ("miopen",) * 3:
                return _HipConv.apply(x, w, lay, engs[0], math, act, reach)
        elif engs[0] != "miopen":
            fop = ops.CONVT_FWD if lay[0] else ops.CONV_FWD
            return _run_data(engs[0], fop, x.contiguous(), w.detach(), lay, math, act, param=w,
                             tiled=engs[0] == "smallmap" and _via_reach("data", fop, lay, bf16, reach))
    if isinstance(m, nn.ConvTranspose2d):
        return F.conv_transpose2d(x, w, None, m.stride, m.padding, m.output_padding, m.groups, m.dilation)
    return F.conv2d(x, w, None, m.stride, m.padding, m.dilation, m.groups)
