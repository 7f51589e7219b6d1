#!/usr/bin/env python3
"""The direct split-bf16 3x3 convolution on fp32 tensors (ops.conv3x3_bf16x3, engine "bf16x3d", opt.conv_math="direct_bf16x3"):

  layers   the training step's k3 s1 p1 shapes at batch 8, forward and input gradient: device time of the new engine, of the fp32
           Winograd engine, of the split-bf16 ("bf16x3") Winograd engine and of MIOpen, and each one's error against an fp64
           convolution (max |err| / max |y64|, first two images).  Times are HIP events around `--iters` back-to-back calls, the
           engines alternated over `--rounds` rounds, median of the rounds (min .. max in brackets for the new engine).
  wrw      the weight gradient of the same shapes, as Conv2d and as ConvTranspose2d (ops.conv3x3_bf16x3_wrw, engine "bf16x3w",
           opt.conv_math="direct_bf16x3_dw"): the new engine against the engine `select_wrw` answers for the shape by default, same
           process, same rounds; err = max |dW - dW64| / max |dW64| against the fp64 weight gradient of the whole batch.
  s2       every k4 s2 p1 layer of the step at batch 8, forward and input gradient (ops.conv4x4s2_bf16x3, engine "bf16x3d" under
           opt.conv_math="direct_bf16x3_s2"): the new kernel against the engine `select` answers for the shape under conv_math "fp32",
           same process, same rounds; err = max |y - y64| / max |y64| against the fp64 convolution (first two images).
  s2wrw    the weight gradient of the same k4 s2 p1 layers (ops.conv4x4s2_bf16x3_wrw, engine "bf16x3w" under
           opt.conv_math="direct_bf16x3_s2_dw"): the new kernel against the engine `select_wrw` answers for the shape under conv_math
           "fp32", same process, same rounds; err = max |dW - dW64| / max |dW64| against the fp64 weight gradient of the whole batch.
  dil      netG's dilated down convolutions Conv2d(C, C, k4, stride 2, pad 3, dilation 2) of the step at batch 8, forward and input
           gradient (ops.conv4x4s2_bf16x3 with ops.S2_DILATED, engine "bf16x3d" under hipconv.set_direct_dilated(True)): the new kernel
           against the engine `select` answers for the shape with the switch off, same process, same rounds; err = max |y - y64| / max |y64|
           against the fp64 convolution (first two images).
  dilwrw   the weight gradient of the same dilated layers (ops.conv4x4s2_bf16x3_dil_wrw, engine "bf16x3w" under
           hipconv.set_direct_dilated_dw(True)): the new kernel against the engine `select_wrw` answers for the shape with the switch off,
           same process, same rounds; err = max |dW - dW64| / max |dW64| against the fp64 weight gradient of the whole batch.
  steps    the whole fp32 training step of bench.py (its model, batch and step function) under conv_math "fp32", "direct_bf16x3",
           "direct_bf16x3_dw", "direct_bf16x3_s2", "direct_bf16x3_s2_dw" and "bf16x3" in ONE process, alternated over `--rounds` rounds
           (`--maths` narrows the list), each with hipconv.set_direct_dilated off and on (two columns; `--dilated off` / `on` keeps one) and,
           with `--dilated-dw both`, with hipconv.set_direct_dilated_dw off and on as further columns (default: off only).

    python tools/bench_direct_bf16x3.py [--what layers wrw s2 s2wrw dil dilwrw steps] [--out profiles/direct_bf16x3_layers.txt]
"""
import argparse
import os
import statistics
import sys
import time

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench  # noqa: E402  (private MIOpen db copy, the step function)
from deepinpainting_amd import ops  # noqa: E402

LAYERS = [("conv", 64, 256, 64), ("conv", 128, 128, 128), ("conv", 256, 64, 256), ("conv", 512, 32, 512), ("conv", 512, 16, 512), ("convT", 512, 64, 128)]


def burst_ms(fn, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters


def layers(B, iters, rounds, emit):
    g = torch.Generator(device="cuda").manual_seed(5)
    emit("batch %d, fp32 NCHW in and out; ms = device time per call (HIP events, %d calls per burst, median of %d alternated rounds); TF = useful flop / time" % (B, iters, rounds))
    emit("err = max |y - y64| / max |y64| against the fp64 convolution of the unrounded operands")
    emit("%-22s %-5s | %-31s | %-18s | %-18s | %-18s" % ("layer", "pass", "direct bf16x3  ms [min..max]  TF   err", "fp32 Winograd ms err", "bf16x3 Winograd ms err", "MIOpen ms err"))
    for kind, Cin, H, Cout in LAYERS:
        tr = kind == "convT"
        w = torch.randn((Cin, Cout, 3, 3) if tr else (Cout, Cin, 3, 3), device="cuda", generator=g) * (1.0 / (3.0 * (Cin ** 0.5)))
        x = torch.randn(B, Cin, H, H, device="cuda", generator=g)
        dy = torch.randn(B, Cout, H, H, device="cuda", generator=g)
        fop, bop = (ops.CONVT_FWD, ops.CONVT_BWD_DATA) if tr else (ops.CONV_FWD, ops.CONV_BWD_DATA)
        flops = 2.0 * 9 * Cin * Cout * B * H * H
        for name, op, inp in (("fwd", fop, x), ("bwdD", bop, dy)):
            shp = (B, Cin, H, H)
            if name == "fwd":
                mi = (lambda: F.conv_transpose2d(x, w, None, 1, 1)) if tr else (lambda: F.conv2d(x, w, None, 1, 1))
                f64 = F.conv_transpose2d if tr else F.conv2d
            else:
                mi = lambda: torch.ops.aten.convolution_backward(dy, x, w, None, [1, 1], [1, 1], [1, 1], tr, [0, 0], 1, [True, False, False])[0]
                f64 = F.conv2d if tr else F.conv_transpose2d
            ref = f64(inp[:2].double(), w.double(), None, 1, 1)
            engines = [("direct", lambda: ops.conv3x3_bf16x3(op, inp, w, shp, Cout)),
                       ("wino_fp32", lambda: ops.conv3x3_winograd(op, inp, w, shp, Cout, math="fp32")),
                       ("wino_bf16x3", lambda: ops.conv3x3_winograd(op, inp, w, shp, Cout, math="bf16x3")),
                       ("miopen", mi)]
            if not ops.conv3x3_bf16x3_supported(op, *shp, Cout):
                emit("%-5s %4d->%-4d @%-3d %-5s | unsupported" % (kind, Cin, Cout, H, name))
                continue
            err, ms = {}, {k: [] for k, _ in engines}
            for k, fn in engines:
                for _ in range(3):
                    y = fn()
                err[k] = float((y[:2].double() - ref).abs().max() / ref.abs().max())
            torch.cuda.synchronize()
            for _ in range(rounds):
                for k, fn in engines:
                    ms[k].append(burst_ms(fn, iters))
            md = {k: statistics.median(v) for k, v in ms.items()}
            emit("%-5s %4d->%-4d @%-3d    %-5s | %7.4f [%6.4f..%6.4f] %6.1f %.1e | %7.4f %.1e | %7.4f %.1e | %7.4f %.1e" %
                 (kind, Cin, Cout, H, name, md["direct"], min(ms["direct"]), max(ms["direct"]), flops / md["direct"] / 1e9, err["direct"],
                  md["wino_fp32"], err["wino_fp32"], md["wino_bf16x3"], err["wino_bf16x3"], md["miopen"], err["miopen"]))


def wrw(B, iters, rounds, emit):
    from deepinpainting_amd.models import hipconv
    g = torch.Generator(device="cuda").manual_seed(6)
    emit("weight gradient, batch %d, fp32 NCHW operands, dW fp32 in the module's layout; ms = device time per call (HIP events, %d calls per burst, "
         "median of %d alternated rounds); TF = useful flop / time" % (B, iters, rounds))
    emit("err = max |dW - dW64| / max |dW64| against the fp64 weight gradient of the unrounded operands; today = the engine select_wrw answers under conv_math fp32")
    emit("%-22s | %-38s | %-28s | %s" % ("layer", "direct bf16x3 wrw  ms [min..max]  TF   err", "today's engine  ms  err", "today / direct"))
    for kind, Cin, H, Cout in [(k, ci, h, co) for _, ci, h, co in LAYERS for k in ("conv", "convT")]:
        tr = kind == "convT"
        lay = (tr, B, Cin, H, H, Cout, 3, 1, 1, 1)
        label = "%-5s %4d->%-4d @%-3d" % (kind, Cin, Cout, H)
        if not ops.conv3x3_bf16x3_wrw_supported(tr, B, Cin, H, H, Cout):
            emit("%s    | unsupported" % label)
            continue
        x = torch.randn(B, Cin, H, H, device="cuda", generator=g)
        dy = torch.randn(B, Cout, H, H, device="cuda", generator=g)
        w = torch.zeros((Cin, Cout, 3, 3) if tr else (Cout, Cin, 3, 3), device="cuda")
        today = hipconv.select_wrw(*lay)
        if today == "miopen":
            base = lambda: torch.ops.aten.convolution_backward(dy, x, w, None, [1, 1], [1, 1], [1, 1], tr, [0, 0], 1, [False, True, False])[1]
        else:
            base = lambda: hipconv._run_wrw(today, x, dy, w, lay, "fp32")
        ref = torch.ops.aten.convolution_backward(dy.double(), x.double(), w.double(), None, [1, 1], [1, 1], [1, 1], tr, [0, 0], 1, [False, True, False])[1]
        engines = [("direct", lambda: ops.conv3x3_bf16x3_wrw(tr, x, dy, Cout)), ("today", base)]
        err, ms = {}, {k: [] for k, _ in engines}
        for k, fn in engines:
            for _ in range(3):
                d = fn()
            err[k] = float((d.double() - ref).abs().max() / ref.abs().max())
        torch.cuda.synchronize()
        for _ in range(rounds):
            for k, fn in engines:
                ms[k].append(burst_ms(fn, iters))
        md = {k: statistics.median(v) for k, v in ms.items()}
        flops = 2.0 * 9 * Cin * Cout * B * H * H
        emit("%s    | %7.4f [%6.4f..%6.4f] %6.1f %.1e     | %-9s %7.4f %.1e     | %.2fx" %
             (label, md["direct"], min(ms["direct"]), max(ms["direct"]), flops / md["direct"] / 1e9, err["direct"], today, md["today"], err["today"],
              md["today"] / md["direct"]))


# (kind, Kc, Cf, coarse n): Conv2d Cf -> Kc on 2n x 2n, ConvTranspose2d Kc -> Cf on n x n (netP / netD / netF down, netP / netG up)
S2_LAYERS = [("conv", 128, 64, 64), ("conv", 256, 128, 32), ("conv", 512, 256, 16), ("conv", 512, 512, 8), ("conv", 512, 512, 4),
             ("convT", 64, 64, 128), ("convT", 128, 128, 64), ("convT", 256, 256, 32), ("convT", 512, 512, 16), ("convT", 256, 64, 64),
             ("convT", 512, 128, 32), ("convT", 1024, 256, 16), ("convT", 1024, 512, 8), ("convT", 512, 512, 8)]


def s2(B, iters, rounds, emit):
    from deepinpainting_amd.models import hipconv
    g = torch.Generator(device="cuda").manual_seed(7)
    hipconv.set_conv_math(fp32="fp32")
    emit("k4 s2 p1 data passes, batch %d, fp32 NCHW in and out; ms = device time per call (HIP events, %d calls per burst, median of %d alternated "
         "rounds, [min..max]); TF = useful flop / time" % (B, iters, rounds))
    emit("err = max |y - y64| / max |y64| against the fp64 convolution of the unrounded operands; today = the engine select answers under conv_math fp32")
    emit("%-25s %-5s | %-40s | %-44s | %s" % ("layer", "pass", "direct bf16x3  ms [min..max]  TF   err", "today's engine  ms [min..max]  err", "today / direct"))
    for kind, Kc, Cf, n in S2_LAYERS:
        tr = kind == "convT"
        Cin, Cout, H = (Kc, Cf, n) if tr else (Cf, Kc, 2 * n)
        Ho = 2 * n if tr else n
        lay = (tr, B, Cin, H, H, Cout, 4, 2, 1, 1)
        w = torch.randn(Kc, Cf, 4, 4, device="cuda", generator=g) * (1.0 / (4.0 * (Cin ** 0.5)))
        x = torch.randn(B, Cin, H, H, device="cuda", generator=g)
        dy = torch.randn(B, Cout, Ho, Ho, device="cuda", generator=g)
        fop, bop = (ops.CONVT_FWD, ops.CONVT_BWD_DATA) if tr else (ops.CONV_FWD, ops.CONV_BWD_DATA)
        flops = 2.0 * 16 * Kc * Cf * B * n * n
        for name, op, inp in (("fwd", fop, x), ("bwdD", bop, dy)):
            mode = hipconv._s2_mode(op)
            label = "%-5s Kc=%4d Cf=%4d n=%-3d %-5s" % (kind, Kc, Cf, n, name)
            today = hipconv.select(op, B, Cin, H, H, Cout, 4, 2, 1, 1)
            if not ops.conv4x4s2_bf16x3_supported(mode, B, Kc, Cf, n, n):
                emit("%s | unsupported (today: %s)" % (label, today))
                continue
            if today != "miopen":
                base = lambda: hipconv._run_data(today, op, inp, w, lay, "fp32", torch.float32)
            elif name == "fwd":
                base = (lambda: F.conv_transpose2d(x, w, None, 2, 1)) if tr else (lambda: F.conv2d(x, w, None, 2, 1))
            else:
                base = lambda: torch.ops.aten.convolution_backward(dy, x, w, None, [2, 2], [1, 1], [1, 1], tr, [0, 0], 1, [True, False, False])[0]
            f64 = F.conv2d if mode == ops.S2_FINE_TO_COARSE else F.conv_transpose2d
            ref = f64(inp[:2].double(), w.double(), None, 2, 1)
            engines = [("direct", lambda: ops.conv4x4s2_bf16x3(mode, inp, w, B, Kc, Cf, n, n)), ("today", base)]
            err, ms = {}, {k: [] for k, _ in engines}
            for k, fn in engines:
                for _ in range(3):
                    y = fn()
                err[k] = float((y[:2].double() - ref).abs().max() / ref.abs().max())
            torch.cuda.synchronize()
            for _ in range(rounds):
                for k, fn in engines:
                    ms[k].append(burst_ms(fn, iters))
            md = {k: statistics.median(v) for k, v in ms.items()}
            emit("%s | %7.4f [%6.4f..%6.4f] %6.1f %.1e | %-9s %7.4f [%6.4f..%6.4f] %.1e | %.2fx" %
                 (label, md["direct"], min(ms["direct"]), max(ms["direct"]), flops / md["direct"] / 1e9, err["direct"], today, md["today"],
                  min(ms["today"]), max(ms["today"]), err["today"], md["today"] / md["direct"]))


def s2wrw(B, iters, rounds, emit):
    from deepinpainting_amd.models import hipconv
    g = torch.Generator(device="cuda").manual_seed(8)
    hipconv.set_conv_math(fp32="fp32")
    emit("k4 s2 p1 weight gradients, batch %d, fp32 NCHW operands, dW fp32 [Kc][Cf][4][4]; ms = device time per call (HIP events, %d calls per burst, "
         "median of %d alternated rounds, [min..max]); TF = useful flop / time" % (B, iters, rounds))
    emit("err = max |dW - dW64| / max |dW64| against the fp64 weight gradient of the unrounded operands; today = the engine select_wrw answers under conv_math fp32")
    emit("wins = the kernel's slowest round is faster than today's fastest round")
    emit("%-25s | %-40s | %-44s | %s" % ("layer", "direct bf16x3 wrw  ms [min..max]  TF   err", "today's engine  ms [min..max]  err", "today / direct"))
    for kind, Kc, Cf, n in S2_LAYERS:
        tr = kind == "convT"
        Cin, Cout, H = (Kc, Cf, n) if tr else (Cf, Kc, 2 * n)
        Ho = 2 * n if tr else n
        lay = (tr, B, Cin, H, H, Cout, 4, 2, 1, 1)
        label = "%-5s Kc=%4d Cf=%4d n=%-3d" % (kind, Kc, Cf, n)
        today = hipconv.select_wrw(*lay)
        if not ops.conv4x4s2_bf16x3_wrw_supported(B, Kc, Cf, n, n):
            emit("%s | unsupported (today: %s)" % (label, today))
            continue
        x = torch.randn(B, Cin, H, H, device="cuda", generator=g)
        dy = torch.randn(B, Cout, Ho, Ho, device="cuda", generator=g)
        w = torch.zeros(Kc, Cf, 4, 4, device="cuda")
        fine, coarse = (dy, x) if tr else (x, dy)
        if today == "miopen":
            base = lambda: torch.ops.aten.convolution_backward(dy, x, w, None, [2, 2], [1, 1], [1, 1], tr, [0, 0], 1, [False, True, False])[1]
        else:
            base = lambda: hipconv._run_wrw(today, x, dy, w, lay, "fp32")
        ref = torch.ops.aten.convolution_backward(dy.double(), x.double(), w.double(), None, [2, 2], [1, 1], [1, 1], tr, [0, 0], 1, [False, True, False])[1]
        engines = [("direct", lambda: ops.conv4x4s2_bf16x3_wrw(fine, coarse, B, Kc, Cf, n, n)), ("today", base)]
        err, ms = {}, {k: [] for k, _ in engines}
        for k, fn in engines:
            for _ in range(3):
                d = fn()
            err[k] = float((d.double() - ref).abs().max() / ref.abs().max())
        torch.cuda.synchronize()
        for _ in range(rounds):
            for k, fn in engines:
                ms[k].append(burst_ms(fn, iters))
        md = {k: statistics.median(v) for k, v in ms.items()}
        flops = 2.0 * 16 * Kc * Cf * B * n * n
        emit("%s | %7.4f [%6.4f..%6.4f] %6.1f %.1e | %-9s %7.4f [%6.4f..%6.4f] %.1e | %.2fx %s" %
             (label, md["direct"], min(ms["direct"]), max(ms["direct"]), flops / md["direct"] / 1e9, err["direct"], today, md["today"],
              min(ms["today"]), max(ms["today"]), err["today"], md["today"] / md["direct"], "wins" if max(ms["direct"]) < min(ms["today"]) else "loses"))


# (channels, H = W of the module's input): one per U-Net level that "wino_dil" has
DIL_LAYERS = [(64, 256), (128, 128), (256, 64), (512, 32)]


def dil(B, iters, rounds, emit):
    from deepinpainting_amd.models import hipconv
    g = torch.Generator(device="cuda").manual_seed(9)
    hipconv.set_conv_math(fp32="fp32")
    hipconv.set_direct_dilated(False)
    emit("k4 s2 p3 d2 data passes, batch %d, fp32 NCHW in and out; ms = device time per call (HIP events, %d calls per burst, median of %d alternated "
         "rounds, [min..max]); TF = useful flop / time" % (B, iters, rounds))
    emit("err = max |y - y64| / max |y64| against the fp64 convolution of the unrounded operands; today = the engine select answers with the switch off")
    emit("wins = the kernel's slowest round is faster than today's fastest round; loses = the reverse; ties = the ranges overlap")
    emit("%-22s %-5s | %-40s | %-44s | %s" % ("layer", "pass", "direct bf16x3  ms [min..max]  TF   err", "today's engine  ms [min..max]  err", "today / direct"))
    for C, H in DIL_LAYERS:
        n = H // 2
        lay = (False, B, C, H, H, C, 4, 2, 3, 2)
        w = torch.randn(C, C, 4, 4, device="cuda", generator=g) * (1.0 / (4.0 * (C ** 0.5)))
        x = torch.randn(B, C, H, H, device="cuda", generator=g)
        dy = torch.randn(B, C, n, n, device="cuda", generator=g)
        flops = 2.0 * 16 * C * C * B * n * n
        for name, op, inp in (("fwd", ops.CONV_FWD, x), ("bwdD", ops.CONV_BWD_DATA, dy)):
            mode = hipconv._dil_mode(op)
            label = "conv %4d->%-4d @%-3d   %-5s" % (C, C, H, name)
            today = hipconv.select(op, B, C, H, H, C, 4, 2, 3, 2)
            if not ops.conv4x4s2_bf16x3_supported(mode, B, C, C, n, n):
                emit("%s | unsupported (today: %s)" % (label, today))
                continue
            if today != "miopen":
                base = lambda: hipconv._run_data(today, op, inp, w, lay, "fp32", torch.float32)
            elif name == "fwd":
                base = lambda: F.conv2d(x, w, None, 2, 3, 2)
            else:
                base = lambda: torch.ops.aten.convolution_backward(dy, x, w, None, [2, 2], [3, 3], [2, 2], False, [0, 0], 1, [True, False, False])[0]
            if name == "fwd":
                ref = F.conv2d(inp[:2].double(), w.double(), None, 2, 3, 2)
            else:
                ref = F.conv_transpose2d(inp[:2].double(), w.double(), None, 2, 3, 1, 1, 2)
            engines = [("direct", lambda: ops.conv4x4s2_bf16x3(mode, inp, w, B, C, C, n, n)), ("today", base)]
            err, ms = {}, {k: [] for k, _ in engines}
            for k, fn in engines:
                for _ in range(3):
                    y = fn()
                err[k] = float((y[:2].double() - ref).abs().max() / ref.abs().max())
            torch.cuda.synchronize()
            for _ in range(rounds):
                for k, fn in engines:
                    ms[k].append(burst_ms(fn, iters))
            md = {k: statistics.median(v) for k, v in ms.items()}
            verdict = "wins" if max(ms["direct"]) < min(ms["today"]) else "loses" if min(ms["direct"]) > max(ms["today"]) else "ties"
            emit("%s | %7.4f [%6.4f..%6.4f] %6.1f %.1e | %-9s %7.4f [%6.4f..%6.4f] %.1e | %.2fx %s" %
                 (label, md["direct"], min(ms["direct"]), max(ms["direct"]), flops / md["direct"] / 1e9, err["direct"], today, md["today"],
                  min(ms["today"]), max(ms["today"]), err["today"], md["today"] / md["direct"], verdict))


def dilwrw(B, iters, rounds, emit):
    from deepinpainting_amd.models import hipconv
    g = torch.Generator(device="cuda").manual_seed(10)
    hipconv.set_conv_math(fp32="fp32")
    hipconv.set_direct_dilated_dw(False)
    emit("k4 s2 p3 d2 weight gradient, batch %d, fp32 NCHW operands, dW fp32; ms = device time per call (HIP events, %d calls per burst, median of %d "
         "alternated rounds, [min..max]); TF = useful flop / time" % (B, iters, rounds))
    emit("err = max |dW - dW64| / max |dW64| against the fp64 weight gradient of the unrounded operands; today = the engine select_wrw answers with the switch off")
    emit("wins = the kernel's slowest round is faster than today's fastest round; loses = the reverse; ties = the ranges overlap")
    emit("%-22s %-5s | %-40s | %-44s | %s" % ("layer", "pass", "direct bf16x3  ms [min..max]  TF   err", "today's engine  ms [min..max]  err", "today / direct"))
    for C, H in DIL_LAYERS:
        n = H // 2
        lay = (False, B, C, H, H, C, 4, 2, 3, 2)
        w = torch.zeros(C, C, 4, 4, device="cuda")
        x = torch.randn(B, C, H, H, device="cuda", generator=g)
        dy = torch.randn(B, C, n, n, device="cuda", generator=g)
        flops = 2.0 * 16 * C * C * B * n * n
        label = "conv %4d->%-4d @%-3d   %-5s" % (C, C, H, "wrw")
        today = hipconv.select_wrw(False, B, C, H, H, C, 4, 2, 3, 2)
        if not ops.conv4x4s2_bf16x3_dil_wrw_supported(B, C, C, n, n):
            emit("%s | unsupported (today: %s)" % (label, today))
            continue
        if today != "miopen":
            base = lambda: hipconv._run_wrw(today, x, dy, w, lay, "fp32")
        else:
            base = lambda: torch.ops.aten.convolution_backward(dy, x, w, None, [2, 2], [3, 3], [2, 2], False, [0, 0], 1, [False, True, False])[1]
        ref = torch.ops.aten.convolution_backward(dy.double(), x.double(), w.double(), None, [2, 2], [3, 3], [2, 2], False, [0, 0], 1, [False, True, False])[1]
        engines = [("direct", lambda: ops.conv4x4s2_bf16x3_dil_wrw(x, dy, B, C, C, n, n)), ("today", base)]
        err, ms = {}, {k: [] for k, _ in engines}
        for k, fn in engines:
            for _ in range(3):
                y = fn()
            err[k] = float((y.double() - ref).abs().max() / ref.abs().max())
        del ref
        torch.cuda.synchronize()
        for _ in range(rounds):
            for k, fn in engines:
                ms[k].append(burst_ms(fn, iters))
        md = {k: statistics.median(v) for k, v in ms.items()}
        verdict = "wins" if max(ms["direct"]) < min(ms["today"]) else "loses" if min(ms["direct"]) > max(ms["today"]) else "ties"
        emit("%s | %7.4f [%6.4f..%6.4f] %6.1f %.1e | %-9s %7.4f [%6.4f..%6.4f] %.1e | %.2fx %s" %
             (label, md["direct"], min(ms["direct"]), max(ms["direct"]), flops / md["direct"] / 1e9, err["direct"], today, md["today"],
              min(ms["today"]), max(ms["today"]), err["today"], md["today"] / md["direct"], verdict))


def steps(B, ksteps, rounds, emit, maths=None, dilated=(False, True), dilated_dw=(False,)):
    from deepinpainting_amd.models import hipconv
    from deepinpainting_amd.models.models import create_model
    from deepinpainting_amd.options import Option
    device = torch.device("cuda", 0)
    opt = Option(gpu_ids=[0], batchSize=B, use_dropout=True, quiet=True, allow_random_vgg=True, batch_vgg=False, batch_disc=True, amp_bf16=False,
                 conv_math="fp32", checkpoints_dir=os.path.join("/tmp", "ipsr_bench_direct_bf16x3"))
    torch.manual_seed(1234)
    model = bench.quiet(create_model, opt)
    img, mask, ref = bench.synthetic_batch(device, B, 1234)
    maths = tuple(maths) if maths else ("fp32", "direct_bf16x3", "direct_bf16x3_dw", "direct_bf16x3_s2", "direct_bf16x3_s2_dw", "bf16x3")
    variants = [(m, d, dw) for m in maths for d in dilated for dw in dilated_dw]
    rate = {v: [] for v in variants}

    def use(v):
        hipconv.set_conv_math(fp32=v[0])
        hipconv.set_direct_dilated(v[1])
        hipconv.set_direct_dilated_dw(v[2])
    try:
        for v in variants:                                     # every variant's shapes warmed before any is timed
            use(v)
            for _ in range(3):
                bench.train_step(model, img, mask, ref)
        torch.cuda.synchronize()
        for _ in range(rounds):
            for v in variants:
                use(v)
                bench.train_step(model, img, mask, ref)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(ksteps):
                    bench.train_step(model, img, mask, ref)
                torch.cuda.synchronize()
                rate[v].append(B * ksteps / (time.perf_counter() - t0))
    finally:
        use(("fp32", False, False))
    emit("whole fp32 training step (bench.py's model and step, batch %d, eager, one process): images/s over %d steps, %d alternated rounds" % (B, ksteps, rounds))
    emit("  one column per setting of hipconv.set_direct_dilated%s: median (rounds)" % (" / set_direct_dilated_dw" if len(dilated_dw) > 1 else ""))
    onoff = lambda b: "on" if b else "off"
    for m in maths:
        emit("  conv_math %-19s %s" % (m, "   ".join("dilated %-3s%s median %7.1f (%s)" % (
            onoff(d), " dw %-3s" % onoff(dw) if len(dilated_dw) > 1 else "", statistics.median(rate[(m, d, dw)]), " ".join("%.1f" % r for r in rate[(m, d, dw)]))
            for d in dilated for dw in dilated_dw)))
    losses = {k: float(v) for k, v in model.get_current_errors().items()}
    emit("  losses after the last step finite: %s" % all(v == v and abs(v) != float("inf") for v in losses.values()))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--what", nargs="+", default=["layers", "steps"], choices=("layers", "wrw", "s2", "s2wrw", "dil", "dilwrw", "steps"))
    ap.add_argument("--maths", nargs="+", default=None, help="the arithmetics of the step table (default: all six)")
    ap.add_argument("--dilated", choices=("both", "off", "on"), default="both", help="the step table's columns: hipconv.set_direct_dilated off, on or both")
    ap.add_argument("--dilated-dw", choices=("off", "both", "on"), default="off", help="the step table's columns: hipconv.set_direct_dilated_dw off, on or both")
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("needs the GPU: nothing is measured without one")
    fh = open(a.out, "w") if a.out else None

    def emit(line):
        print(line, flush=True)
        if fh:
            fh.write(line + "\n")
            fh.flush()
    emit("# tools/bench_direct_bf16x3.py on %s" % torch.cuda.get_device_name(0))
    if "layers" in a.what:
        layers(a.batch, a.iters, a.rounds, emit)
    if "wrw" in a.what:
        wrw(a.batch, a.iters, a.rounds, emit)
    if "s2" in a.what:
        s2(a.batch, a.iters, a.rounds, emit)
    if "s2wrw" in a.what:
        s2wrw(a.batch, a.iters, a.rounds, emit)
    if "dil" in a.what:
        dil(a.batch, a.iters, a.rounds, emit)
    if "dilwrw" in a.what:
        dilwrw(a.batch, a.iters, a.rounds, emit)
    if "steps" in a.what:
        cols = {"both": (False, True), "off": (False,), "on": (True,)}
        steps(a.batch, a.steps, a.rounds, emit, a.maths, cols[a.dilated], cols[a.dilated_dw])


if __name__ == "__main__":
    main()
