#!/usr/bin/env python3
"""A/B of the one-launch Winograd kernel of csrc/wino_fused.hip against the three launches of csrc/winograd.hip inside one build
(ipsr_debug_set_option key 7: 1 = three launches, 2 = fused wherever the envelope allows) on the 3x3 data passes that produce at
most 64 channels: whole-convolution time, batch 8, fp32.  The two forms alternate, `--rounds` rounds of a median of `--iters` calls
each; reported: the median over the rounds of each form, the spread (max - min) of the three-launch rounds, the difference, and
whether the size rule (key 7 = 0) sends the shape to the fused kernel.  A shape belongs in the rule only where the fused form is
faster by more than the spread.

    python tools/ab_wino_fused.py [--rounds 5] [--iters 20] > wino_fused_layers.txt
"""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench  # noqa: F401  (private MIOpen db copy)
from deepinpainting_amd import _lib, ops

# (op, Cin, H, Cout, epilogue, filter cache valid)   — Cin / Cout of the MODULE; the step's launches first
SHAPES = [("CONV_FWD", 64, 256, 64, "relu_pool", True),        # VGG conv1_2 (frozen weights: cached filter), three times per step
          ("CONV_FWD", 64, 256, 64, None, False),
          ("CONVT_FWD", 256, 128, 64, None, False),            # netG upconv_3, outermost but one
          ("CONV_BWD_DATA", 64, 128, 128, None, False),        # input gradient of netG downconv_3 64 -> 128: produces 64
          ("CONV_FWD", 64, 128, 64, None, False),              # 8192 tiles: the rule's edge
          ("CONV_FWD", 128, 128, 64, None, False),
          ("CONV_FWD", 64, 64, 64, None, False),               # 2048 tiles: 64 workgroups
          ("CONVT_FWD", 512, 64, 64, None, False),
          ("CONV_FWD", 64, 256, 32, None, False),
          ("CONV_FWD", 16, 256, 64, None, False)]


def timed(fn, n):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(n):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        ts.append(a.elapsed_time(b))
    return statistics.median(ts)


def cases(B):
    r = lambda *s: torch.randn(*s, device="cuda")
    for opname, Cin, H, Cout, epi, cached in SHAPES:
        op = getattr(ops, opname)
        fwd = opname.endswith("FWD")
        x = r(B, Cin if fwd else Cout, H, H)
        w = r(*((Cin, Cout, 3, 3) if opname.startswith("CONVT") else (Cout, Cin, 3, 3))) * 0.05
        bias = r(Cout) if epi else None
        sh = (B, Cin, H, H)
        cache = ops.winograd_filter_cache(op, Cin, Cout, x.device) if cached else None
        if cached:
            ops.conv3x3_winograd(op, x, w, sh, Cout, bias=bias, epilogue=epi, filter_cache=cache, filter_cache_valid=False)
        name = "%-13s %3d->%-3d @%3d %-9s %s" % (opname, Cin, Cout, H, epi or "-", "cached" if cached else "")
        tiles = B * ((H + 3) // 4) ** 2
        yield name, tiles, lambda op=op, x=x, w=w, sh=sh, Cout=Cout, bias=bias, epi=epi, cache=cache, cached=cached: ops.conv3x3_winograd(
            op, x, w, sh, Cout, bias=bias, epilogue=epi, filter_cache=cache, filter_cache_valid=cached)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=20)
    a = ap.parse_args()
    L = _lib.lib()
    print("# whole convolution, ms: median of %d alternating rounds (each the median of %d calls); batch %d, fp32" % (a.rounds, a.iters, a.batch))
    print("%-48s %7s %9s %9s %9s %8s %9s" % ("op  shape", "tiles", "three", "spread", "fused", "diff", "rule(0)"))
    for name, tiles, fn in cases(a.batch):
        t = {1: [], 2: [], 0: []}
        for _ in range(a.rounds):
            for v in (1, 2, 0):
                _lib.check(L.ipsr_debug_set_option(7, v), "ipsr_debug_set_option")
                t[v].append(timed(fn, a.iters))
        L.ipsr_debug_set_option(7, 0)
        three, fused, rule = (statistics.median(t[v]) for v in (1, 2, 0))
        print("%-48s %7d %9.4f %9.4f %9.4f %+7.1f%% %9.4f" % (name, tiles, three, max(t[1]) - min(t[1]), fused, 100.0 * (fused - three) / three, rule),
              flush=True)


if __name__ == "__main__":
    main()
