#!/usr/bin/env python3
"""A/B of the paired transform launches of csrc/winograd.hip (ipsr_debug_set_option key 2: 0 = one launch per pair, 1 = two launches)
on the 3x3 shapes of profiles/r04_persistent_gemm_experiment.txt and the step's larger 4x4 layers: whole-convolution time of every
pass, batch 8, fp32.  The two variants alternate, `--rounds` rounds of a median of `--iters` calls each; reported: the median over
the rounds, the spread (max - min) of the two-launch rounds, and the difference.

    python tools/ab_wino_pair.py [--rounds 5] [--iters 20] > wino_pair_layers.txt
"""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench  # noqa: F401  (private MIOpen db copy)
from deepinpainting_amd import _lib, ops

K3 = [(512, 16, 512), (512, 32, 512), (256, 64, 256), (128, 128, 128), (1024, 32, 256), (256, 32, 512), (64, 256, 64)]      # Cin, H, Cout
S2 = [(512, 256, 16), (128, 64, 64), (512, 512, 8), (256, 128, 32)]                                                     # Kc, Cf, nh
DIL = [(128, 128, 128), (256, 64, 256), (512, 32, 512)]                                                                 # Cin, H, Cout


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
    for Cin, H, Cout in K3:
        x, dy, w = r(B, Cin, H, H), r(B, Cout, H, H), r(Cout, Cin, 3, 3) * 0.05
        sh = (B, Cin, H, H)
        yield "k3 fwd  %d,%d,%d" % (Cin, H, Cout), lambda x=x, w=w, sh=sh, Cout=Cout: ops.conv3x3_winograd(ops.CONV_FWD, x, w, sh, Cout)
        yield "k3 bwd  %d,%d,%d" % (Cin, H, Cout), lambda dy=dy, w=w, sh=sh, Cout=Cout: ops.conv3x3_winograd(ops.CONV_BWD_DATA, dy, w, sh, Cout)
        yield "k3 wrw  %d,%d,%d" % (Cin, H, Cout), lambda x=x, dy=dy, Cout=Cout: ops.conv3x3_winograd_wrw(False, x, dy, Cout)
    for Kc, Cf, nh in S2:
        fine, coarse, w = r(B, Cf, 2 * nh, 2 * nh), r(B, Kc, nh, nh), r(Kc, Cf, 4, 4) * 0.05
        for mode, (a, b) in enumerate(((fine, w), (coarse, w), (fine, coarse))):
            yield "s2 m%d   %d,%d,%d" % (mode, Kc, Cf, nh), lambda mode=mode, a=a, b=b, Kc=Kc, Cf=Cf, nh=nh: ops.conv4x4s2_winograd(mode, a, b, B, Kc, Cf, nh, nh)
    for Cin, H, Cout in DIL:
        x, dy, w = r(B, Cin, H, H), r(B, Cout, H // 2, H // 2), r(Cout, Cin, 4, 4) * 0.05
        for mode, (a, b) in enumerate(((x, w), (dy, w), (x, dy))):
            yield "dil m%d  %d,%d,%d" % (mode, Cin, H, Cout), lambda mode=mode, a=a, b=b, Cin=Cin, H=H, Cout=Cout: ops.conv4x4_dilated_winograd(mode, a, b, (B, Cin, H, H), Cout)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=20)
    a = ap.parse_args()
    L = _lib.lib()
    print("# whole convolution, ms: median of %d alternating rounds (each the median of %d calls); batch %d, fp32" % (a.rounds, a.iters, a.batch))
    print("%-28s %10s %10s %10s %9s" % ("pass  shape", "two", "spread", "paired", "diff"))
    for name, fn in cases(a.batch):
        t = {0: [], 1: []}
        for _ in range(a.rounds):
            for two in (1, 0):
                _lib.check(L.ipsr_debug_set_option(2, two), "ipsr_debug_set_option")
                t[two].append(timed(fn, a.iters))
        L.ipsr_debug_set_option(2, 0)
        two, pair = statistics.median(t[1]), statistics.median(t[0])
        print("%-28s %10.4f %10.4f %10.4f %+8.1f%%" % (name, two, max(t[1]) - min(t[1]), pair, 100.0 * (pair - two) / two), flush=True)


if __name__ == "__main__":
    main()
