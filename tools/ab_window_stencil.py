#!/usr/bin/env python3
"""A/B of the LDS-tiled window stencil of csrc/window_stencil.hip against the streaming kernel of csrc/corr_argmax.hip inside one build
(ipsr_debug_set_option key 8: 1 = streaming everywhere, 2 = LDS-tiled wherever the envelope allows): the whole layer forward with
shift_sz > 1, fp32 and bf16 correlation.  The forms alternate, `--rounds` rounds of a median of `--iters` calls each; reported: the
median over the rounds of each form, the spread (max - min) of the streaming rounds, the difference, what the size rule (key 8 = 0)
gives, and the tiled kernel's plan.  A shape class belongs in the rule only where the tiled form is faster by more than twice the
spread.

    python tools/ab_window_stencil.py [--rounds 5] [--iters 20] > window_stencil_lds.txt

`--kernels N` instead runs every shape N times per form without timing, for a kernel trace of the two stencil kernels themselves
(`--shape i` restricts either mode to one shape, so that a trace's per-kernel totals belong to it).
"""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from deepinpainting_amd import _lib, ops  # noqa: E402

OPTION = 8
# (B, C, h, w, p): BASELINE config 4, config 2's feature, their batch-of-one forms, config 4 with 2x2 patches
SHAPES = [(4, 512, 64, 64, 3), (8, 512, 32, 32, 3), (1, 512, 64, 64, 3), (1, 512, 32, 32, 3), (4, 512, 64, 64, 2)]


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


def inputs(B, C, h, w, p):
    g = torch.Generator(device="cuda").manual_seed(1234)
    x = torch.randn(B, C, h, w, device="cuda", generator=g).abs()
    ref = torch.relu(torch.randn(B, C, h, w, device="cuda", generator=g))
    feat = torch.zeros(h, w, dtype=torch.uint8, device="cuda")
    feat[h // 4:3 * h // 4, w // 4:3 * w // 4] = 1                      # the centre hole of the BASELINE configs
    _, mpi, cnt = ops.index_prep(feat, p, 1, 1)
    return x, ref, mpi[:int(cnt.item())].contiguous()


def set_option(L, v):
    _lib.check(L.ipsr_debug_set_option(OPTION, v), "ipsr_debug_set_option")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--shape", type=int, default=-1, help="index into SHAPES (default: all)")
    ap.add_argument("--kernels", type=int, default=0, help="run each form this many times untimed (for a kernel trace) and exit")
    a = ap.parse_args()
    L = _lib.lib()
    shapes = [s for i, s in enumerate(SHAPES) if a.shape < 0 or i == a.shape]
    if a.kernels:
        for shape in shapes:
            x, ref, mpi = inputs(*shape)
            for v in (1, 2):
                set_option(L, v)
                for _ in range(a.kernels):
                    ops.forward(x, ref, mpi, patch=shape[4])
                torch.cuda.synchronize()
            set_option(L, 0)
        return
    print("# layer forward, ms: median of %d alternating rounds (each the median of %d calls) on %s" % (a.rounds, a.iters, torch.cuda.get_device_name(0)))
    print("%-22s %-5s %10s %9s %9s %8s %9s %8s  %s" % ("[B,C,h,w] p", "corr", "streaming", "spread", "tiled", "diff", "rule(0)", "rule is", "tiled plan"))
    for shape in shapes:
        B, C, h, w, p = shape
        x, ref, mpi = inputs(*shape)
        for corr in ("fp32", "bf16"):
            fn = lambda: ops.forward(x, ref, mpi, patch=p, corr=corr)
            t = {1: [], 2: [], 0: []}
            ind = {}
            for _ in range(a.rounds):
                for v in (1, 2, 0):
                    set_option(L, v)
                    t[v].append(timed(fn, a.iters))
                    ind[v] = fn().ind
            set_option(L, 2)
            plan = ops.window_corr_plan(B, h, w, p)
            set_option(L, 0)
            rule = "tiled" if ops.window_corr_plan(B, h, w, p)["variant"] else "streaming"
            assert torch.equal(ind[1], ind[2]) and torch.equal(ind[1], ind[0]), "the two kernels disagree"
            s, tl, r0 = (statistics.median(t[v]) for v in (1, 2, 0))
            print("%-22s %-5s %10.4f %9.4f %9.4f %+7.1f%% %9.4f %8s  %d wgs, split %d, %d B LDS" % (
                "[%d,%d,%d,%d] p=%d" % shape, corr, s, max(t[1]) - min(t[1]), tl, 100.0 * (tl - s) / s, r0, rule,
                plan["workgroups"], plan["split"], plan["lds_bytes"]), flush=True)
        del x, ref, mpi
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
