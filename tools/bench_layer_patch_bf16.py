#!/usr/bin/env python3
"""Time the IPSR layer with 3x3 patches, fp32 correlation against bf16 correlation (the 1x1 correlation R of the shifted-sum form
on the bf16 matrix cores), in one process.

The two precisions alternate call by call after a warm-up, each forward and backward timed with HIP events; the arg-max
agreement of the bf16 forward with the fp32 one is printed per shape.

    python3 tools/bench_layer_patch_bf16.py [--iters 20] [--out profiles/r05_layer_p3_bf16.txt]
"""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from deepinpainting_amd import ops  # noqa: E402

# (B, C, h, mask image size, hole lo, hi): config 4's [4,512,64,64] and config 2's [8,512,32,32] feature, p = 3
SHAPES = [(4, 512, 64, 512, 128, 384), (8, 512, 32, 256, 64, 192)]


def median(v):
    v = sorted(v)
    return v[len(v) // 2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--patch", type=int, default=3)
    ap.add_argument("--shape", type=int, default=-1, help="index into SHAPES (default: all)")
    ap.add_argument("--out", default=None, help="also write the report to this file")
    a = ap.parse_args()
    P = a.patch
    lines = ["IPSR layer, shift_sz=%d, fp32 vs bf16 correlation on %s (median of %d alternating calls after %d warm-up)"
             % (P, torch.cuda.get_device_name(0), a.iters, a.warmup)]
    for si, (B, C, h, size, lo, hi) in enumerate(SHAPES):
        if a.shape >= 0 and si != a.shape:
            continue
        g = torch.Generator(device="cuda").manual_seed(1234)
        x = torch.randn(B, C, h, h, device="cuda", generator=g).abs()
        ref = torch.relu(torch.randn(B, C, h, h, device="cuda", generator=g))
        grad = torch.randn(B, C, h, h, device="cuda", generator=g)
        m = torch.zeros(size, size, dtype=torch.uint8, device="cuda")
        m[lo:hi, lo:hi] = 1
        feat = ops.feat_mask(m, 3, 5 / 16.0)
        _, mpi, cnt = ops.index_prep(feat, P, 1, 1)
        M = int(cnt.item())
        mpi = mpi[:M].contiguous()
        t = {("fp32", "fwd"): [], ("fp32", "bwd"): [], ("bf16", "fwd"): [], ("bf16", "bwd"): []}
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
        res = {}
        for it in range(a.warmup + a.iters):
            for corr in ("fp32", "bf16"):
                ev[0].record()
                f = ops.forward(x, ref, mpi, patch=P, corr=corr)
                ev[1].record()
                ops.backward(grad, f.bwd_index, 1.0, M, patch=P)
                ev[2].record()
                torch.cuda.synchronize()
                if it >= a.warmup:
                    t[(corr, "fwd")].append(ev[0].elapsed_time(ev[1]))
                    t[(corr, "bwd")].append(ev[1].elapsed_time(ev[2]))
                res[corr] = f.ind
        agree = float((res["fp32"] == res["bf16"]).double().mean())
        Np = (h - P + 1) ** 2
        K = C * P * P
        fl = 2.0 * B * (h * h) ** 2 * C
        f32, f16 = median(t[("fp32", "fwd")]), median(t[("bf16", "fwd")])
        lines.append("[%d,%d,%d,%d] p=%d N'=%d K=%d M=%d: forward fp32 %.3f ms  bf16 %.3f ms (x%.2f) | backward fp32 %.3f ms  bf16 %.3f ms | "
                     "arg-max agreement %.4f | R = x^T ref %.1f GFLOP"
                     % (B, C, h, h, P, Np, K, M, f32, f16, f32 / f16, median(t[("fp32", "bwd")]), median(t[("bf16", "bwd")]), agree, fl / 1e9))
        del x, ref, grad, f, res
        torch.cuda.empty_cache()
    text = "\n".join(lines)
    print(text)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
