#!/usr/bin/env python3
"""A/B of the small-map convolution engine (csrc/smallmap.hip, ipsr_conv_smallmap) on the shapes the fp32 training step gives it
(BASELINE config 2: batch 8, 256x256): device time per call by HIP events.

The shapes are collected the way tools/engine_map.py collects them: one step of the model with models/hipconv._check_hook installed,
every call that lands on the "smallmap" engine — the 2x2 and 1x1 levels for the forward / input-gradient passes (ops SM_FWD, SM_DATA),
the four innermost levels for the weight gradients (SM_WRW).

Two comparisons, the variants of a row alternating within every round:
  * inside this build: `new`, the default, against `staged` (`ipsr_debug_set_option(3, 1)`: pre-pass launches + workspace images
    in every call), `gathered` (option 3 = 2: operands gathered in the main kernels in every call) and, for the data pass,
    `c2i_loop` (option 4 = 1: the default with the looping col2im kernel);
  * with `--parent-lib PATH`: a libipsr_hip.so built from the parent commit in another directory, loaded next to this one and called
    through the same C entry point on the same tensors.
A time is the median over `--rounds` rounds of the median of `--iters` measurements, each one HIP-event pair around `--inner` calls,
divided by `--inner`.  The spread is max - min over the rounds.  A row counts as gained when the new median is below the parent's
minimum by more than the parent's spread, as slower when it is above the parent's maximum by more than that spread, else level.

    python tools/ab_smallmap.py --parent-lib _ab/parent/deepinpainting_amd/libipsr_hip.so > smallmap_stream_layers.txt

`--tiled`: the table of the tiled regime instead (profiles/smallmap_tiled_layers.txt) — the 512 / 1024-channel layers of netG, netP and
netF on 2x2 .. 16x16 maps that MIOpen has without a reach (TILED_LAYERS), every pass: MIOpen through torch (its layout transposes and
fills included) against the streaming kernels (`tiled=False`) and the tiled regime (`tiled=True`; the weight gradient has none), the
three alternating within every round.  A pass moves when the median of the engine's best form is below MIOpen's minimum by more than
MIOpen's spread.

    python tools/ab_smallmap.py --tiled > smallmap_tiled_layers.txt
"""
import argparse
import collections
import contextlib
import ctypes
import io
import os
import statistics
import sys
import tempfile

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench  # noqa: F401,E402  (private MIOpen find-db copy, as the benchmark runs)
from deepinpainting_amd import _lib, ops  # noqa: E402
from deepinpainting_amd.models import hipconv  # noqa: E402

OP_NAME = {ops.SM_DATA: "data", ops.SM_WRW: "wrw", ops.SM_FWD: "fwd"}


def step_shapes(batch):
    """{(op, geometry): calls per step} of the "smallmap" engine in one training step."""
    from deepinpainting_amd.models.models import create_model
    from deepinpainting_amd.options import Option
    opt = Option(gpu_ids=[0], batchSize=batch, use_dropout=True, quiet=True, allow_random_vgg=True, checkpoints_dir=tempfile.mkdtemp())
    torch.manual_seed(5)
    with contextlib.redirect_stdout(io.StringIO()):
        m = create_model(opt)
    g = torch.Generator(device="cuda").manual_seed(21)
    img = torch.rand(batch, 3, 256, 256, device="cuda", generator=g) * 2 - 1
    ref = torch.rand(batch, 3, 256, 256, device="cuda", generator=g) * 2 - 1
    mask = torch.zeros(1, 1, 256, 256, dtype=torch.bool, device="cuda")
    mask[:, :, 64:192, 64:192] = 1
    calls = collections.Counter()

    def hook(kind, engine, geom, operands, result):
        if engine != "smallmap":
            return
        transposed, k, stride, pad, dil, Cout = geom
        x = operands[0] if kind == "forward" else operands[1]
        B, Cin, H, W = x.shape
        lay = (transposed, B, Cin, H, W, Cout, k, stride, pad, dil)
        if kind == "weight_grad":
            op = ops.SM_WRW
        elif kind == "forward":
            op = hipconv._smallmap_op(ops.CONVT_FWD if transposed else ops.CONV_FWD)
        else:
            op = hipconv._smallmap_op(ops.CONVT_BWD_DATA if transposed else ops.CONV_BWD_DATA)
        calls[(op, tuple(hipconv._smallmap_geometry(lay)))] += 1

    for step in range(2):
        hipconv._check_hook = hook if step == 1 else None
        try:
            m.set_input(img, mask, ref)
            m.set_ref_latent()
            m.set_gt_latent()
            m.optimize_parameters()
        finally:
            hipconv._check_hook = None
    torch.cuda.synchronize()
    del m
    torch.cuda.empty_cache()
    return calls


def load_parent(path):
    L = ctypes.CDLL(os.path.abspath(path))
    for name in ("ipsr_conv_smallmap", "ipsr_conv_smallmap_workspace_bytes"):
        res, args = _lib.SIGNATURES[name]
        getattr(L, name).restype, getattr(L, name).argtypes = res, args
    return L


def timed(fn, iters, inner):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(inner):
            fn()
        b.record()
        torch.cuda.synchronize()
        ts.append(a.elapsed_time(b) * 1e3 / inner)
    return statistics.median(ts)


# (net, module, Cin, Cout, (k, stride, pad, dil), input extent, batch)
TILED_LAYERS = (
    ("netP/F", "conv", 512, 512, (4, 2, 1, 1), 16, 8), ("netP/F", "conv", 512, 512, (4, 2, 1, 1), 8, 8),
    ("netF", "conv", 512, 512, (4, 2, 1, 1), 16, 16), ("netF", "conv", 512, 512, (4, 2, 1, 1), 8, 16),
    ("netP", "convT", 1024, 512, (4, 2, 1, 1), 4, 8), ("netP", "convT", 1024, 512, (4, 2, 1, 1), 8, 8),
    ("netG", "conv", 512, 512, (4, 2, 3, 2), 16, 8), ("netG", "conv", 512, 512, (4, 2, 3, 2), 8, 8),
    ("netG", "conv", 512, 512, (3, 1, 1, 1), 8, 8), ("netG", "conv", 512, 512, (3, 1, 1, 1), 4, 8), ("netG", "conv", 512, 512, (3, 1, 1, 1), 2, 8),
    ("netG", "convT", 1024, 512, (3, 1, 1, 1), 2, 8), ("netG", "convT", 1024, 512, (3, 1, 1, 1), 4, 8), ("netG", "convT", 1024, 512, (3, 1, 1, 1), 8, 8),
    ("netG", "convT", 512, 512, (4, 2, 1, 1), 4, 8), ("netG", "convT", 512, 512, (4, 2, 1, 1), 8, 8),
)


def tiled_table(a):
    import torch.nn.functional as F
    print("# the small-map engine against MIOpen through torch, device us per call: median of %d alternating rounds (each the median of %d event "
          "pairs around %d calls), fp32" % (a.rounds, a.iters, a.inner))
    print("# pass: fwd / dx / dw of the module; base = the dispatcher's answer without a reach; P = positions; verdict: the engine's better form "
          "against MIOpen (moves: its median < MIOpen's minimum - MIOpen's spread)")
    print("%-7s %-28s %-4s %-9s %5s %9s %9s %9s %9s %9s %9s %9s  %s" % ("net", "layer", "pass", "base", "P", "miopen", "m.min", "m.spread", "stream",
                                                                        "s.spread", "tiled", "t.spread", "verdict"))
    tot = collections.Counter()
    for net, kind, Cin, Cout, geom, H, B in TILED_LAYERS:
        tr = kind == "convT"
        k, stride, pad, dil = geom
        lay = (tr, B, Cin, H, H, Cout) + geom
        g = hipconv._smallmap_geometry(lay)
        x = torch.randn(B, Cin, H, H, device="cuda")
        w = torch.randn((Cin, Cout, k, k) if tr else (Cout, Cin, k, k), device="cuda") * 0.05
        y = hipconv._miopen_forward(x, w, tr, stride, pad, dil)
        dy = torch.randn_like(y)
        for name in ("fwd", "dx", "dw"):
            if name == "dw":
                base = hipconv.select_wrw(*lay)
                sm_op, ops_ab = ops.SM_WRW, ((x, dy) if tr else (dy, x))
                mi = lambda: hipconv._miopen_backward(dy, x, w, tr, stride, pad, dil, [False, True, False])
            else:
                op = {("fwd", False): ops.CONV_FWD, ("dx", False): ops.CONV_BWD_DATA, ("fwd", True): ops.CONVT_FWD, ("dx", True): ops.CONVT_BWD_DATA}[name, tr]
                base = hipconv.select(op, *lay[1:])
                sm_op, ops_ab = hipconv._smallmap_op(op), ((x, w) if name == "fwd" else (dy, w))
                mi = (lambda: hipconv._miopen_forward(x, w, tr, stride, pad, dil)) if name == "fwd" else \
                    (lambda: hipconv._miopen_backward(dy, x, w, tr, stride, pad, dil, [True, False, False]))
            variants = {"miopen": mi}
            if ops.smallmap_supported(sm_op, *g):
                variants["stream"] = lambda: ops.conv_smallmap(sm_op, *ops_ab, *g)
            if name != "dw" and ops.smallmap_supported(sm_op, *g, tiled=True):
                variants["tiled"] = lambda: ops.conv_smallmap(sm_op, *ops_ab, *g, tiled=True)
            t = {v: [] for v in variants}
            for _ in range(a.rounds):
                for v, fn in variants.items():
                    t[v].append(timed(fn, a.iters, a.inner))
            sweep = ""
            if "tiled" in variants and a.sweep:          # the tiled regime under a forced number of splits (debug option 6)
                L = _lib.lib()
                try:
                    for ks in (int(v) for v in a.sweep.split(",")):
                        _lib.check(L.ipsr_debug_set_option(6, ks), "ipsr_debug_set_option")
                        sweep += "  ks%d=%.2f" % (ks, timed(variants["tiled"], a.iters, a.inner))
                finally:
                    L.ipsr_debug_set_option(6, 0)
            med = {v: statistics.median(r) for v, r in t.items()}
            spread = {v: max(r) - min(r) for v, r in t.items()}
            ours = min((v for v in med if v != "miopen"), key=med.get, default=None)
            verdict = "-"
            if ours is not None:
                verdict = ("moves (%s)" % ours) if med[ours] < min(t["miopen"]) - spread["miopen"] else \
                    "loses" if med[ours] > max(t["miopen"]) + spread["miopen"] else "level"
            f = lambda d, v: "%.2f" % d[v] if v in d else "-"
            print("%-7s %-28s %-4s %-9s %5d %9s %9.2f %9s %9s %9s %9s %9s  %s" % (
                net, "%s %d->%d k%d s%d p%d d%d @%d B%d" % ((kind, Cin, Cout) + geom + (H, B)), name, base, g[0] * g[3] * g[4], f(med, "miopen"),
                min(t["miopen"]), f(spread, "miopen"), f(med, "stream"), f(spread, "stream"), f(med, "tiled"), f(spread, "tiled"), verdict + sweep), flush=True)
            for v in med:
                tot[v] += med[v]
    print("# sum of the medians over the rows that have the column, us: " + ", ".join("%s %.1f" % (v, tot[v]) for v in tot))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--inner", type=int, default=20)
    ap.add_argument("--parent-lib", default=None, help="libipsr_hip.so of the parent commit, built in another directory")
    ap.add_argument("--tiled", action="store_true", help="the table of the tiled regime against MIOpen and the streaming kernels")
    ap.add_argument("--sweep", default="", help="with --tiled: also time the tiled regime under these split counts, e.g. 8,16,32")
    a = ap.parse_args()
    if a.tiled:
        return tiled_table(a)
    L = _lib.lib()
    parent = load_parent(a.parent_lib) if a.parent_lib else None
    shapes = step_shapes(a.batch)
    st = ops._stream()
    print("# ipsr_conv_smallmap, device us per call: median of %d alternating rounds (each the median of %d event pairs around %d calls); "
          "batch %d, fp32" % (a.rounds, a.iters, a.inner, a.batch))
    print("# geometry = B,R,Cq,Ho,Wo,Hf,Wf,k,s,p,d; n = calls per step; verdict: new against parent (gained / level / slower)")
    cols = ("parent", "staged", "gathered", "c2i_loop", "new")
    print("%-5s %-34s %2s %8s %8s %8s %8s %8s %8s %8s %8s  %s" % (("op", "geometry", "n", "parent", "p.min", "p.spread") + cols[1:] + ("n.spread", "verdict")))
    setting = {"parent": (0, 0), "staged": (1, 0), "gathered": (2, 0), "c2i_loop": (0, 1), "new": (0, 0)}      # options 3 and 4
    tot = collections.Counter()
    for (op, geo), n in sorted(shapes.items()):
        B, R, Cq, Ho, Wo, Hf, Wf, k = geo[:8]
        coarse, fine, w = (B, R, Ho, Wo), (B, Cq, Hf, Wf), (R, Cq, k, k)
        sa, sb, so = {ops.SM_DATA: (coarse, w, fine), ops.SM_WRW: (coarse, fine, w), ops.SM_FWD: (fine, w, coarse)}[op]
        ta, tb = torch.randn(sa, device="cuda"), torch.randn(sb, device="cuda") * 0.05
        out = torch.empty(so, device="cuda")
        nbytes = L.ipsr_conv_smallmap_workspace_bytes(op, *geo)
        if parent is not None:
            assert parent.ipsr_conv_smallmap_workspace_bytes(op, *geo) == nbytes, "the workspace size moved"
        ws = torch.empty(nbytes, dtype=torch.uint8, device="cuda")

        def call(lib):
            rc = lib.ipsr_conv_smallmap(op, ta.data_ptr(), tb.data_ptr(), out.data_ptr(), *geo, ws.data_ptr(), nbytes, st)
            if rc != 0:
                raise RuntimeError("ipsr_conv_smallmap: %d" % rc)

        variants = [v for v in cols if (v != "parent" or parent is not None) and (v != "c2i_loop" or op == ops.SM_DATA)]
        t = {v: [] for v in variants}
        try:
            for _ in range(a.rounds):
                for v in variants:
                    for key, val in zip((3, 4), setting[v]):
                        _lib.check(L.ipsr_debug_set_option(key, val), "ipsr_debug_set_option")
                    t[v].append(timed((lambda: call(parent)) if v == "parent" else (lambda: call(L)), a.iters, a.inner))
        finally:
            L.ipsr_debug_set_option(3, 0)
            L.ipsr_debug_set_option(4, 0)
        med = {v: statistics.median(x) for v, x in t.items()}
        spread = {v: max(x) - min(x) for v, x in t.items()}
        verdict = "-"
        if parent is not None:
            if med["new"] < min(t["parent"]) - spread["parent"]:
                verdict = "gained"
            elif med["new"] > max(t["parent"]) + spread["parent"]:
                verdict = "slower"
            else:
                verdict = "level"
        for v in variants:
            tot[v] += med[v] * n
        f = lambda v: "%.2f" % med[v] if v in med else "-"
        print("%-5s %-34s %2d %8s %8s %8s %8s %8s %8s %8s %8.2f  %s" % (
            OP_NAME[op], ",".join(map(str, geo)), n, f("parent"), "%.2f" % min(t["parent"]) if parent else "-",
            "%.2f" % spread["parent"] if parent else "-", f("staged"), f("gathered"), f("c2i_loop"), f("new"), spread["new"], verdict), flush=True)
    print("# per step (sum of median x n), us: " + ", ".join("%s %.1f" % (v, tot[v]) for v in tot))


if __name__ == "__main__":
    main()
