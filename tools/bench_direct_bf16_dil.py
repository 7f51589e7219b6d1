#!/usr/bin/env python3
"""The direct bf16 kernels of netG's dilated down convolution Conv2d(C, C, k4, stride 2, pad 3, dilation 2) under bf16 activations
(ops.conv4x4s2_bf16_dil, engine "bf16d" under hipconv.set_direct_dilated_bf16(True) / opt.direct_dilated_bf16; its weight gradient
ops.conv4x4s2_bf16_dil_wrw under hipconv.set_direct_dilated_bf16_dw(True) / opt.direct_dilated_bf16_dw), in the style of
tools/bench_direct_bf16x3.py:

  layers   the step's four dilated layers at batch 16, the legs of `--passes` (fwd, bwdD: bf16 NCHW in and out; wrw: bf16 in, fp32 dW): the
           kernel against what `select` / `select_wrw` answers for the shape with the switches off — "wino_dil" through the dispatcher's own
           call, "miopen" through the dispatcher's MIOpen path (the fp32 weight cast to bf16 per call, as in the step) — alternated in ONE
           process over `--rounds` rounds; device time per call by HIP events around `--iters` back-to-back calls, median and [min..max] of the
           rounds; err = max |y - y64| / max |y64| against the fp64 convolution of the bf16-rounded operands (first two images; the weight
           gradient: the whole batch).
  steps    the config-5 step rate, `bench.py --gpus 1 --dtype bf16 --batch 16` as it stands, with the switch off and on: one fresh bench.py
           process per measurement, off and on alternated over `--rounds` rounds.  "on" runs bench.py through this file (`--bench-child`), which
           does nothing but make `Option` carry the switch before bench.py builds its model.  Without `--dilated-dw` the switch is
           direct_dilated_bf16; with it the switch is direct_dilated_bf16_dw and direct_dilated_bf16 is on in BOTH columns.

    python tools/bench_direct_bf16_dil.py [--what layers steps] [--out profiles/direct_bf16_dil_layers.txt]
    python tools/bench_direct_bf16_dil.py --passes wrw --dilated-dw --out profiles/direct_bf16_dil_wrw_layers.txt
"""
import argparse
import json
import os
import runpy
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

# (channels, H = W of the module's input): netG's dilated levels whose coarse grid is 16 .. 128 wide
DIL_LAYERS = [(64, 256), (128, 128), (256, 64), (512, 32)]


def burst_ms(fn, iters):
    import torch
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters


def layers(B, iters, rounds, emit, passes=("fwd", "bwdD", "wrw")):
    import torch
    import torch.nn.functional as F
    import bench  # noqa: F401  (private MIOpen db copy)
    from deepinpainting_amd import ops
    from deepinpainting_amd.models import hipconv
    BF16 = torch.bfloat16
    g = torch.Generator(device="cuda").manual_seed(9)
    hipconv.set_direct_dilated_bf16(False)
    hipconv.set_direct_dilated_bf16_dw(False)
    emit("k4 s2 p3 d2 passes (%s) under bf16 activations, batch %d, bf16 NCHW in (weight gradient: fp32 dW out); ms = device time per call (HIP events, %d calls per burst, "
         "median of %d alternated rounds, [min..max]); TF = useful flop / time" % (" ".join(passes), B, iters, rounds))
    emit("err = max |y - y64| / max |y64| against the fp64 convolution of the bf16-rounded operands; today = the engine select / select_wrw answers with the switches off")
    emit("wins = the kernel's slowest round is faster than today's fastest round; loses = the reverse; ties = the ranges overlap")
    emit("%-22s %-5s | %-40s | %-44s | %s" % ("layer", "pass", "direct bf16  ms [min..max]  TF   err", "today's engine  ms [min..max]  err", "today / direct"))
    for C, H in DIL_LAYERS:
        n = H // 2
        lay = (False, B, C, H, H, C, 4, 2, 3, 2)
        w = torch.randn(C, C, 4, 4, device="cuda", generator=g) * (1.0 / (4.0 * (C ** 0.5)))
        x = torch.randn(B, C, H, H, device="cuda", generator=g).to(BF16)
        dy = torch.randn(B, C, n, n, device="cuda", generator=g).to(BF16)
        flops = 2.0 * 16 * C * C * B * n * n
        for name, op, inp in (("fwd", ops.CONV_FWD, x), ("bwdD", ops.CONV_BWD_DATA, dy)):
            if name not in passes:
                continue
            mode = ops.S2_FINE_TO_COARSE if name == "fwd" else ops.S2_COARSE_TO_FINE
            label = "conv %4d->%-4d @%-3d   %-5s" % (C, C, H, name)
            today = hipconv.select(op, B, C, H, H, C, 4, 2, 3, 2, True)
            if not ops.conv4x4s2_bf16_dil_supported(mode, B, C, C, n, n):
                emit("%s | unsupported (today: %s)" % (label, today))
                continue
            if today != "miopen":
                base = lambda: hipconv._run_data(today, op, inp, w, lay, hipconv.conv_math(True), BF16)
            elif name == "fwd":
                def base():
                    with torch.autocast(device_type="cuda", dtype=BF16):
                        return hipconv._miopen_forward(x, w, False, 2, 3, 2)
            else:
                base = lambda: hipconv._miopen_backward(dy, x, w, False, 2, 3, 2, [True, False, False])[0]
            wd = w.to(BF16).double()
            ref = F.conv2d(inp[:2].double(), wd, None, 2, 3, 2) if name == "fwd" else F.conv_transpose2d(inp[:2].double(), wd, None, 2, 3, 1, 1, 2)
            engines = [("direct", lambda: ops.conv4x4s2_bf16_dil(mode, inp, w, B, C, C, n, n)), ("today", base)]
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


        if "wrw" in passes:
            label = "conv %4d->%-4d @%-3d   %-5s" % (C, C, H, "wrw")
            today = hipconv.select_wrw(False, B, C, H, H, C, 4, 2, 3, 2, True)
            if not ops.conv4x4s2_bf16_dil_wrw_supported(B, C, C, n, n):
                emit("%s | unsupported (today: %s)" % (label, today))
                continue
            if today != "miopen":
                base = lambda: hipconv._run_wrw(today, x, dy, w, lay, hipconv.conv_math(True))
            else:
                base = lambda: hipconv._miopen_backward(dy, x, w, False, 2, 3, 2, [False, True, False])[1]
            w64 = torch.zeros(C, C, 4, 4, dtype=torch.float64, device="cuda", requires_grad=True)
            ref = torch.zeros(C, C, 4, 4, dtype=torch.float64, device="cuda")
            for b in range(B):                                  # image by image: the fp64 copies of the 256x256 level stay small
                ref += torch.autograd.grad(F.conv2d(x[b:b + 1].double(), w64, None, 2, 3, 2), w64, dy[b:b + 1].double())[0]
            engines = [("direct", lambda: ops.conv4x4s2_bf16_dil_wrw(x, dy, B, C, C, n, n)), ("today", base)]
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
            verdict = "wins" if max(ms["direct"]) < min(ms["today"]) else "loses" if min(ms["direct"]) > max(ms["today"]) else "ties"
            emit("%s | %7.4f [%6.4f..%6.4f] %6.1f %.1e | %-9s %7.4f [%6.4f..%6.4f] %.1e | %.2fx %s" %
                 (label, md["direct"], min(ms["direct"]), max(ms["direct"]), flops / md["direct"] / 1e9, err["direct"], today, md["today"],
                  min(ms["today"]), max(ms["today"]), err["today"], md["today"] / md["direct"], verdict))


def steps(B, ksteps, warmup, rounds, emit, dilated_dw=False):
    """bench.py as it stands, one process per measurement, the switch off and on alternated.  dilated_dw: the switch is direct_dilated_bf16_dw,
    and direct_dilated_bf16 is on in both columns."""
    args = ["--gpus", "1", "--dtype", "bf16", "--batch", str(B), "--steps", str(ksteps), "--warmup", str(warmup)]
    me = [sys.executable, os.path.abspath(__file__)]
    switch = "direct_dilated_bf16_dw" if dilated_dw else "direct_dilated_bf16"
    cmds = {"off": me + ["--bench-child=direct_dilated_bf16"] + args if dilated_dw else [sys.executable, os.path.join(ROOT, "bench.py")] + args,
            "on": me + ["--bench-child=direct_dilated_bf16,direct_dilated_bf16_dw" if dilated_dw else "--bench-child=direct_dilated_bf16"] + args}
    rate = {"off": [], "on": []}
    for _ in range(rounds):
        for k in ("off", "on"):
            res = subprocess.run(cmds[k], cwd=ROOT, capture_output=True, text=True)
            if res.returncode != 0:
                raise SystemExit("bench.py (%s) failed:\n%s" % (k, res.stderr[-2000:]))
            want = ["direct_dilated_bf16=%s" % (dilated_dw or k == "on")] + (["direct_dilated_bf16_dw=%s" % (k == "on")] if dilated_dw else [])
            if (k == "on" or dilated_dw) and not all(line in res.stderr.splitlines() for line in want):
                raise SystemExit("the switches of the '%s' run did not reach its model (%s)" % (k, want))
            line = [ln for ln in res.stdout.splitlines() if ln.startswith("{")][-1]
            rate[k].append(float(json.loads(line)["value"]))
    emit("config-5 step rate: bench.py --gpus 1 --dtype bf16 --batch %d --steps %d --warmup %d, one process per measurement, %d alternated rounds, images/s%s"
         % (B, ksteps, warmup, rounds, "; direct_dilated_bf16 on in both columns" if dilated_dw else ""))
    for k in ("off", "on"):
        emit("  %s %-3s  median %7.1f (%s)" % (switch, k, statistics.median(rate[k]), " ".join("%.1f" % r for r in rate[k])))
    apart = min(rate["on"]) > max(rate["off"]) or max(rate["on"]) < min(rate["off"])
    emit("  on / off = %.3f, the ranges %s" % (statistics.median(rate["on"]) / statistics.median(rate["off"]), "are apart" if apart else "overlap"))


def bench_child(fields, argv):
    """bench.py with `opt.<field> = True` for every name in `fields`: every Option built from here on carries them; bench.py itself is run as
    it stands."""
    from deepinpainting_amd.options import Option
    init = Option.__init__

    def with_switch(self, **overrides):
        for name in fields:
            overrides.setdefault(name, True)
        init(self, **overrides)
    Option.__init__ = with_switch
    sys.argv = [os.path.join(ROOT, "bench.py")] + argv
    try:
        runpy.run_path(sys.argv[0], run_name="__main__")
    finally:
        from deepinpainting_amd.models import hipconv
        print("direct_dilated_bf16=%s" % hipconv.direct_dilated_bf16(), file=sys.stderr)         # what `steps` checks the runs by
        print("direct_dilated_bf16_dw=%s" % hipconv.direct_dilated_bf16_dw(), file=sys.stderr)


def main():
    if len(sys.argv) > 1 and sys.argv[1].startswith("--bench-child"):
        fields = sys.argv[1].partition("=")[2] or "direct_dilated_bf16"
        assert set(fields.split(",")) <= {"direct_dilated_bf16", "direct_dilated_bf16_dw"}, fields
        return bench_child(fields.split(","), sys.argv[2:])
    import torch
    ap = argparse.ArgumentParser()
    ap.add_argument("--what", nargs="+", default=["layers", "steps"], choices=("layers", "steps"))
    ap.add_argument("--passes", nargs="+", default=["fwd", "bwdD", "wrw"], choices=("fwd", "bwdD", "wrw"), help="the legs of `layers`")
    ap.add_argument("--dilated-dw", action="store_true", help="`steps`: off / on = direct_dilated_bf16_dw, with direct_dilated_bf16 on in both columns")
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--step-rounds", type=int, default=2)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("needs the GPU: nothing is measured without one")
    fh = open(a.out, "a" if a.out and "layers" not in a.what else "w") if a.out else None

    def emit(line):
        print(line, flush=True)
        if fh:
            fh.write(line + "\n")
            fh.flush()
    emit("# tools/bench_direct_bf16_dil.py on %s" % torch.cuda.get_device_name(0))
    if "layers" in a.what:
        layers(a.batch, a.iters, a.rounds, emit, tuple(a.passes))
    if "steps" in a.what:
        steps(a.batch, a.steps, a.warmup, a.step_rounds, emit, a.dilated_dw)


if __name__ == "__main__":
    main()
