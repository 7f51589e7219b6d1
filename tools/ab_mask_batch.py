#!/usr/bin/env python3
"""A/B of the batched per-sample-mask entries against one call per sample, inside one process (IPSR_model.batched_masks: True = ONE
ipsr_mask_index for feature masks + index and ONE innercos_loss_masks per tap, False = ipsr_feat_mask / ipsr_index_prep /
innercos_loss once per sample).  After warm-up the two routes alternate; every time is HOST wall clock around a run of calls that a
device synchronise ends: the routes differ in how many dispatches the host enqueues, which device events between launches would hide.

  (a) mask -> index   [8,256,256] and [4,512,512] stroke masks: the per-row sequence vs ops.mask_index
  (b) the two taps    [8,512,32,32] and [8,1024->512,32,32] with per-sample masks: the loop vs one call
  (c) the whole step  batch 8, 256x256, fp32, a fresh batch of per-sample stroke masks every step (set_input + set_ref_latent +
                      set_gt_latent + optimize_parameters, as bench.py times it): switch off vs on, images/s

(a), (b): median over `--rounds` alternated rounds of `--reps` repetitions each, and the spread (max - min) of each arm's rounds.
(c): `--step-rounds` alternated rounds of `--steps` steps each; every round of both arms is printed.

    python tools/ab_mask_batch.py > profiles/mask_batch_ab.txt
"""
import argparse
import os
import statistics
import sys
import tempfile
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from deepinpainting_amd import _lib, ops  # noqa: E402
from deepinpainting_amd.models.IPSR_model import IPSR_model  # noqa: E402
from deepinpainting_amd.util.staging import random_stroke_mask  # noqa: E402

COUNTED = ("ipsr_mask_index", "ipsr_feat_mask", "ipsr_index_prep", "innercos_loss", "innercos_loss_masks")


def wall_us(fn, reps):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / reps * 1e6


def alternate(arms, rounds, reps):
    """arms: {name: fn} -> {name: [us per call, one per round]}, the arms taking turns inside every round."""
    for fn in arms.values():
        for _ in range(10):
            fn()
    out = {name: [] for name in arms}
    for _ in range(rounds):
        for name, fn in arms.items():
            out[name].append(wall_us(fn, reps))
    return out


def report(label, t):
    old, new = t["per sample"], t["batched"]
    mo, mn = statistics.median(old), statistics.median(new)
    print("%-34s %10.1f %8.1f %10.1f %8.1f %7.2fx" % (label, mo, max(old) - min(old), mn, max(new) - min(new), mo / mn), flush=True)
    return mo, mn


def stroke_masks(R, size, seed):
    return torch.cat([random_stroke_mask(size, torch.Generator().manual_seed(seed + r), device="cuda") for r in range(R)], 0)[:, 0].contiguous()


def mask_to_index(a):
    print("# (a) mask -> feature masks + flags + ordered index + counts, 3 layers, threshold 5/16, shift_sz 1; us per mask BATCH")
    print("%-34s %10s %8s %10s %8s %8s" % ("masks", "per sample", "spread", "batched", "spread", "ratio"))
    for R, size in ((8, 256), (4, 512)):
        masks = stroke_masks(R, size, 100)

        def per_sample():
            feat = torch.cat([ops.feat_mask(m, 3, 5 / 16.0)[None] for m in masks], 0)
            outs = [ops.index_prep(f, 1, 1, 1) for f in feat]
            return feat, torch.stack([o[0] for o in outs]), torch.stack([o[1] for o in outs]), torch.cat([o[2] for o in outs])

        def batched():
            return ops.mask_index(masks, 3, 5 / 16.0, 1, 1, 1)
        assert all(torch.equal(x, y) for x, y in zip(per_sample(), batched())), "the two routes disagree"
        report("[%d,%d,%d] bool" % (R, size, size), alternate({"per sample": per_sample, "batched": batched}, a.rounds, a.reps))


def taps(a):
    print("# (b) the loss taps with one mask per sample, strength 1; us per tap (forward value only, as the training step uses it)")
    print("%-34s %10s %8s %10s %8s %8s" % ("x -> channels used", "per sample", "spread", "batched", "spread", "ratio"))
    g = torch.Generator(device="cuda").manual_seed(5)
    feat = ops.mask_index(stroke_masks(8, 256, 100), 3, 5 / 16.0, 1, 1, 1)[0].float()
    for B, Cx, Cuse, h in ((8, 512, 512, 32), (8, 1024, 512, 32)):
        x = torch.randn(B, Cx, h, h, device="cuda", generator=g)
        t = torch.rand(B, Cuse, h, h, device="cuda", generator=g)

        def per_sample():
            return torch.stack([ops.innercos_loss(x[b:b + 1], Cuse, feat[b], t[b:b + 1], 1.0) for b in range(B)]).mean()

        def batched():
            return ops.innercos_loss(x, Cuse, feat, t, 1.0)
        lo, ln = float(per_sample()), float(batched())
        assert abs(lo - ln) <= 1e-6 * abs(lo), "the two routes disagree: %r %r" % (lo, ln)
        report("[%d,%d,%d,%d] -> %d" % (B, Cx, h, h, Cuse), alternate({"per sample": per_sample, "batched": batched}, a.rounds, a.reps))


def whole_step(a):
    from deepinpainting_amd.models.models import create_model
    from deepinpainting_amd.options import Option
    import contextlib
    import io
    B, size = 8, 256
    opt = Option(gpu_ids=[0], batchSize=B, use_dropout=True, quiet=True, allow_random_vgg=True, checkpoints_dir=tempfile.mkdtemp(prefix="ipsr_ab_"))
    torch.manual_seed(1234)
    with contextlib.redirect_stdout(io.StringIO()):
        model = create_model(opt)
    g = torch.Generator(device="cuda").manual_seed(9)
    img = torch.rand(B, 3, size, size, device="cuda", generator=g) * 2 - 1
    ref = torch.rand(B, 3, size, size, device="cuda", generator=g) * 2 - 1
    pool = [stroke_masks(B, size, 1000 + 16 * i)[:, None] for i in range(4)]
    L = _lib.lib()
    seen = {}
    plain = {name: getattr(L, name) for name in COUNTED}

    def step(i):
        model.set_input(img, pool[i % len(pool)].clone(), ref)     # a new tensor every step: set_mask computes, as with a data loader
        model.set_ref_latent()
        model.set_gt_latent()
        model.optimize_parameters()

    def count_calls(on):
        """library calls of one step, by name (wrappers on the handle for this one step only)"""
        IPSR_model.batched_masks = on
        seen.clear()
        for name, fn in plain.items():
            setattr(L, name, lambda *args, _fn=fn, _n=name: (seen.__setitem__(_n, seen.get(_n, 0) + 1), _fn(*args))[1])
        step(0)
        torch.cuda.synchronize()
        for name, fn in plain.items():
            setattr(L, name, fn)
        return dict(seen)

    for on in (False, True):
        IPSR_model.batched_masks = on
        for i in range(5):
            step(i)
    print("# (c) the training step, batch %d, %dx%d, fp32, a fresh batch of per-sample stroke masks every step; %d steps per round" % (B, size, size, a.steps))
    print("library calls of the input and tap path in one step, per sample: %s" % sorted(count_calls(False).items()))
    print("library calls of the input and tap path in one step, batched:    %s" % sorted(count_calls(True).items()))
    rate = {False: [], True: []}
    for r in range(a.step_rounds):
        for on in (False, True):
            IPSR_model.batched_masks = on
            step(0)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for i in range(a.steps):
                step(i)
            torch.cuda.synchronize()
            rate[on].append(B * a.steps / (time.perf_counter() - t0))
    IPSR_model.batched_masks = True
    for on, name in ((False, "per sample"), (True, "batched")):
        v = rate[on]
        print("%-11s images/s per round: %s   median %.1f, lowest %.1f, spread %.1f" % (name, " ".join("%.1f" % x for x in v), statistics.median(v), min(v), max(v) - min(v)))
    old, new = rate[False], rate[True]
    diff = statistics.median(new) - statistics.median(old)
    noise = max(max(old) - min(old), max(new) - min(new))
    print("batched - per sample: %+.1f images/s (%+.2f%%); the larger spread of the two arms is %.1f: %s" % (
        diff, 100.0 * diff / statistics.median(old), noise, "outside the spread" if abs(diff) > noise else "NO difference outside the spread"))
    print("batched median >= lowest per-sample round: %s" % (statistics.median(new) >= min(old)))
    errs = model.get_current_errors()
    assert all(v == v and abs(v) != float("inf") for v in errs.values()), errs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=2000)
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--step-rounds", type=int, default=5)
    ap.add_argument("--skip-step", action="store_true", help="(a) and (b) only")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("ab_mask_batch.py needs the GPU: the entries it times have no CPU path")
    torch.cuda.set_device(0)
    print("# host wall clock on %s; median of %d alternated rounds of %d repetitions, spread = max - min over the rounds" % (
        torch.cuda.get_device_name(0), a.rounds, a.reps))
    mask_to_index(a)
    taps(a)
    if not a.skip_step:
        whole_step(a)


if __name__ == "__main__":
    main()
