"""What the evaluation path costs: recorded in profiles/image_quality.txt, no pass mark hangs on it.

  1. `ops.image_quality` (the HIP kernel, fp64) at [1,3,256,256] and [16,3,256,256] beside a torch fp32 composite of the same three
     numbers on the same tensors (grouped F.conv2d SSIM + two means), HIP events around `iters` back-to-back calls after a warm-up;
  2. images/s of test.ipynb's loop as written (batch 1, autograd on, two host reads per image) against `metrics.evaluate` at batch 16
     with one mask per sample and one host read at the end, on the same synthetic images and masks.

    python tools/bench_image_quality.py [--images 64] [--iters 200] [--out FILE]
"""
import argparse
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
os.environ.setdefault("IPSR_ALLOW_RANDOM_VGG", "1")

import torch  # noqa: E402


def _events(fn, iters, warmup=10):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / iters * 1e3          # us per call


def kernel_table(iters, say):
    from deepinpainting_amd import metrics, ops
    win = torch.from_numpy(ops.ssim_window()).cuda()
    say("call (HIP events, %d back-to-back calls after 10 warm-up calls, random pair in [-1,1])" % iters)
    for B in (1, 16):
        g = torch.Generator(device="cuda").manual_seed(B)
        X = torch.rand(B, 3, 256, 256, device="cuda", generator=g) * 2 - 1
        Y = (X + 0.05 * torch.randn(B, 3, 256, 256, device="cuda", generator=g)).clamp(-1, 1)

        def composite():
            d = (X - Y).flatten(1)
            return metrics._ssim_map_mean(X, Y, win), (d * d).mean(1), d.abs().mean(1)
        rounds = []
        for _ in range(3):                         # alternated
            rounds.append((_events(lambda: ops.image_quality(X, Y), iters), _events(lambda: ops.image_quality(X, Y, ssim=False), iters),
                           _events(composite, iters)))
        q = ops.image_quality(X, Y)
        c = composite()
        err = float((q[:, 0] - c[0].double()).abs().max())
        for name, col in (("ops.image_quality (fp64, 2 launches)", 0), ("ops.image_quality ssim=False", 1), ("torch fp32 composite (SSIM + 2 means)", 2)):
            say("  [%2d,3,256,256] %-40s %s us" % (B, name, " / ".join("%.1f" % r[col] for r in rounds)))
        say("  [%2d,3,256,256] max |fp32 composite SSIM - kernel SSIM| = %.2e" % (B, err))


def loops(n_images, say):
    from deepinpainting_amd import metrics
    from deepinpainting_amd.models.models import create_model
    from deepinpainting_amd.options import Option
    opt = Option(gpu_ids=[0], use_dropout=False, quiet=True, checkpoints_dir=tempfile.mkdtemp(prefix="ipsr_iq_"))
    model = create_model(opt)
    g = torch.Generator().manual_seed(0)
    images = torch.rand(n_images, 3, 256, 256, generator=g) * 2 - 1
    masks = torch.zeros(n_images, 1, 256, 256)
    for i in range(n_images):
        y0, x0 = 16 + (37 * i) % 120, 16 + (53 * i) % 120
        masks[i, :, y0:y0 + 96, x0:x0 + 80] = 1

    def notebook():
        mod = metrics.SSIM(channels=3)
        psnr_sum, ssim_sum = 0, 0
        for i in range(n_images):
            image, mask = images[i:i + 1].cuda(), masks[i:i + 1].cuda()
            mask = mask[0][0].unsqueeze(0).unsqueeze(1).bool()
            model.set_input(image, mask, image)
            model.set_ref_latent()
            model.set_gt_latent()
            model.test()
            _, _, fake_B, _, real_B = model.get_current_visuals()
            mse = torch.mean((real_B - fake_B) ** 2)
            psnr = 100 if mse == 0 else 10 * torch.log10((2 ** 2) / mse)
            score = mod(real_B, fake_B, as_loss=False)
            psnr_sum += float(psnr)
            ssim_sum += float(score)
        return psnr_sum / n_images, ssim_sum / n_images

    def batched():
        it = ((images[i:i + 16], masks[i:i + 16], images[i:i + 16]) for i in range(0, n_images, 16))
        r = metrics.evaluate(model, it, max_images=n_images)
        return r["psnr_average"], r["ssim_average"]

    say("loops (%d synthetic 256x256 images, one hole each; host clock around the loop, device synchronised; one warm-up pass each, alternated)" % n_images)
    notebook(), batched()
    for _ in range(3):
        out = []
        for fn in (notebook, batched):
            torch.cuda.synchronize()
            t = time.perf_counter()
            avg = fn()
            torch.cuda.synchronize()
            out.append((n_images / (time.perf_counter() - t), avg))
        say("  test.ipynb loop, batch 1, two host reads per image: %7.1f images/s (PSNR %.4f SSIM %.5f)   metrics.evaluate, batch 16, per-sample masks, "
            "one host read: %7.1f images/s (PSNR %.4f SSIM %.5f)" % (out[0][0], out[0][1][0], out[0][1][1], out[1][0], out[1][1][0], out[1][1][1]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=64)
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU: a CPU run says nothing about this path's cost"
    torch.cuda.set_device(0)
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)
    say("image quality path on %s, torch %s" % (torch.cuda.get_device_name(0), torch.__version__))
    kernel_table(a.iters, say)
    loops(a.images, say)
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
