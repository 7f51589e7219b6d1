"""Image-quality numbers of the evaluation path: what test.ipynb asks of `IQA_pytorch` and computes by hand, in batches on the device.

    sys.modules.setdefault("IQA_pytorch", deepinpainting_amd.metrics)      # test.ipynb cell 1: from IQA_pytorch import SSIM

`SSIM` restates IQA_pytorch 0.1's SSIM from memory (DESIGN.md "Image quality" is the definition): parity with the pip package is
UNVERIFIED, the package is not available where this was written.  2-D 11x11 Gaussian window (sigma 1.5, float32), depthwise, stride 1,
no padding, C1 = 0.01^2, C2 = 0.03^2, cs clamped at 0, values taken as they are (the notebooks feed [-1,1]; the score can be negative).

CUDA tensors with `as_loss=False` go through the HIP kernel (`ops.image_quality`, fp64 sums); `as_loss=True` and CPU tensors go
through a differentiable torch composite of the same formula (grouped F.conv2d in the input's precision) — NOT the HIP path.

`Evaluator` runs test.ipynb cell 3 and train.ipynb's validation loop in batches, every sample with its own mask if wanted, and reads the
host ONCE, in `result()`.
"""
import torch
import torch.nn.functional as F

from . import ops

C1, C2 = 0.01 ** 2, 0.03 ** 2


def _ssim_map_mean(X, Y, win):
    """The definition as a torch composite: X, Y [B,C,H,W] -> [B] in X's dtype.  win [11,11] of X's dtype and device."""
    C = X.shape[1]
    w = win[None, None].expand(C, 1, 11, 11).contiguous()
    mu1, mu2 = F.conv2d(X, w, groups=C), F.conv2d(Y, w, groups=C)
    mu1_sq, mu2_sq, mu1_mu2 = mu1 * mu1, mu2 * mu2, mu1 * mu2
    s1 = F.conv2d(X * X, w, groups=C) - mu1_sq
    s2 = F.conv2d(Y * Y, w, groups=C) - mu2_sq
    s12 = F.conv2d(X * Y, w, groups=C) - mu1_mu2
    cs = F.relu((2 * s12 + C2) / (s1 + s2 + C2))
    ssim_map = ((2 * mu1_mu2 + C1) / (mu1_sq + mu2_sq + C1)) * cs
    return ssim_map.mean([1, 2, 3])


class SSIM(torch.nn.Module):
    """`IQA_pytorch.SSIM(channels=3)`: forward(X, Y, as_loss=True) -> 1 - score.mean() with gradients, or, as_loss=False, the
    per-image score [B] (float32) under no_grad."""

    def __init__(self, channels=3):
        super().__init__()
        self.channels = channels
        self.register_buffer("win", torch.from_numpy(ops.ssim_window()), persistent=False)

    def _composite(self, X, Y):
        if X.shape != Y.shape or X.dim() != 4 or X.shape[1] != self.channels:
            raise ValueError("SSIM(channels=%d): X %s and Y %s must be [B,%d,H,W] of one shape" % (self.channels, tuple(X.shape), tuple(Y.shape), self.channels))
        if X.shape[2] < 11 or X.shape[3] < 11:
            raise NotImplementedError("SSIM: H, W >= 11 (11x11 window, no padding), got %dx%d" % (X.shape[2], X.shape[3]))
        dt = X.dtype if X.dtype in (torch.float32, torch.float64) else torch.float32
        return _ssim_map_mean(X.to(dt), Y.to(dt), self.win.to(device=X.device, dtype=dt))

    def forward(self, X, Y, as_loss=True):
        if as_loss:
            return 1 - self._composite(X, Y).mean()
        with torch.no_grad():
            if X.is_cuda and Y.is_cuda:
                if X.dim() != 4 or X.shape[1] != self.channels:
                    raise ValueError("SSIM(channels=%d): X %s must be [B,%d,H,W]" % (self.channels, tuple(X.shape), self.channels))
                return ops.image_quality(X, Y, ssim=True)[:, 0].float()
            return self._composite(X, Y).float()


def _psnr_of_mse(mse, peak):
    """test.ipynb cell 3 per image: 100 where mse == 0, else 10 log10(peak^2 / mse); stays on mse's device."""
    safe = torch.where(mse == 0, torch.ones_like(mse), mse)
    return torch.where(mse == 0, torch.full_like(mse, 100.0), 10.0 * torch.log10((peak * peak) / safe))


def psnr(real, fake, peak=2.0):
    """Per-image PSNR [B] on the inputs' device (float64 from the HIP kernel's mean squared difference on CUDA tensors, the inputs'
    precision on the CPU): 100 where the two images are equal."""
    if real.is_cuda and fake.is_cuda:
        mse = ops.image_quality(real, fake, ssim=False)[:, 1]
    else:
        mse = ((real - fake) ** 2).flatten(1).mean(1)
    return _psnr_of_mse(mse, float(peak))


class Evaluator:
    """The notebooks' evaluation (test.ipynb cell 3) and validation (train.ipynb cell 2) loops in batches.

        ev = Evaluator(model)
        for image, mask, ref in loader:           # mask [1,1,H,W] bool, or one per sample [B,1,H,W]
            ev.step(image, mask, ref)
        r = ev.result()                           # the one host read

    Per image: PSNR (peak 2), SSIM, and the validation loss (mean|fake_B - real_B| + mean|fake_P - real_B|) * lambda_A of
    `IPSR.get_loss`; nothing is read back before `result()`.  `model` may be None when only `update` is used (`lambda_A` then given)."""

    def __init__(self, model=None, lambda_A=None, peak=2.0):
        self.model = model
        if lambda_A is None:
            lambda_A = model.opt.lambda_A if model is not None else 100.0
        self.lambda_A = float(lambda_A)
        self.peak = float(peak)
        self.reset()

    def reset(self):
        self._quality = []          # [B,3] float64 per batch: SSIM, mean squared and mean absolute difference of (real_B, fake_B)
        self._l1_P = []             # [B] float64 per batch: mean |fake_P - real_B|, or None

    def step(self, image, mask, ref):
        m = self.model
        with torch.no_grad():
            m.set_input(image, mask, ref)
            m.set_ref_latent()
            m.set_gt_latent()
            m.test()
            _, _, fake_B, fake_P, real_B = m.get_current_visuals()
            self.update(real_B, fake_B, fake_P)

    def update(self, real_B, fake_B, fake_P=None):
        with torch.no_grad():
            self._quality.append(ops.image_quality(real_B, fake_B, ssim=True))
            self._l1_P.append(ops.image_quality(fake_P, real_B, ssim=False)[:, 2] if fake_P is not None else None)

    def result(self):
        """-> dict of numpy float64 arrays `psnr`, `ssim`, `valid_loss` (one entry per image, NaN where no fake_P was given), their
        means `psnr_average`, `ssim_average`, `valid_loss_average`, and `images`.  The only host read of the evaluator."""
        if not self._quality:
            raise RuntimeError("Evaluator.result: no batch was added")
        q = torch.cat(self._quality, 0)
        l1p = torch.cat([p if p is not None else torch.full_like(b[:, 2], float("nan")) for p, b in zip(self._l1_P, self._quality)], 0)
        table = torch.stack((_psnr_of_mse(q[:, 1], self.peak), q[:, 0], (q[:, 2] + l1p) * self.lambda_A), 0).cpu().numpy()
        ps, ss, vl = table[0], table[1], table[2]
        return dict(psnr=ps, ssim=ss, valid_loss=vl, psnr_average=float(ps.mean()), ssim_average=float(ss.mean()),
                    valid_loss_average=float(vl.mean()), images=int(ps.shape[0]))


def evaluate(model, iterator, max_images=500):
    """test.ipynb cell 3 over a DataLoader-like iterator of (image, mask, ref): the reference image is the image itself, as in the
    notebook.  mask [1,*,H,W] (one hole for the batch) or [B,*,H,W] (one per sample), any dtype: channel 0, made bool, as the
    notebook's `mask[0][0]` does for its batch of one.  Stops after `max_images` images -> Evaluator.result()."""
    ev = Evaluator(model)
    seen = 0
    for image, mask, ref in iterator:
        if seen >= max_images:
            break
        if seen + image.size(0) > max_images:
            keep = max_images - seen
            image, mask = image[:keep], (mask[:keep] if mask.size(0) > 1 else mask)
        dev = getattr(model, "device", "cuda")
        image, mask = image.to(dev), mask.to(dev)[:, :1].bool()
        ev.step(image, mask, image)
        seen += image.size(0)
    return ev.result()
