"""The reference of the image-quality tests: the float64 restatement of DESIGN.md "Image quality" (the issue's "The metric, exactly"),
written with F.conv2d in double on the CPU, and the tiling plan of csrc/image_quality.hip restated.  A plain module (like
golden_cases.py).  The reference is THIS file, not the code under test: nothing here imports deepinpainting_amd.

    window()                      2-D 11x11 Gaussian, sigma 1.5, normalised, rounded to float32
    ssim(X, Y) -> [B] float64     depthwise, stride 1, no padding, C1 = 0.01^2, C2 = 0.03^2, cs clamped at 0, no rescaling
    quality(X, Y) -> [B,3]        {ssim, mean (x - y)^2, mean |x - y|} per image, float64
    psnr_of_mse(mse, peak=2)      100 where mse == 0, else 10 log10(peak^2 / mse)
"""
import numpy as np
import torch
import torch.nn.functional as F

C1, C2 = 0.01 ** 2, 0.03 ** 2

# csrc/image_quality.hip
T = 32                          # IQ_T: output tile edge
WIN = 11                        # IQ_WIN
THREADS = 256                   # IQ_THREADS
IQ_SSIM = 1                     # IPSR_IQ_SSIM


def tiles(n):
    """Tiles along an extent of n input pixels."""
    return -(-(n - (WIN - 1)) // T) if n > WIN - 1 else 1


def workspace_bytes(B, C, H, W):
    """One fp64 triple per workgroup = per (image, channel, tile)."""
    return B * C * tiles(H) * tiles(W) * 3 * 8


def window():
    x, y = np.mgrid[-5:6, -5:6]
    g = np.exp(-(x ** 2 + y ** 2) / (2.0 * 1.5 ** 2))
    return (g / g.sum()).astype(np.float32)


def ssim(X, Y):
    X, Y = X.detach().cpu().double(), Y.detach().cpu().double()
    C = X.shape[1]
    w = torch.from_numpy(window()).double()[None, None].repeat(C, 1, 1, 1)
    mu1, mu2 = F.conv2d(X, w, groups=C), F.conv2d(Y, w, groups=C)
    s1 = F.conv2d(X * X, w, groups=C) - mu1 * mu1
    s2 = F.conv2d(Y * Y, w, groups=C) - mu2 * mu2
    s12 = F.conv2d(X * Y, w, groups=C) - mu1 * mu2
    cs = F.relu((2 * s12 + C2) / (s1 + s2 + C2))
    ssim_map = ((2 * mu1 * mu2 + C1) / (mu1 * mu1 + mu2 * mu2 + C1)) * cs
    return ssim_map.mean([1, 2, 3])


def quality(X, Y, with_ssim=True):
    Xd, Yd = X.detach().cpu().double(), Y.detach().cpu().double()
    d = (Xd - Yd).flatten(1)
    s = ssim(Xd, Yd) if with_ssim else torch.full((X.shape[0],), float("nan"), dtype=torch.float64)
    return torch.stack((s, (d * d).mean(1), d.abs().mean(1)), 1)


def psnr_of_mse(mse, peak=2.0):
    mse = torch.as_tensor(mse, dtype=torch.float64)
    return torch.where(mse == 0, torch.full_like(mse, 100.0), 10.0 * torch.log10(peak * peak / torch.where(mse == 0, torch.ones_like(mse), mse)))
