"""Float64 oracle of the SSIM / L1 image loss (utils/loss_util.py:ssim semantics), written as explicit window sums rather than as
the reference's conv2d calls, and differentiable through torch autograd (so that device tests can take its gradient).

Window: the one the reference convolves with -- the 1-D taps exp(-(x-5)^2 / 4.5) rounded to fp32 and normalised by their fp32 sum,
their outer product rounded to fp32 -- then applied in float64.  The HIP kernels apply the 1-D taps separably; the products differ
from this window by at most 1 fp32 ulp per weight.

Also: `ssim_torch32`, the same formula as an fp32 torch composition (depthwise conv2d), the yardstick the device tests calibrate
their bars with."""
import math

import torch
import torch.nn.functional as F

WIN, RAD = 11, 5
C1, C2 = 0.01 ** 2, 0.03 ** 2


def taps32() -> torch.Tensor:
    g = torch.tensor([math.exp(-((x - RAD) ** 2) / (2 * 1.5 ** 2)) for x in range(WIN)], dtype=torch.float32)
    return g / g.sum()


def window32() -> torch.Tensor:
    g = taps32()
    return torch.outer(g, g)          # each weight one fp32 rounding of the product


def _as4d(x: torch.Tensor) -> torch.Tensor:
    return x.unsqueeze(0) if x.dim() == 3 else x


def _wsum(x: torch.Tensor, w: torch.Tensor) -> torch.Tensor:
    """sum_{i,j} w[i,j] x[y+i-5, x+j-5] with zero padding, per plane, as 121 shifted slices (float64)."""
    H, W = x.shape[-2:]
    xp = F.pad(x, (RAD, RAD, RAD, RAD))
    out = torch.zeros_like(x)
    for i in range(WIN):
        for j in range(WIN):
            out = out + w[i, j] * xp[..., i:i + H, j:j + W]
    return out


def ssim_map64(img1: torch.Tensor, img2: torch.Tensor) -> torch.Tensor:
    p, g = _as4d(img1).double(), _as4d(img2).double()
    w = window32().double().to(p.device)
    mu1, mu2 = _wsum(p, w), _wsum(g, w)
    s1 = _wsum(p * p, w) - mu1 * mu1
    s2 = _wsum(g * g, w) - mu2 * mu2
    s12 = _wsum(p * g, w) - mu1 * mu2
    return (2 * mu1 * mu2 + C1) * (2 * s12 + C2) / ((mu1 * mu1 + mu2 * mu2 + C1) * (s1 + s2 + C2))


def ssim64(img1: torch.Tensor, img2: torch.Tensor) -> torch.Tensor:
    return ssim_map64(img1, img2).mean()


def loss64(pred: torch.Tensor, target: torch.Tensor, l1_weight: float = 1.0, ssim_weight: float = 0.2) -> torch.Tensor:
    p, g = pred.double(), target.double()
    return l1_weight * (p - g).abs().mean() + ssim_weight * (1 - ssim64(p, g))


def ssim_torch32(img1: torch.Tensor, img2: torch.Tensor) -> torch.Tensor:
    """The same SSIM as an fp32 torch composition: five depthwise 11 x 11 conv2d calls (what a user would write)."""
    p, g = _as4d(img1).float(), _as4d(img2).float()
    C = p.shape[1]
    w = window32().to(p.device).expand(C, 1, WIN, WIN).contiguous()
    conv = lambda x: F.conv2d(x, w, padding=RAD, groups=C)  # noqa: E731
    mu1, mu2 = conv(p), conv(g)
    s1 = conv(p * p) - mu1 * mu1
    s2 = conv(g * g) - mu2 * mu2
    s12 = conv(p * g) - mu1 * mu2
    return ((2 * mu1 * mu2 + C1) * (2 * s12 + C2) / ((mu1 * mu1 + mu2 * mu2 + C1) * (s1 + s2 + C2))).mean()


def loss_torch32(pred: torch.Tensor, target: torch.Tensor, l1_weight: float = 1.0, ssim_weight: float = 0.2) -> torch.Tensor:
    return l1_weight * F.l1_loss(pred, target) + ssim_weight * (1 - ssim_torch32(pred, target))
