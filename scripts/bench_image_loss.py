"""Fused L1 + SSIM image loss (ops/image_loss.py) against the same loss composed in torch (five depthwise 11 x 11 conv2d calls and
F.l1_loss, autograd backward), forward + backward at the training shape 24 x 3 x 512^2 and the bench shape 24 x 3 x 800^2; then the
training-loss step render_loss_frames against render_frames + the torch-composed loss (262 144 Gaussians, 24 views, 800 x 800, SH 2).
GPU only.  Prints ms, the ratio, and the achieved rates against the counted bytes and FLOPs of the fused kernels."""
import math
import os
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from gvfdiffusion_amd import synthetic  # noqa: E402
from gvfdiffusion_amd.ops.image_loss import image_loss  # noqa: E402
from gvfdiffusion_amd.renderers import GaussianRenderer  # noqa: E402
from gvfdiffusion_amd.training import render_loss_frames  # noqa: E402

dev = torch.device("cuda:0")
N_STEPS = int(os.environ.get("GVF_STEPS", 20))
MODE = os.environ.get("GVF_BENCH_MODE", "lr")     # l: loss alone, r: render step; f: fused loss only (for the kernel trace)

# counted per pixel (csrc/loss.hip, 64 x 16 tiles: the horizontal passes run over 26 / 16 of the rows)
#   bytes: forward reads p, g (8) and writes the three maps (12); backward reads the maps (12) and p, g (8), writes the gradient (4)
#   FLOP (fma = 2): forward 1.625 * 110 (horizontal, 5 moments) + 110 (vertical) + ~40 (S and its partials) ~= 330;
#                   backward 1.625 * 66 + 66 + ~8 ~= 180
BYTES_PX, FLOP_PX = 44, 510


def window(C):
    g = torch.tensor([math.exp(-(x - 5) ** 2 / 4.5) for x in range(11)], dtype=torch.float32)
    g = g / g.sum()
    return torch.outer(g, g).expand(C, 1, 11, 11).contiguous().to(dev)


def torch_loss(pred, gt, w, l1_weight=1.0, ssim_weight=0.2):
    C = pred.shape[1]
    conv = lambda x: F.conv2d(x, w, padding=5, groups=C)  # noqa: E731
    mu1, mu2 = conv(pred), conv(gt)
    s1, s2, s12 = conv(pred * pred) - mu1 * mu1, conv(gt * gt) - mu2 * mu2, conv(pred * gt) - mu1 * mu2
    c1, c2 = 0.01 ** 2, 0.03 ** 2
    ssim = ((2 * mu1 * mu2 + c1) * (2 * s12 + c2) / ((mu1 * mu1 + mu2 * mu2 + c1) * (s1 + s2 + c2))).mean()
    return l1_weight * F.l1_loss(pred, gt) + ssim_weight * (1 - ssim)


def timed(fn, n):
    fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n


if "l" in MODE or "f" in MODE:
    for S in (512, 800):
        g = torch.Generator().manual_seed(0)
        gt = torch.rand((24, 3, S, S), generator=g).to(dev)
        pred = (gt + 0.1 * torch.randn((24, 3, S, S), generator=g).to(dev)).clamp(0, 1).requires_grad_(True)
        w = window(3)

        def fused():
            pred.grad = None
            image_loss(pred, gt).backward()

        def composed():
            pred.grad = None
            torch_loss(pred, gt, w).backward()

        tf = timed(fused, N_STEPS)
        px = 24 * 3 * S * S
        line = f"24x3x{S}^2 ({px / 1e6:.1f} M px): fused {tf:.3f} ms"
        if "l" in MODE:
            tc = timed(composed, N_STEPS)
            line += f", torch-composed {tc:.3f} ms, {tc / tf:.1f}x"
        line += (f"; fused achieves {BYTES_PX * px / tf / 1e9:.2f} TB/s of {BYTES_PX} counted B/px, "
                 f"{FLOP_PX * px / tf / 1e9:.1f} TFLOP/s of {FLOP_PX} counted FLOP/px")
        print(line, flush=True)
        del gt, pred

if "r" in MODE:
    P, S, V = int(os.environ.get("GVF_P", 262144)), 800, 24
    attrs = synthetic.random_gaussians(P, sh_degree=2, seed=0, scale_lo=0.002, scale_hi=0.01)
    gm = synthetic.gaussian_model_from(attrs, 2, dev)
    for k in ("_xyz", "_features_dc", "_scaling", "_rotation", "_opacity"):
        setattr(gm, k, getattr(gm, k).detach().contiguous().requires_grad_(True))
    rend = GaussianRenderer({"resolution": S, "near": synthetic.NEAR, "far": synthetic.FAR, "ssaa": 1, "bg_color": (1, 1, 1)})
    rend.pipe.use_mip_gaussian = True
    rend.pipe.kernel_size = synthetic.KERNEL_2D
    K = synthetic.intrinsics().to(dev)
    ext = torch.stack([synthetic.orbit_w2c(15.0 * v, 10.0) for v in range(V)]).to(dev)
    delta = synthetic.random_deltas(V, P, seed=1, std=0.01).to(dev).requires_grad_(True)
    with torch.no_grad():
        targets = rend.render_frames(gm, ext, K, delta_pc=synthetic.random_deltas(V, P, seed=2, std=0.02).to(dev),
                                     delta_index=list(range(V)))["rgb"].clone()
    w = window(3)

    def step_fused():
        render_loss_frames(rend, gm, ext, K, delta, targets).backward()

    def step_composed():
        imgs = rend.render_frames(gm, ext, K, delta_pc=delta, delta_index=list(range(V)))["rgb"]
        torch_loss(imgs, targets, w).backward()

    tf, tc = timed(step_fused, N_STEPS // 2), timed(step_composed, N_STEPS // 2)
    print(f"training-loss step, P={P} {S}x{S} SH2, {V} views, forward + backward: render_loss_frames {tf:.2f} ms, "
          f"render_frames + torch-composed loss {tc:.2f} ms, {tc / tf:.2f}x", flush=True)
