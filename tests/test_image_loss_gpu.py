"""The fused L1 + SSIM image loss (ops/image_loss.py -> gvf_image_loss_forward / _backward) on an MI355X: value and gradient against the
float64 oracle (tests/ssim_ref.py) and the reference's golden, with bars calibrated by an fp32 torch composition of the same formula
(computed on host copies: ssim_ref.ssim_torch32 / loss_torch32 return host tensors, and every comparison below is made on the host);
the L1-only case against torch; identical images; determinism; refusals; and the loss through the batched renderer in training.
The element-wise measure of the same kernels is tests/test_image_loss_conformance_gpu.py."""
import math
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import ssim_ref
from gvfdiffusion_amd import _lib, synthetic
from gvfdiffusion_amd.ops import image_loss as IL
from gvfdiffusion_amd.renderers import GaussianRenderer

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ssim_golden.npz")
W_L1, W_SSIM = 1.0, 0.2


def rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.linalg.norm(a - b) / max(1e-30, np.linalg.norm(b)))


def _pair(shape, seed, dev, noise=0.15):
    g = torch.Generator().manual_seed(seed)
    a = torch.rand(shape, generator=g)
    b = (a + noise * torch.randn(shape, generator=g)).clamp(0, 1)
    return a.to(dev), b.to(dev)


def _grad(fn, a, b):
    x = a.clone().requires_grad_(True)
    y = fn(x, b)
    y.backward()
    return y.detach(), x.grad


@pytest.mark.parametrize("shape", [(2, 3, 37, 53), (1, 3, 5, 7), (4, 3, 24, 24), (1, 3, 64, 64), (4, 3, 128, 160), (2, 3, 512, 512),
                                   (1, 3, 800, 800), (3, 1, 1), (1, 2, 1, 70), (1, 1, 67, 3)])
def test_against_the_fp64_oracle(cuda, shape):
    a, b = _pair(shape, sum(shape), cuda)
    for name, fused, t32, o64 in [("ssim", IL.ssim, ssim_ref.ssim_torch32, ssim_ref.ssim64),
                                  ("loss", IL.image_loss, ssim_ref.loss_torch32, ssim_ref.loss64)]:
        vk, gk = _grad(fused, a, b)
        vt, gt = _grad(t32, a, b)
        vo, go = _grad(o64, a.double(), b.double())
        ek, et = abs(float(vk) - float(vo)), abs(float(vt) - float(vo))
        rk, rt = rel(gk.cpu(), go.cpu()), rel(gt.cpu(), go.cpu())
        print(f"{shape} {name}: |value-fp64| hip {ek:.2e} torch32 {et:.2e}; grad rel L2 hip {rk:.2e} torch32 {rt:.2e}")
        assert gk.dtype == torch.float32 and gk.shape == a.shape and torch.isfinite(gk).all()
        assert ek <= max(2 * et, 1e-7)
        assert rk <= max(2 * rt, 1e-6)


def test_against_the_reference_golden(cuda):
    d = np.load(GOLDEN)
    for k in range(int(d["n_cases"])):
        a, b = torch.from_numpy(d[f"img1_{k}"]).to(cuda), torch.from_numpy(d[f"img2_{k}"]).to(cuda)
        vk, gk = _grad(IL.ssim, a, b)
        s64, s32 = float(d[f"ssim64_{k}"]), float(d[f"ssim32_{k}"])
        ek, er = abs(float(vk) - s64), abs(s32 - s64)
        rk, rr = rel(gk.cpu(), d[f"grad64_{k}"]), rel(d[f"grad32_{k}"], d[f"grad64_{k}"])
        print(f"golden {a.shape}: |value-fp64| hip {ek:.2e} reference fp32 {er:.2e}; grad rel L2 hip {rk:.2e} reference fp32 {rr:.2e}")
        assert ek <= max(2 * er, 1e-7)
        assert rk <= max(2 * rr, 1e-6)


def test_l1_only_equals_torch_l1(cuda):
    a, b = _pair((4, 3, 77, 91), 5, cuda)
    b[0, 0, :4] = a[0, 0, :4]                      # exact ties: sign(0) = 0
    vk, gk = _grad(lambda x, y: IL.image_loss(x, y, l1_weight=1.0, ssim_weight=0.0), a, b)
    vt, gt = _grad(F.l1_loss, a, b)
    assert abs(float(vk) - float(vt)) <= 4e-7 * abs(float(vt)), (float(vk), float(vt))
    ulps = (gk.view(torch.int32).long() - gt.view(torch.int32).long()).abs()
    assert int(ulps.max()) <= 1
    assert float(gk[0, 0, :4].abs().max()) == 0.0
    # weights and the incoming gradient scale the L1 part linearly
    x = a.clone().requires_grad_(True)
    (3.0 * IL.image_loss(x, b, l1_weight=0.5, ssim_weight=0.0)).backward()
    assert torch.allclose(x.grad, 1.5 * gt, rtol=1e-6, atol=0)


def test_identical_images(cuda):
    a, _ = _pair((2, 3, 96, 80), 7, cuda)
    s, g = _grad(IL.ssim, a, a.clone())
    assert abs(float(s) - 1.0) <= 1e-6
    _, g_ref = _grad(IL.ssim, a, _pair((2, 3, 96, 80), 8, cuda)[1])
    print(f"identical images: |1 - ssim| {abs(float(s) - 1):.1e}, max|grad| {float(g.abs().max()):.1e} vs {float(g_ref.abs().max()):.1e}")
    assert float(g.abs().max()) <= 1e-4 * float(g_ref.abs().max())


def test_deterministic_and_stream_independent(cuda):
    a, b = _pair((6, 3, 200, 260), 11, cuda)
    runs = []
    for stream in (None, None, torch.cuda.Stream(cuda)):
        if stream is not None:
            stream.wait_stream(torch.cuda.current_stream(cuda))
        with torch.cuda.stream(stream if stream is not None else torch.cuda.current_stream(cuda)):
            x = a.clone().requires_grad_(True)
            loss, l1, s = IL.image_loss(x, b, return_terms=True)
            loss.backward()
        torch.cuda.synchronize(cuda)
        runs.append((loss.detach(), l1.detach(), s.detach(), x.grad))
    for r in runs[1:]:
        for u, v in zip(runs[0], r):
            assert torch.equal(u, v)
    with torch.no_grad():
        nl, nl1, ns = IL.image_loss(a, b, return_terms=True)
    assert torch.equal(nl, runs[0][0]) and torch.equal(nl1, runs[0][1]) and torch.equal(ns, runs[0][2])
    # the terms are the loss's parts
    assert abs(float(runs[0][0]) - (W_L1 * float(runs[0][1]) + W_SSIM * (1 - float(runs[0][2])))) <= 1e-6


def test_terms_are_differentiable(cuda):
    a, b = _pair((2, 3, 40, 44), 13, cuda)
    x = a.clone().requires_grad_(True)
    loss, l1, s = IL.image_loss(x, b, l1_weight=0.7, ssim_weight=0.3, return_terms=True)
    (2.0 * l1 - 5.0 * s).backward()
    y = a.double().clone().requires_grad_(True)
    (2.0 * (y - b.double()).abs().mean() - 5.0 * ssim_ref.ssim64(y, b.double())).backward()
    assert rel(x.grad.cpu(), y.grad.cpu()) <= 1e-5


def test_refusals_and_conversions(cuda):
    a, b = _pair((2, 3, 16, 16), 17, cuda)
    with pytest.raises(_lib.GvfError):
        IL.image_loss(a.cpu(), b.cpu())
    with pytest.raises(ValueError):
        IL.image_loss(a, b[:, :, :8])
    with pytest.raises(ValueError):
        IL.ssim(a[0, 0], b[0, 0])
    with pytest.raises(ValueError):
        IL.image_loss(a, b.clone().requires_grad_(True))
    for dt in (torch.float16, torch.bfloat16):
        ah, bh = a.to(dt), b.to(dt)
        assert torch.equal(IL.image_loss(ah, bh), IL.image_loss(ah.float(), bh.float()))
        x = ah.clone().requires_grad_(True)
        IL.ssim(x, bh).backward()
        assert x.grad.dtype == dt and torch.isfinite(x.grad.float()).all()
    # non-contiguous input
    at = a.transpose(2, 3)
    assert torch.equal(IL.ssim(at, b.transpose(2, 3)), IL.ssim(at.contiguous(), b.transpose(2, 3).contiguous()))


# ---- through the renderer ------------------------------------------------------------------------------------------------------
BG = (0.3, 0.3, 0.3)
RAW = ("_xyz", "_features_dc", "_scaling", "_rotation", "_opacity")


def _renderer(S):
    rend = GaussianRenderer({"resolution": S, "near": synthetic.NEAR, "far": synthetic.FAR, "ssaa": 1, "bg_color": BG})
    rend.pipe.use_mip_gaussian = True
    rend.pipe.kernel_size = synthetic.KERNEL_2D
    return rend


def _scene(dev, P=3000, S=96, V=3):
    attrs = synthetic.random_gaussians(P, sh_degree=0, seed=21, scale_lo=0.01, scale_hi=0.05)
    deltas = synthetic.random_deltas(V, P, seed=22, std=0.01).to(dev)
    ext = torch.stack([synthetic.orbit_w2c(40.0 * f + 7.0, 10.0) for f in range(V)]).to(dev)
    K = synthetic.intrinsics().to(dev)
    rend = _renderer(S)
    with torch.no_grad():
        gm = synthetic.gaussian_model_from(attrs, 0, dev)
        targets = rend.render_frames(gm, ext, K, delta_pc=synthetic.random_deltas(V, P, seed=23, std=0.02).to(dev),
                                     delta_index=list(range(V)))["rgb"].clone()
    return attrs, deltas, ext, K, rend, targets


def _grads_through(attrs, deltas, ext, K, rend, loss_of_frames):
    gm = synthetic.gaussian_model_from(attrs, 0, deltas.device)
    for k in RAW:
        setattr(gm, k, getattr(gm, k).detach().clone().contiguous().requires_grad_(True))
    d = deltas.clone().requires_grad_(True)
    loss_of_frames(gm, d)
    g = {k: getattr(gm, k).grad for k in RAW}
    g["delta"] = d.grad
    return g


def test_render_loss_frames_gradients(cuda):
    from gvfdiffusion_amd.training import render_loss_frames
    attrs, deltas, ext, K, rend, targets = _scene(cuda)
    V = ext.shape[0]

    def oracle(gm, d):
        imgs = rend.render_frames(gm, ext, K, delta_pc=d, delta_index=list(range(V)))["rgb"]
        x = imgs.detach().double().requires_grad_(True)
        ssim_ref.loss64(x, targets.double(), W_L1, W_SSIM).backward()
        imgs.backward(x.grad.float())

    def torch32(gm, d):
        imgs = rend.render_frames(gm, ext, K, delta_pc=d, delta_index=list(range(V)))["rgb"]
        ssim_ref.loss_torch32(imgs, targets, W_L1, W_SSIM).backward()

    def fused(gm, d):
        render_loss_frames(rend, gm, ext, K, d, targets, l1_weight=W_L1, ssim_weight=W_SSIM).backward()

    go = _grads_through(attrs, deltas, ext, K, rend, oracle)
    gt = _grads_through(attrs, deltas, ext, K, rend, torch32)
    gk = _grads_through(attrs, deltas, ext, K, rend, fused)
    for k in go:
        rk, rt = rel(gk[k].cpu(), go[k].cpu()), rel(gt[k].cpu(), go[k].cpu())
        print(f"render_loss_frames {k}: rel L2 hip {rk:.2e} torch32 {rt:.2e}")
        assert torch.isfinite(gk[k]).all() and float(go[k].abs().max()) > 0
        assert rk <= max(2 * rt, 1e-6), k
    # the value: the reference's loss on the stacked views (L1 over the stack = mean of the per-view L1s)
    with torch.no_grad():
        gm = synthetic.gaussian_model_from(attrs, 0, cuda)
        v = render_loss_frames(rend, gm, ext, K, deltas, targets)
        imgs = rend.render_frames(gm, ext, K, delta_pc=deltas, delta_index=list(range(V)))["rgb"]
        assert abs(float(v) - float(ssim_ref.loss64(imgs, targets))) <= 1e-6


def test_training_steps_on_render_loss_frames(cuda):
    from gvfdiffusion_amd.training import DeltaHead, render_loss_frames, train_step
    Pn, Sn, Tn, feat = 4000, 96, 3, 8
    attrs = synthetic.random_gaussians(Pn, sh_degree=0, seed=3, scale_lo=0.01, scale_hi=0.05)
    gm = synthetic.gaussian_model_from(attrs, 0, cuda)
    rend = _renderer(Sn)
    ext = torch.stack([synthetic.orbit_w2c(40.0 * f, 10.0) for f in range(Tn)]).to(cuda)
    K = synthetic.intrinsics().to(cuda)
    g = torch.Generator().manual_seed(0)
    feats = torch.randn((Tn, Pn, feat), generator=g).to(cuda)
    with torch.no_grad():
        true = DeltaHead(feat).to(cuda)
        true.to_outputs.weight.copy_(0.01 * torch.randn((14, feat), generator=g).to(cuda))
        targets = rend.render_frames(gm, ext, K, delta_pc=true(feats), delta_index=list(range(Tn)))["rgb"].clone()
    torch.manual_seed(1)
    h = DeltaHead(feat).to(cuda)
    with torch.no_grad():
        h.to_outputs.weight.copy_(0.005 * torch.randn((14, feat), device=cuda))
    params = list(h.parameters())
    opt = torch.optim.Adam(params, lr=2e-3)
    losses = []
    for _ in range(8):
        info = train_step(params, opt, lambda: render_loss_frames(rend, gm, ext, K, h(feats), targets), max_grad_norm=1.0)
        assert math.isfinite(info["loss"]) and math.isfinite(info["grad_norm"])
        losses.append(info["loss"])
    print("render loss (L1 + 0.2 (1 - SSIM)):", " ".join(f"{v:.5f}" for v in losses))
    assert losses[-1] < 0.9 * losses[0]
