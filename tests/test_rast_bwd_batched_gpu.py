"""Backward of the batched, fused-activation render (GaussianRenderer.render_frames -> _RasterizeBatchedFn -> gvf_rast_backward_batched) against
the single-frame path summed over frames, against the double oracle, over every record layout the forward can choose, and in a training step --
needs an MI355X."""
import math
import os

import numpy as np
import pytest
import torch

import oracle
from gvfdiffusion_amd import _lib, synthetic
from gvfdiffusion_amd import rasterizer as _r
from gvfdiffusion_amd.renderers import GaussianRenderer

pytestmark = pytest.mark.gpu
BG = (0.3, 0.3, 0.3)
RAW = ("_xyz", "_features_dc", "_scaling", "_rotation", "_opacity")


def rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.linalg.norm(a - b) / max(1e-30, np.linalg.norm(b)))


def _renderer(S):
    rend = GaussianRenderer({"resolution": S, "near": synthetic.NEAR, "far": synthetic.FAR, "ssaa": 1, "bg_color": BG})
    rend.pipe.use_mip_gaussian = True
    rend.pipe.kernel_size = synthetic.KERNEL_2D
    return rend


def _scene(P, deg, seed, n_slices, dev, scale_lo=0.004, scale_hi=0.04):
    a = synthetic.random_gaussians(P, sh_degree=deg, seed=seed, scale_lo=scale_lo, scale_hi=scale_hi)
    a["means3D"] = a["means3D"] * 0.8
    a["opacities"] = a["opacities"].clamp(0.02, 0.95)
    return a, synthetic.random_deltas(n_slices, P, seed=seed + 1, std=0.01).to(dev)


def _cams(F, dev):
    ext = torch.stack([synthetic.orbit_w2c(360.0 * f / F + 7.0, 10.0 - 3.0 * (f % 3)) for f in range(F)]).to(dev)
    return ext, synthetic.intrinsics().to(dev)


def _leaves(attrs, deg, dev, raw=True):
    gm = synthetic.gaussian_model_from(attrs, deg, dev)
    for k in RAW:
        setattr(gm, k, getattr(gm, k).detach().clone().contiguous().requires_grad_(raw))
    return gm


def _batched(attrs, deg, deltas, di, ext, K, wc, S, raw=True, **kw):
    """one render_frames + backward: (frames, {name: grad})"""
    gm = _leaves(attrs, deg, deltas.device, raw)
    d = deltas.clone().requires_grad_(True)
    out = _renderer(S).render_frames(gm, ext, K, delta_pc=d, delta_index=di, **kw)
    (out.rgb * wc).sum().backward()
    g = {k: getattr(gm, k).grad for k in RAW}
    g["delta"] = d.grad
    return out.rgb.detach(), g


def _per_frame(attrs, deg, deltas, di, ext, K, wc, S):
    """the single-frame path (torch activations -> _RasterizeFn), summed over the frames"""
    gm = _leaves(attrs, deg, deltas.device)
    d = deltas.clone().requires_grad_(True)
    rend = _renderer(S)
    for f in range(ext.shape[0]):
        out = rend.render(gm, ext[f], K, delta_pc=d[di[f]] if di[f] >= 0 else None)
        (out.rgb * wc[f]).sum().backward()
    g = {k: getattr(gm, k).grad for k in RAW}
    g["delta"] = d.grad
    return g


def _compare(ga, gb, bar, what):
    errs = {k: rel(ga[k].cpu().numpy(), gb[k].cpu().numpy()) for k in gb}
    print(what, " ".join(f"{k}={v:.1e}" for k, v in errs.items()))
    for k, v in errs.items():
        assert torch.isfinite(ga[k]).all(), k
        assert v <= bar, (what, k, v)
    return errs


def test_matches_the_per_frame_path(cuda):
    """F = 8 frames over 3 delta slices, two static frames: all six gradients of one batched backward against the sum of the
    single-frame backwards."""
    P, S, deg, F = 5000, 128, 2, 8
    attrs, deltas = _scene(P, deg, 11, 3, cuda)
    di = [0, 1, 2, 0, 1, 2, -1, -1]
    ext, K = _cams(F, cuda)
    wc = torch.randn((F, 3, S, S), generator=torch.Generator().manual_seed(5)).to(cuda)
    _, gb = _batched(attrs, deg, deltas, di, ext, K, wc, S)
    gp = _per_frame(attrs, deg, deltas, di, ext, K, wc, S)
    _compare(gb, gp, 1e-4, "batched vs per-frame:")


def test_matches_the_double_oracle(cuda):
    """The oracle backward per frame, chained through GaussianModel.get_*_with_delta under CPU autograd, summed over frames."""
    P, S, deg = 1500, 64, 1
    attrs, deltas = _scene(P, deg, 21, 2, cuda)
    di = [0, 1, -1]
    F = len(di)
    ext, K = _cams(F, cuda)
    wc = torch.randn((F, 3, S, S), generator=torch.Generator().manual_seed(6))
    _, gb = _batched(attrs, deg, deltas, di, ext, K, wc.to(cuda), S)
    from gvfdiffusion_amd.renderers.gaussian_render import _camera
    gmc = _leaves(attrs, deg, torch.device("cpu"))
    dc = deltas.cpu().clone().requires_grad_(True)
    rend = _renderer(S)
    n = lambda t: t.detach().double().numpy()
    for f in range(F):
        cam = _camera(ext[f].cpu(), K.cpu(), synthetic.NEAR, synthetic.FAR, S)
        if di[f] >= 0:
            d = dc[di[f]]
            act = [gmc.get_xyz_with_delta(d[..., :3]), gmc.get_features_with_delta(d[..., 10:13].unsqueeze(1)),
                   gmc.get_opacity_with_delta(d[..., 13:]), gmc.get_scaling_with_delta(d[..., 3:6]), gmc.get_rotation_with_delta(d[..., 6:10])]
        else:
            act = [gmc.get_xyz, gmc.get_features, gmc.get_opacity, gmc.get_scaling, gmc.get_rotation]
        kw = dict(H=S, W=S, tanfovx=math.tan(float(cam.FoVx) * 0.5), tanfovy=math.tan(float(cam.FoVy) * 0.5),
                  kernel_size=float(rend.pipe.kernel_size), scale_modifier=1.0, viewmatrix=cam.world_view_transform.numpy(),
                  projmatrix=cam.full_proj_transform.numpy(), campos=cam.camera_center.numpy(), sh_degree=deg, bg=np.asarray(BG), mode=0)
        ref = oracle.rast64_backward(n(act[0]), n(act[1]), None, n(act[2]), n(act[3]), n(act[4]), None, n(wc[f]), **kw)
        gouts = [torch.tensor(ref[k].reshape(t.shape), dtype=torch.float32) for k, t in
                 zip(("means3D", "shs", "opacities", "scales", "rotations"), act)]
        torch.autograd.backward(act, gouts)
    gref = {k: getattr(gmc, k).grad for k in RAW}
    gref["delta"] = dc.grad
    _compare(gb, gref, 6e-6, "batched vs double oracle:")     # measured 1.6e-06 .. 3.0e-06 (_xyz, delta): twice the worst


def test_every_record_layout_gives_the_same_gradients(cuda, monkeypatch):
    """Shared activation + slot order (the default at F >= 2 x slices, P >= 4096), GVF_RAST_SHARED_ACT=0, GVF_RAST_SLOT_ORDER=0, radix
    binning: the backward reads the layout the forward recorded."""
    P, S, deg = 6000, 128, 2
    attrs, deltas = _scene(P, deg, 31, 2, cuda)
    di = [0] * 6 + [1] * 6 + [-1] * 4
    F = len(di)
    ext, K = _cams(F, cuda)
    wc = torch.randn((F, 3, S, S), generator=torch.Generator().manual_seed(7)).to(cuda)
    lib = _lib.lib()
    n0 = lib.gvf_rast_shared_activation_calls()
    frames0, g0 = _batched(attrs, deg, deltas, di, ext, K, wc, S)
    assert lib.gvf_rast_shared_activation_calls() > n0, "the shared-activation path did not run"
    variants = [("GVF_RAST_SHARED_ACT", "0", None), ("GVF_RAST_SLOT_ORDER", "0", None), (None, None, _lib.RAST_BIN_RADIX)]
    for env, val, algo in variants:
        with monkeypatch.context() as m:
            if env:
                m.setenv(env, val)
            if algo is not None:
                m.setattr(_r, "DEFAULT_BIN_ALGO", algo)
            n1 = lib.gvf_rast_shared_activation_calls()
            frames, g = _batched(attrs, deg, deltas, di, ext, K, wc, S)
            if env == "GVF_RAST_SLOT_ORDER":
                assert lib.gvf_rast_shared_activation_calls() > n1
            else:
                assert lib.gvf_rast_shared_activation_calls() == n1
        assert torch.equal(frames, frames0)
        _compare(g, g0, 1e-5, f"layout {env or 'bin_algo'}={val or algo}:")


def test_forward_is_unaffected_by_autograd(cuda, monkeypatch):
    P, S, deg = 3000, 96, 2
    attrs, deltas = _scene(P, deg, 41, 2, cuda)
    di = [0, 1, 0, 1, -1]
    ext, K = _cams(len(di), cuda)
    calls = []
    orig = _r._RasterizeBatchedFn.apply
    monkeypatch.setattr(_r._RasterizeBatchedFn, "apply", lambda *a: calls.append(1) or orig(*a))
    gm = _leaves(attrs, deg, cuda)
    d = deltas.clone().requires_grad_(True)
    out = _renderer(S).render_frames(gm, ext, K, delta_pc=d, delta_index=di)
    assert out.rgb.requires_grad and len(calls) == 1
    with torch.no_grad():
        ref = _renderer(S).render_frames(gm, ext, K, delta_pc=d, delta_index=di)
    assert len(calls) == 1, "a no-grad call went through the autograd Function (private workspace)"
    assert not ref.rgb.requires_grad
    assert torch.equal(out.rgb.detach(), ref.rgb)
    assert torch.equal(out.num_rendered, ref.num_rendered)
    with torch.no_grad():                                       # the uint8 entry point stays off the graph as well
        u8 = _renderer(S).render_frames(gm, ext, K, delta_pc=d, delta_index=di, as_uint8=True)
    assert u8.rgb.dtype == torch.uint8 and len(calls) == 1


def test_edge_cases(cuda):
    P, S, deg = 2500, 64, 1
    attrs, deltas = _scene(P, deg, 51, 4, cuda)
    di = [0, 2, 0, 2, -1]
    F = len(di)
    ext, K = _cams(F, cuda)
    wc = torch.randn((F, 3, S, S), generator=torch.Generator().manual_seed(9)).to(cuda)
    frames0, g0 = _batched(attrs, deg, deltas, di, ext, K, wc, S)
    # slices no frame selects: exact zeros; the selected ones carry gradient
    assert torch.count_nonzero(g0["delta"][1]) == 0 and torch.count_nonzero(g0["delta"][3]) == 0
    assert g0["delta"][0].abs().max() > 0 and g0["delta"][2].abs().max() > 0
    # detach_static: only the deltas require grad -> no raw gradients computed, the delta gradient unchanged
    _, gd = _batched(attrs, deg, deltas, di, ext, K, wc, S, raw=False)
    assert all(gd[k] is None for k in RAW)
    assert rel(gd["delta"].cpu().numpy(), g0["delta"].cpu().numpy()) <= 1e-5
    # an instance-count overflow of the first attempt: the differentiable call grows its workspace and retries
    key = (P, S, S, F)
    _r._CAP_HINT[key] = 1024
    frames1, g1 = _batched(attrs, deg, deltas, di, ext, K, wc, S)
    assert _r._CAP_HINT[key] > 1024
    assert torch.equal(frames1, frames0)
    _compare(g1, g0, 1e-5, "after the retry:")
    # P = 0: background frames, empty gradients
    act = synthetic.gaussian_model_from(attrs, deg, cuda).activation_struct()
    st = _r.make_settings(S, S, deg, _lib.RAST_MODE_MIP, synthetic.KERNEL_2D, 1.0, BG)
    fr = _renderer(S).make_frames(ext, K, [-1] * F)
    z = lambda *s: torch.zeros(s, device=cuda, requires_grad=True)
    leaves = [z(0, 3), z(0, (deg + 1) ** 2, 3), z(0, 3), z(0, 4), z(0, 1)]
    out = _r.rasterize_batched(st, fr, act, *leaves)
    out["color"].sum().backward()
    assert all(t.grad is not None and t.grad.numel() == 0 for t in leaves)
    assert torch.allclose(out["color"][:, 0], torch.full((F, S, S), BG[0], device=cuda))


def test_bench_shape_matches_the_per_frame_path(cuda):
    """P = 262 144 at 800 x 800, SH 2, 8 frames over 2 slices."""
    P, S, deg = 262_144, 800, 2
    attrs, deltas = _scene(P, deg, 61, 2, cuda, scale_lo=0.002, scale_hi=0.01)
    di = [0, 1] * 4
    F = len(di)
    ext, K = _cams(F, cuda)
    wc = torch.randn((F, 3, S, S), generator=torch.Generator().manual_seed(10)).to(cuda)
    _, gb = _batched(attrs, deg, deltas, di, ext, K, wc, S)
    gp = _per_frame(attrs, deg, deltas, di, ext, K, wc, S)
    _compare(gb, gp, 1e-4, "bench shape, batched vs per-frame:")


def test_training_steps_through_the_batched_backward(cuda):
    """A few train_steps of DeltaHead on render_l1_loss_frames lower the loss; the first step's gradients equal render_l1_loss's."""
    from gvfdiffusion_amd.training import DeltaHead, render_l1_loss, render_l1_loss_frames, train_step
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
        targets = torch.stack([rend.render(gm, ext[v], K, delta_pc=true(feats)[v]).rgb for v in range(Tn)])

    def head():
        torch.manual_seed(1)
        h = DeltaHead(feat).to(cuda)
        with torch.no_grad():
            h.to_outputs.weight.copy_(0.005 * torch.randn((14, feat), device=cuda))
        return h

    fn = lambda gaussian, e, k, d: rend.render(gaussian, e, k, delta_pc=d).rgb
    h1, h2 = head(), head()
    render_l1_loss(fn, gm, ext, K, h1(feats), targets).backward()
    render_l1_loss_frames(rend, gm, ext, K, h2(feats), targets).backward()
    for p1, p2 in zip(h1.parameters(), h2.parameters()):
        assert rel(p2.grad.cpu().numpy(), p1.grad.cpu().numpy()) <= 1e-4
    params = list(h2.parameters())
    opt = torch.optim.Adam(params, lr=2e-3)
    losses = []
    for _ in range(8):
        info = train_step(params, opt, lambda: render_l1_loss_frames(rend, gm, ext, K, h2(feats), targets), max_grad_norm=1.0)
        assert math.isfinite(info["loss"]) and math.isfinite(info["grad_norm"])
        losses.append(info["loss"])
    print("render-L1 loss (batched backward):", " ".join(f"{v:.5f}" for v in losses))
    assert losses[-1] < 0.9 * losses[0]
