"""Host side of the batched rasteriser backward (gvf_rast_backward_batched), no GPU: the library exports it, its scratch size, every argument
error it reports before touching the device, and training.render_l1_loss_frames == render_l1_loss on the double-precision CPU oracle."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
S, P, DEG, FEAT, T = 24, 60, 0, 5, 3


def _lib():
    from gvfdiffusion_amd import _lib
    return _lib


def test_library_exports_the_batched_backward():
    from gvfdiffusion_amd import _build
    lib = ctypes.CDLL(_build.LIB_PATH)
    assert hasattr(lib, "gvf_rast_backward_batched")
    assert hasattr(lib, "gvf_rast_backward_batched_scratch_bytes")
    assert "gvf_rast_backward_batched" in _lib().SIGNATURES


def _scratch(P, F):
    out = ctypes.c_size_t(0)
    assert _lib().lib().gvf_rast_backward_batched_scratch_bytes(P, F, ctypes.byref(out)) == 0
    return out.value


def test_scratch_grows_with_gaussians_and_frames():
    L = _lib()
    out = ctypes.c_size_t(0)
    assert _scratch(1000, 4) < _scratch(2000, 4) < _scratch(2000, 8)
    assert _scratch(262144, 24) >= 24 * 262144 * 10 * 4          # per-(frame, Gaussian) accumulators
    assert L.lib().gvf_rast_backward_batched_scratch_bytes(-1, 4, ctypes.byref(out)) == L.GVF_EINVAL
    assert L.lib().gvf_rast_backward_batched_scratch_bytes(10, 0, ctypes.byref(out)) == L.GVF_EINVAL


class _Call:
    """A well-formed argument set (fake but aligned device addresses: every case below is refused before the first HIP call)."""

    def __init__(self, P=100, F=3, H=32, W=32, deg=1, n_delta=2):
        L = _lib()
        self.L = L
        self.st = L.GvfRastSettings()
        self.st.image_height, self.st.image_width, self.st.sh_degree, self.st.mode = H, W, deg, L.RAST_MODE_MIP
        self.st.kernel_size, self.st.scale_modifier = 0.1, 1.0
        self.act = L.GvfGaussianActivation()
        self.act.scaling_activation = 1
        self.frames = (L.GvfRastFrame * F)()
        for f in range(F):
            self.frames[f].delta_index = f % n_delta if n_delta > 0 else -1
        self.F, self.P, self.M, self.n_delta = F, P, (deg + 1) ** 2, n_delta
        self.cap = 4096
        ws = ctypes.c_size_t(0)
        assert L.lib().gvf_rast_workspace_bytes(P, F, H, W, self.cap, ctypes.byref(ws)) == 0
        self.ws_bytes = ws.value
        self.scratch_bytes = _scratch(P, F)
        self.fake = ctypes.c_void_p(1 << 20)                     # 256-byte aligned, never dereferenced

    def run(self, **over):
        a = dict(st=ctypes.byref(self.st), frames=self.frames, F=self.F, act=ctypes.byref(self.act), P=self.P, M=self.M,
                 xyz=self.fake, fdc=self.fake, scal=self.fake, rot=self.fake, op=self.fake, delta=self.fake, n_delta=self.n_delta,
                 ws=self.fake, ws_bytes=self.ws_bytes, cap=self.cap, g_color=self.fake, g_alpha=None, g_depth=None,
                 scratch=self.fake, scratch_bytes=self.scratch_bytes)
        a.update(over)
        return self.L.lib().gvf_rast_backward_batched(
            a["st"], a["frames"], a["F"], a["act"], a["P"], a["M"], a["xyz"], a["fdc"], a["scal"], a["rot"], a["op"], a["delta"],
            a["n_delta"], a["ws"], a["ws_bytes"], a["cap"], a["g_color"], a["g_alpha"], a["g_depth"], a["scratch"], a["scratch_bytes"],
            self.fake, self.fake, self.fake, self.fake, self.fake, self.fake, None)


def test_argument_errors_are_reported_without_a_gpu():
    c = _Call()
    L = c.L
    assert c.run(g_color=None) == L.GVF_EINVAL
    assert c.run(F=0) == L.GVF_EINVAL
    assert c.run(F=-2) == L.GVF_EINVAL
    c.st.sh_degree = 4
    assert c.run() == L.GVF_EINVAL
    c.st.sh_degree = 1
    assert c.run(M=2) == L.GVF_EINVAL                           # fewer coefficients than the degree needs
    assert c.run(n_delta=0) == L.GVF_EINVAL                     # a frame selects slice 0 / 1
    assert c.run(delta=None) == L.GVF_EINVAL
    c.st.mode = L.RAST_MODE_DILATE                              # the batched backward is the mip path's
    assert c.run() == L.GVF_EINVAL
    c.st.mode = L.RAST_MODE_MIP
    assert c.run(scratch_bytes=c.scratch_bytes - 1) == L.GVF_ENOSPC
    assert c.run(scratch=None) == L.GVF_ENOSPC
    assert c.run(ws_bytes=c.ws_bytes // 2) == L.GVF_ENOSPC
    assert c.run(ws=ctypes.c_void_p((1 << 20) + 16)) == L.GVF_EINVAL   # the workspace is 256-byte aligned


def test_static_frames_need_no_delta():
    c = _Call(n_delta=0)
    L = c.L
    assert c.run(delta=None, scratch_bytes=c.scratch_bytes - 1) == L.GVF_ENOSPC   # valid up to the short scratch
    c2 = _Call(P=0)
    assert c2.run() == L.GVF_OK                                   # nothing to differentiate: no HIP call


# ---- render_l1_loss_frames == render_l1_loss on the CPU oracle (copied from tests/test_training_step.py's pattern)

def _scene(sample):
    from gvfdiffusion_amd import synthetic
    a = synthetic.random_gaussians(P, sh_degree=DEG, seed=40 + sample, scale_lo=0.02, scale_hi=0.08)
    a["means3D"] = a["means3D"] * 0.6
    a["opacities"] = a["opacities"].clamp(0.05, 0.9)
    g = torch.Generator().manual_seed(70 + sample)
    feats = torch.randn((T, P, FEAT), generator=g, dtype=torch.float64)
    targets = torch.rand((4, 3, S, S), generator=g, dtype=torch.float64)
    return a, feats, targets


class _OracleRasterize(torch.autograd.Function):
    """The rasteriser operator on the CPU oracle (double precision): forward gvfo64_forward, backward gvfo64_backward."""

    @staticmethod
    def forward(ctx, means3D, shs, opacities, scales, rotations, kw):
        import oracle
        n = lambda t: t.detach().double().numpy()
        out = oracle.rast64_forward(n(means3D), n(shs), None, n(opacities).reshape(-1), n(scales), n(rotations), None, mode=0, **kw)
        ctx.save_for_backward(means3D, shs, opacities, scales, rotations)
        ctx.kw = kw
        return torch.from_numpy(out["color"])

    @staticmethod
    def backward(ctx, g_color):
        import oracle
        means3D, shs, opacities, scales, rotations = ctx.saved_tensors
        n = lambda t: t.detach().double().numpy()
        g = oracle.rast64_backward(n(means3D), n(shs), None, n(opacities).reshape(-1), n(scales), n(rotations), None,
                                   g_color.double().numpy(), mode=0, **ctx.kw)
        f = lambda k, like: torch.from_numpy(g[k]).reshape(like.shape).to(like.dtype)
        return f("means3D", means3D), f("shs", shs), f("opacities", opacities), f("scales", scales), f("rotations", rotations), None


def _oracle_render_fn(attrs):
    """render_fn(gaussian, azimuth, intrinsics, delta): the (P,14) delta applied with torch ops, then the oracle operator."""
    from gvfdiffusion_amd import synthetic
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from rast_util import camera_block

    def fn(gaussian, azimuth, _intr, delta):
        cam = camera_block(azi=float(azimuth), elev=10.0)
        kw = dict(H=S, W=S, tanfovx=cam["tanfovx"], tanfovy=cam["tanfovy"], kernel_size=synthetic.KERNEL_2D, scale_modifier=1.0,
                  viewmatrix=cam["viewmatrix"].numpy(), projmatrix=cam["projmatrix"].numpy(), campos=cam["campos"].numpy(),
                  sh_degree=DEG, bg=np.asarray([1.0, 1.0, 1.0]))
        a = {k: v.double() for k, v in gaussian.items()}
        means = a["means3D"] + delta[:, :3]
        scales = a["scales"] * torch.exp(delta[:, 3:6])
        rots = torch.nn.functional.normalize(a["rotations"] + delta[:, 6:10], dim=1)
        shs = a["shs"] + delta[:, 10:13].unsqueeze(1)
        opac = torch.sigmoid(torch.logit(a["opacities"]) + delta[:, 13:])
        return _OracleRasterize.apply(means, shs, opac, scales, rots, kw)
    return fn


class _StackingRenderer:
    """Stand-in for GaussianRenderer: render_frames stacks the per-view oracle renders (slice delta_index[v] for view v)."""

    def __init__(self, attrs):
        self.fn = _oracle_render_fn(attrs)
        self.calls = 0

    def render_frames(self, gaussian, extrinsics, intrinsics, delta_pc=None, delta_index=None):
        self.calls += 1
        imgs = [self.fn(gaussian, extrinsics[v], intrinsics, delta_pc[delta_index[v]]) for v in range(extrinsics.shape[0])]
        return {"rgb": torch.stack(imgs)}


def _head(seed=0):
    from gvfdiffusion_amd.training import DeltaHead
    torch.manual_seed(seed)
    h = DeltaHead(FEAT).double()
    with torch.no_grad():                                  # non-zero start so that every delta channel carries gradient
        h.to_outputs.weight.copy_(0.02 * torch.randn(14, FEAT, dtype=torch.float64))
    return h


@pytest.mark.parametrize("frame_of_view", [None, [2, 0, 2, 1]])
def test_render_l1_loss_frames_equals_render_l1_loss_on_the_oracle(frame_of_view):
    sys.path.insert(0, ROOT)
    from gvfdiffusion_amd.training import render_l1_loss, render_l1_loss_frames
    a, feats, targets = _scene(0)
    V = 3 if frame_of_view is None else len(frame_of_view)
    az = torch.tensor([15.0, 75.0, 140.0, 230.0])[:V]
    targets = targets[:V]
    h1, h2 = _head(), _head()
    l1 = render_l1_loss(_oracle_render_fn(a), a, az, None, h1(feats), targets, frame_of_view)
    rend = _StackingRenderer(a)
    l2 = render_l1_loss_frames(rend, a, az, None, h2(feats), targets, frame_of_view)
    assert rend.calls == 1                                  # all views in one render_frames call
    l1.backward()
    l2.backward()
    assert abs(float(l1.detach()) - float(l2.detach())) <= 1e-12 * max(1.0, abs(float(l1.detach())))
    for p1, p2 in zip(h1.parameters(), h2.parameters()):
        assert p1.grad.abs().max() > 1e-8
        assert torch.allclose(p1.grad, p2.grad, rtol=1e-10, atol=1e-14)
