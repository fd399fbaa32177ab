"""Bucket binning of the fused launch on a Morton-hostile sample -- needs an MI355X.

The fused launch (preprocess_kernel<false>) stores its bin records at the Gaussians' own indices and bins them in index order when a frame's
tiles fit the whole-frame table (rast_front.hip, bin_index_kernel), over Morton slots otherwise; the shared-activation launch keeps its Morton-slot
layout.  A spatially presorted sample and a random permutation of it must give the same instance counts per frame, and on each of them the
fused path must give the shared path's bits (same per-tile key sets -> same sorted lists -> same images)."""
import os

import pytest
import torch

from gvfdiffusion_amd import synthetic
from rast_util import camera_block

pytestmark = pytest.mark.gpu


def _morton_order(xyz):
    q = ((xyz - xyz.min(0).values) / (xyz.max(0).values - xyz.min(0).values).clamp_min(1e-30) * 1023).long().clamp(0, 1023)
    code = torch.zeros(xyz.shape[0], dtype=torch.long)
    for b in range(10):
        for k in range(3):
            code |= ((q[:, k] >> b) & 1) << (3 * b + k)
    return torch.argsort(code, stable=True)


def _render(cuda, attrs, delta, S, deg, shared):
    from gvfdiffusion_amd import rasterizer as R, _lib
    gm = synthetic.gaussian_model_from(attrs, deg, cuda)
    idx = [0, 0, 0, 1, 1, 1, 0, 1]                                # two slices over eight frames: shared activation when allowed
    cams = [camera_block(azi=41.0 * f, elev=5.0 * f - 12.0) for f in range(len(idx))]
    frames = [R.make_frame(c["viewmatrix"], c["projmatrix"], c["campos"], c["tanfovx"], c["tanfovy"], di) for c, di in zip(cams, idx)]
    st = R.make_settings(S, S, deg, 0, synthetic.KERNEL_2D, 1.0, synthetic.BG)
    raw = [t.contiguous().float() for t in (gm._xyz, gm.get_features, gm._scaling, gm._rotation, gm._opacity.reshape(-1))]
    old = os.environ.get("GVF_RAST_SHARED_ACT")
    os.environ["GVF_RAST_SHARED_ACT"] = "1" if shared else "0"
    try:
        before = int(_lib.lib().gvf_rast_shared_activation_calls())
        out = R.rasterize_batched(st, frames, gm.activation_struct(), *raw, delta=delta, want_alpha_depth=True, want_radii=True)
        torch.cuda.synchronize()
        n_shared = int(_lib.lib().gvf_rast_shared_activation_calls()) - before
        # the call plan (host only, same switches): shared activation in slot order, or the fused wave-frames launch with records at the
        # Gaussians' indices -- counted in index order when the frame's tiles fit the table (256 x 256), gathered in Morton order
        plan = R.call_plan(st, frames, attrs["means3D"].shape[0], raw[1].shape[1], out["max_rendered"])
        assert plan.shared == plan.slot_mode == int(shared) and plan.morton == 1
        assert plan.wave_frames == plan.rec_gather == int(not shared) and plan.index_count == int(not shared and S == 256)
    finally:
        if old is None:
            os.environ.pop("GVF_RAST_SHARED_ACT", None)
        else:
            os.environ["GVF_RAST_SHARED_ACT"] = old
    assert (n_shared >= 1) == shared
    return out


# 256 x 256: 256 tiles (index-order binning); 1088 x 1088: 4624 tiles, more than the whole-frame table holds (Morton-slot binning)
@pytest.mark.parametrize("S", [256, 1088])
def test_fused_binning_equals_shared_on_permuted_sample(cuda, S):
    P, deg = 40_000, 1
    attrs = synthetic.random_gaussians(P, sh_degree=deg, seed=23, scale_lo=0.003, scale_hi=0.03)
    delta = synthetic.random_deltas(2, P, seed=31)
    pre = _morton_order(attrs["means3D"])
    perm = torch.randperm(P, generator=torch.Generator().manual_seed(77))
    presorted = {k: v[pre] for k, v in attrs.items()}
    hostile = {k: v[perm] for k, v in presorted.items()}
    d_pre = delta[:, pre].contiguous()
    d_host = d_pre[:, perm].contiguous()
    counts = []
    for a, d, name in ((presorted, d_pre, "presorted"), (hostile, d_host, "permuted")):
        fused = _render(cuda, a, d.to(cuda), S, deg, shared=False)
        shared = _render(cuda, a, d.to(cuda), S, deg, shared=True)
        for k in ("color", "alpha", "depth", "radii", "num_rendered"):
            assert torch.equal(fused[k], shared[k]), f"{name} sample, {k}: fused path differs from the shared-activation path"
        assert int(fused["num_rendered"].sum()) > 0 and float(fused["color"].std()) > 0
        counts.append(fused)
    # the same Gaussians in another order: the same instances per frame, the same radius per Gaussian
    assert torch.equal(counts[0]["num_rendered"], counts[1]["num_rendered"])
    assert torch.equal(counts[0]["radii"][:, perm], counts[1]["radii"])
