"""The two workgroup mappings of the fused preprocess launch give the same bits -- needs an MI355X.

Bucket binning without shared activation runs preprocess_kernel<false, true> (rast_front.hip): a workgroup owns 64 consecutive Gaussians, stages their
SH rows once and its four waves walk different frames (wave w: frames 4 G by + w + 4 ff, G = PRE_WAVE_FB).  GVF_RAST_PRE_WAVE_FRAMES=0 puts the
call back on preprocess_kernel<false> (256 Gaussians per workgroup, four frames in turn), which the radix binning always takes.  Both run the
same per-Gaussian functions in the same order, so every output must be equal bit for bit.  The shapes are the smallest at which the mapping can
go wrong: a partial wave (P = 1), a partial quad of the quad-transposed record store (P = 63), one Gaussian past a workgroup (P = 65), several
workgroups with a tail (P = 300), a call with a Morton order (P = 5000 >= 4096, F >= 4); waves without a frame (F = 1, 3), F no multiple of 4
(F = 5, 9), a second blockIdx.y with two frames (F = 4 G + 2); SH staging spans of 768 B, 6912 B and 12 288 B (degree 0, 2, 3)."""
import os

import numpy as np
import pytest
import torch

from gvfdiffusion_amd import synthetic
from rast_util import camera_block, oracle_render, compare_images, cam_from_frame, oracle_activated

pytestmark = pytest.mark.gpu

PRE_WAVE_FB = 6                     # csrc/rast_plan.h: frames per wave of the wave-frames mapping, 4 * PRE_WAVE_FB per workgroup
KEYS = ("color", "alpha", "depth", "radii", "num_rendered")


def _scene(cuda, P, F, deg, seed):
    """F orbit cameras, every frame its own delta slice (the last one none): too many slices for the shared activation, so the call takes the
    fused launch."""
    from gvfdiffusion_amd import rasterizer as R
    attrs = synthetic.random_gaussians(P, sh_degree=deg, seed=seed, scale_lo=0.01, scale_hi=0.05)
    gm = synthetic.gaussian_model_from(attrs, deg, cuda)
    delta = synthetic.random_deltas(F, P, seed=seed + 1).to(cuda)
    idx = list(range(F))
    if F > 1:
        idx[-1] = -1
    cams = [camera_block(azi=29.0 * f, elev=3.0 * (f % 9) - 12.0) for f in range(F)]
    frames = [R.make_frame(c["viewmatrix"], c["projmatrix"], c["campos"], c["tanfovx"], c["tanfovy"], di) for c, di in zip(cams, idx)]
    return gm, delta, idx, frames


def _render(gm, delta, frames, S, deg, wave_frames, bin_algo=None):
    from gvfdiffusion_amd import rasterizer as R, _lib
    st = R.make_settings(S, S, deg, 0, synthetic.KERNEL_2D, 1.0, synthetic.BG, bin_algo=bin_algo)
    raw = [t.contiguous().float() for t in (gm._xyz, gm.get_features, gm._scaling, gm._rotation, gm._opacity.reshape(-1))]
    old = {k: os.environ.get(k) for k in ("GVF_RAST_PRE_WAVE_FRAMES", "GVF_RAST_SHARED_ACT")}
    os.environ["GVF_RAST_SHARED_ACT"] = "0"
    if wave_frames:
        os.environ.pop("GVF_RAST_PRE_WAVE_FRAMES", None)          # the default
    else:
        os.environ["GVF_RAST_PRE_WAVE_FRAMES"] = "0"
    try:
        before = int(_lib.lib().gvf_rast_shared_activation_calls())
        out = R.rasterize_batched(st, frames, gm.activation_struct(), *raw, delta=delta, want_alpha_depth=True, want_radii=True)
        torch.cuda.synchronize()
        assert int(_lib.lib().gvf_rast_shared_activation_calls()) == before, "the call did not take the fused launch"
        # the call plan (host only, same switches): the fused launch on the mapping the switch selects -- the radix binning always on the
        # 256-Gaussian one --, the index-ordered count pass (at most 64 tiles here) and, with a Morton order, the gathering bin passes
        P, bucket = gm._xyz.shape[0], st.bin_algo != _lib.RAST_BIN_RADIX
        plan = R.call_plan(st, frames, P, raw[1].shape[1], out["max_rendered"])
        assert plan.shared == 0 and plan.wave_frames == int(wave_frames and bucket) and plan.index_count == int(bucket)
        assert plan.rec_gather == plan.morton == int(bucket and len(frames) >= 4 and P >= 4096)
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
    return out


def _assert_same(a, b, what):
    for k in KEYS:
        assert torch.equal(a[k], b[k]), f"{what}: {k} differs"


@pytest.mark.parametrize("P,F,deg,S", [(1, 1, 0, 64), (63, 3, 2, 64), (65, 5, 3, 96), (300, 9, 2, 128),
                                       (5000, 4 * PRE_WAVE_FB + 2, 2, 128)])
def test_wave_frames_mapping_equals_block_mapping(cuda, oracle_lib, P, F, deg, S):
    gm, delta, idx, frames = _scene(cuda, P, F, deg, seed=100 + P)
    new = _render(gm, delta, frames, S, deg, wave_frames=True)
    old = _render(gm, delta, frames, S, deg, wave_frames=False)
    _assert_same(new, old, f"P={P} F={F} deg={deg}")
    assert new["radii"].shape == (F, P) and int(new["num_rendered"].sum()) > 0
    assert int((new["radii"] > 0).sum()) > 0 and float(new["color"].std()) > 0
    if P != 5000:
        return
    # not only against its sibling: frames of different waves (f % 4), loop trips (f // 4) and of the second blockIdx.y against the CPU oracle
    for f in (0, 5, 14, F - 1):
        oattrs = oracle_activated(oracle_lib, gm, None if idx[f] < 0 else delta[idx[f]])
        cam = cam_from_frame(frames[f])
        ref = oracle_render(oracle_lib, oattrs, cam, S, S, deg, mode=0)
        assert np.array_equal(new["radii"][f].cpu().numpy(), ref["radii"])
        compare_images(new["color"][f].cpu().numpy(), ref["color"], ref["flags"])
        # the operator's binning rule (pairs that cannot reach alpha 1/255 in the tile are dropped) restated by the oracle: exact counts
        assert int(new["num_rendered"][f]) == oracle_render(oracle_lib, oattrs, cam, S, S, deg, mode=0, tight=True)["num_rendered"]


def test_radix_binning_keeps_the_block_mapping(cuda):
    """The radix binning needs per-256-Gaussian block sums, i.e. preprocess_kernel<false>, whatever the switch says: the same outputs with the
    switch at 0 and at its default, and the bucket binning's images."""
    from gvfdiffusion_amd import _lib
    P, F, deg, S = 300, 9, 2, 128
    gm, delta, idx, frames = _scene(cuda, P, F, deg, seed=100 + P)
    radix = _render(gm, delta, frames, S, deg, wave_frames=True, bin_algo=_lib.RAST_BIN_RADIX)
    radix0 = _render(gm, delta, frames, S, deg, wave_frames=False, bin_algo=_lib.RAST_BIN_RADIX)
    bucket = _render(gm, delta, frames, S, deg, wave_frames=True, bin_algo=_lib.RAST_BIN_BUCKET)
    _assert_same(radix, radix0, "radix binning, switch at its default and at 0")
    _assert_same(radix, bucket, "radix and bucket binning")
    assert int(radix["num_rendered"].sum()) > 0
