"""Parity of the HIP rasteriser (through the C ABI) against the CPU oracle -- needs an MI355X."""
import os

import numpy as np
import pytest
import torch

from gvfdiffusion_amd import synthetic
from rast_util import camera_block, oracle_render, compare_images, RAST_ATOL, cam_from_frame, oracle_activated, cached

pytestmark = pytest.mark.gpu


def _to(dev, attrs):
    return {k: v.to(dev) for k, v in attrs.items()}


def _settings(cam, H, W, deg, mode, dev, kernel_size=synthetic.KERNEL_2D, scale_modifier=1.0, bg=synthetic.BG,
              subpixel_offset=None):
    common = dict(image_height=H, image_width=W, tanfovx=cam["tanfovx"], tanfovy=cam["tanfovy"],
                  bg=torch.tensor(bg, device=dev), scale_modifier=scale_modifier, viewmatrix=cam["viewmatrix"].to(dev),
                  projmatrix=cam["projmatrix"].to(dev), sh_degree=deg, campos=cam["campos"].to(dev), prefiltered=False,
                  debug=False)
    if mode == 0:
        from gvfdiffusion_amd.diff_gaussian_rasterization import GaussianRasterizationSettings, GaussianRasterizer
        return GaussianRasterizer(GaussianRasterizationSettings(kernel_size=kernel_size, subpixel_offset=subpixel_offset,
                                                                **common))
    from gvfdiffusion_amd.diff_gauss import GaussianRasterizationSettings, GaussianRasterizer
    return GaussianRasterizer(GaussianRasterizationSettings(**common))


@pytest.fixture(autouse=True, params=["bucket", "radix"])
def bin_algo(request):
    """Every test of this file runs with both instance-binning algorithms (include/gvf_rast.h GVF_RAST_BIN_*)."""
    from gvfdiffusion_amd import rasterizer as R, _lib
    old = R.DEFAULT_BIN_ALGO
    R.DEFAULT_BIN_ALGO = _lib.RAST_BIN_BUCKET if request.param == "bucket" else _lib.RAST_BIN_RADIX
    yield request.param
    R.DEFAULT_BIN_ALGO = old


def _run(rast, a, **over):
    kw = dict(means3D=a["means3D"], means2D=torch.zeros_like(a["means3D"]), shs=a["shs"], colors_precomp=None,
              opacities=a["opacities"], scales=a["scales"], rotations=a["rotations"], cov3D_precomp=None)
    kw.update(over)
    return rast(**kw)


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("deg", [0, 1, 2, 3])
@pytest.mark.parametrize("hw", [(256, 256), (200, 312)])
def test_frame_matches_oracle(cuda, oracle_lib, mode, deg, hw):
    H, W = hw
    attrs = synthetic.random_gaussians(20_000, sh_degree=deg, seed=11 + deg, scale_lo=0.003, scale_hi=0.03)
    cam = camera_block(azi=40.0 * deg + 5, elev=12.0)
    ref = oracle_render(oracle_lib, attrs, cam, H, W, deg, mode=mode)
    ret = _run(_settings(cam, H, W, deg, mode, cuda), _to(cuda, attrs))
    if mode == 0:
        assert len(ret) == 2
        color, radii = ret
    else:
        assert len(ret) == 6
        color, depth, normal, alpha, radii, extra = ret
        assert depth.shape == (1, H, W) and alpha.shape == (1, H, W)
        compare_images(alpha[0].cpu().numpy(), ref["alpha"], ref["flags"])
        compare_images(depth[0].cpu().numpy(), ref["depth"], ref["flags"], atol=2e-3, flagged_atol=2e-3, flip_atol=5e-2)
    assert color.shape == (3, H, W) and radii.dtype == torch.int32
    # integer work is bit-exact: radii (hence tile rects and the instance count)
    assert np.array_equal(radii.cpu().numpy(), ref["radii"])
    e_clean, e_flag, frac = compare_images(color.cpu().numpy(), ref["color"], ref["flags"])
    print(f"mode={mode} deg={deg} {H}x{W}: max|d|={e_clean:.2e} flagged={frac:.4f} (max {e_flag:.2e})")


def test_instance_count_and_empty_inputs(cuda, oracle_lib):
    from gvfdiffusion_amd import rasterizer as R, _lib
    cam = camera_block()
    attrs = synthetic.random_gaussians(5000, sh_degree=2, seed=2)
    ref = oracle_render(oracle_lib, attrs, cam, 128, 128, 2)
    a = _to(cuda, attrs)
    st = R.make_settings(128, 128, 2, 0, synthetic.KERNEL_2D, 1.0, synthetic.BG)
    fr = R.make_frame(cam["viewmatrix"], cam["projmatrix"], cam["campos"], cam["tanfovx"], cam["tanfovy"])
    out = R.rasterize(st, fr, a["means3D"], a["opacities"], shs=a["shs"], scales=a["scales"], rotations=a["rotations"])
    # default binning drops (Gaussian, tile) pairs that cannot reach alpha 1/255 in the tile; the oracle restates the
    # rule (tight=True) and the counts agree exactly; upstream_binning=True reproduces upstream's count, same image
    tight = oracle_render(oracle_lib, attrs, cam, 128, 128, 2, tight=True)
    assert out["num_rendered"] == tight["num_rendered"] < ref["num_rendered"]
    st_up = R.make_settings(128, 128, 2, 0, synthetic.KERNEL_2D, 1.0, synthetic.BG, upstream_binning=True)
    up = R.rasterize(st_up, fr, a["means3D"], a["opacities"], shs=a["shs"], scales=a["scales"], rotations=a["rotations"])
    assert up["num_rendered"] == ref["num_rendered"]
    assert torch.equal(up["color"], out["color"]) and torch.equal(up["radii"], out["radii"])
    # P = 0 -> background only
    e = {k: v[:0] for k, v in a.items()}
    out = R.rasterize(st, fr, e["means3D"], e["opacities"], shs=e["shs"], scales=e["scales"], rotations=e["rotations"])
    assert out["num_rendered"] == 0 and torch.all(out["color"] == 1.0)
    # everything behind the camera -> background only, radii 0
    b = dict(a)
    b["means3D"] = a["means3D"] * 0 + torch.tensor([0.0, -5.0, 0.0], device=cuda)
    out = R.rasterize(st, fr, b["means3D"], b["opacities"], shs=b["shs"], scales=b["scales"], rotations=b["rotations"])
    assert out["num_rendered"] == 0 and torch.all(out["radii"] == 0) and torch.all(out["color"] == 1.0)
    # argument contract of the upstream wrapper
    with pytest.raises(Exception):
        R.rasterize(st, fr, a["means3D"], a["opacities"], shs=a["shs"], colors_precomp=a["means3D"], scales=a["scales"],
                    rotations=a["rotations"])
    with pytest.raises(Exception):
        R.rasterize(st, fr, a["means3D"], a["opacities"], shs=a["shs"])
    with pytest.raises(_lib.GvfError):
        R.rasterize(st, fr, a["means3D"].cpu(), a["opacities"].cpu(), shs=a["shs"].cpu(), scales=a["scales"].cpu(),
                    rotations=a["rotations"].cpu())


def test_workspace_overflow_is_reported_and_retried(cuda, oracle_lib):
    from gvfdiffusion_amd import rasterizer as R
    cam = camera_block()
    attrs = synthetic.random_gaussians(3000, sh_degree=0, seed=4, scale_lo=0.02, scale_hi=0.06)
    ref = oracle_render(oracle_lib, attrs, cam, 160, 160, 0, tight=True)
    a = _to(cuda, attrs)
    st = R.make_settings(160, 160, 0, 0, synthetic.KERNEL_2D, 1.0, synthetic.BG)
    fr = R.make_frame(cam["viewmatrix"], cam["projmatrix"], cam["campos"], cam["tanfovx"], cam["tanfovy"])
    R._CAP_HINT[(3000, 160, 160, 1)] = 128   # force an undersized first attempt
    out = R.rasterize(st, fr, a["means3D"], a["opacities"], shs=a["shs"], scales=a["scales"], rotations=a["rotations"])
    assert out["num_rendered"] == ref["num_rendered"] > 128
    compare_images(out["color"].cpu().numpy(), ref["color"], ref["flags"])


def test_precomputed_colour_cov_and_subpixel(cuda, oracle_lib):
    H = W = 192
    attrs = synthetic.random_gaussians(8000, sh_degree=1, seed=21, scale_lo=0.004, scale_hi=0.03)
    cam = camera_block(azi=200.0, elev=-15.0)
    a = _to(cuda, attrs)
    g = torch.Generator().manual_seed(0)
    colors = torch.rand((8000, 3), generator=g)
    from gvfdiffusion_amd.representations.gaussian import build_scaling_rotation, strip_symmetric
    L = build_scaling_rotation(attrs["scales"], attrs["rotations"])
    cov = strip_symmetric(L @ L.transpose(1, 2)).contiguous()
    sub = (torch.rand((H, W, 2), generator=g) - 0.5)
    ref = oracle_render(oracle_lib, attrs, cam, H, W, 1, mode=0, colors_precomp=colors, cov3D_precomp=cov,
                        subpixel_offset=sub)
    rast = _settings(cam, H, W, 1, 0, cuda, subpixel_offset=sub.to(cuda))
    color, radii = _run(rast, a, shs=None, colors_precomp=colors.to(cuda), scales=None, rotations=None,
                        cov3D_precomp=cov.to(cuda))
    assert np.array_equal(radii.cpu().numpy(), ref["radii"])
    compare_images(color.cpu().numpy(), ref["color"], ref["flags"])
    # scale_modifier applied inside the operator
    ref2 = oracle_render(oracle_lib, attrs, cam, H, W, 1, mode=0, colors_precomp=colors, scale_modifier=1.3)
    rast2 = _settings(cam, H, W, 1, 0, cuda, scale_modifier=1.3)
    color2, radii2 = _run(rast2, a, shs=None, colors_precomp=colors.to(cuda))
    assert np.array_equal(radii2.cpu().numpy(), ref2["radii"])
    compare_images(color2.cpu().numpy(), ref2["color"], ref2["flags"])


@pytest.mark.parametrize("n,end_bit", [(0, 64), (1, 64), (63, 40), (4095, 44), (4097, 44), (100_003, 48),
                                      (3_000_000, 44), (5_000_000, 64)])
def test_radix_sort_is_stable_and_exact(cuda, n, end_bit):
    from gvfdiffusion_amd.rasterizer import sort_pairs_u64
    g = torch.Generator().manual_seed(n + end_bit)
    if n:
        hi = torch.randint(0, 1 << 12, (n,), generator=g, dtype=torch.int64)  # duplicate keys -> stability matters
        lo = torch.randint(0, 1 << 8, (n,), generator=g, dtype=torch.int64)
        keys = (hi << (end_bit - 13)) | (lo << 5) | 1
    else:
        keys = torch.zeros((0,), dtype=torch.int64)
    vals = torch.arange(n, dtype=torch.int32)
    k, v = sort_pairs_u64(keys.to(cuda), vals.to(cuda), end_bit)
    order = torch.sort(keys, stable=True).indices
    assert torch.equal(k.cpu(), keys[order])
    assert torch.equal(v.cpu(), vals[order])


def test_activation_kernel_matches_oracle(cuda, oracle_lib):
    from gvfdiffusion_amd import rasterizer as R
    P, M = 10_000, 4
    g = torch.Generator().manual_seed(9)
    raw = dict(xyz=torch.rand((P, 3), generator=g), feat=torch.randn((P, M, 3), generator=g),
               scaling=torch.randn((P, 3), generator=g) * 2, rot=torch.randn((P, 4), generator=g),
               opacity=torch.randn((P, 1), generator=g) * 3, delta=torch.randn((P, 14), generator=g) * 0.1)
    raw["scaling"][0, 0] = 30.0
    for act_name in ("softplus", "exp"):
        gm = synthetic.GaussianModel(sh_degree=1, mininum_kernel_size=0.0009, scaling_bias=0.004, opacity_bias=0.1,
                                     scaling_activation=act_name, device="cpu")
        act = gm.activation_struct()
        for delta in (raw["delta"], None):
            out = R.gaussian_activate(act, raw["xyz"].to(cuda), raw["feat"].to(cuda), raw["scaling"].to(cuda),
                                      raw["rot"].to(cuda), raw["opacity"].to(cuda),
                                      None if delta is None else delta.to(cuda))
            ref = oracle_lib.gaussian_activate(raw["xyz"].numpy(), raw["feat"].numpy(), raw["scaling"].numpy(),
                                               raw["rot"].numpy(), raw["opacity"].numpy(),
                                               None if delta is None else delta.numpy(), aabb=[-0.5, -0.5, -0.5, 1, 1, 1],
                                               scale_bias=act.scale_bias, opacity_bias=act.opacity_bias,
                                               min_kernel_size=0.0009, scaling_activation=act.scaling_activation)
            # everything is bit-exact -- exp / log1p included since round 6: csrc/rast_common.h and oracle/rast_oracle.c evaluate ONE operation
            # sequence (act_expf / act_log1pf; up to round 5 two different libms, relative 2e-6)
            for k in ("means3D", "rotations", "shs", "scales"):
                assert np.array_equal(out[k].cpu().numpy(), ref[k]), k
            assert np.array_equal(out["opacities"].cpu().numpy().reshape(-1), ref["opacities"])


def test_batched_fused_path_equals_per_frame_operator(cuda, oracle_lib):
    """render_frames (F frames, activations + deltas fused into the preprocess kernel) must be
    bit-identical to activate-kernel + single-frame operator, and match the oracle."""
    from gvfdiffusion_amd.renderers import GaussianRenderer
    from gvfdiffusion_amd import rasterizer as R
    P, deg, S, T = 30_000, 2, 208, 3
    attrs = synthetic.random_gaussians(P, sh_degree=deg, seed=31, scale_lo=0.003, scale_hi=0.02)
    gm = synthetic.gaussian_model_from(attrs, deg, cuda)
    delta = synthetic.random_deltas(T, P, seed=5).to(cuda)
    n = lambda t: t.detach().cpu().numpy()
    for use_mip in (True, False):
        rend = GaussianRenderer({"resolution": S, "near": synthetic.NEAR, "far": synthetic.FAR, "bg_color": synthetic.BG})
        rend.pipe.use_mip_gaussian = use_mip
        cams = [camera_block(azi=15.0 * f, elev=5.0) for f in range(4)]
        ext = torch.stack([c["extrinsics"] for c in cams]).to(cuda)
        K = cams[0]["intrinsics"].to(cuda)
        idx = [0, 1, 2, -1]
        out = rend.render_frames(gm, ext, K, delta_pc=delta, delta_index=idx, want_alpha_depth=True)
        assert out.rgb.shape == (4, 3, S, S)
        for f in range(4):
            d = None if idx[f] < 0 else delta[idx[f]]
            single = rend.render(gm, ext[f], K, delta_pc=d)          # torch activations -> operator
            act = R.gaussian_activate(gm.activation_struct(), gm._xyz, gm.get_features, gm._scaling, gm._rotation,
                                      gm._opacity, d)
            st = R.make_settings(S, S, deg, 0 if use_mip else 1, rend.pipe.kernel_size, 1.0, synthetic.BG)
            fr = rend.make_frames(ext[f:f + 1], K)[0]                # the same camera block render_frames used
            two = R.rasterize(st, fr, act["means3D"], act["opacities"], shs=act["shs"], scales=act["scales"],
                              rotations=act["rotations"], want_alpha_depth=True)
            dmax = float((out.rgb[f] - two["color"]).abs().max())
            assert dmax == 0.0, f"mip={use_mip} frame {f}: fused vs two-step differ by {dmax}"  # bit-exact
            assert torch.equal(out.alpha[f], two["alpha"]) and torch.equal(out.depth[f], two["depth"])
            assert int(out.num_rendered[f]) == two["num_rendered"]
            # vs the torch-activated facade path (different exp/log implementations): close
            assert (single.rgb - out.rgb[f]).abs().max() < 2e-2
            # vs the oracle (activations + render on the CPU)
            oa = oracle_lib.gaussian_activate(n(gm._xyz), n(gm.get_features), n(gm._scaling), n(gm._rotation),
                                              n(gm._opacity), None if d is None else n(d),
                                              aabb=[-0.5, -0.5, -0.5, 1, 1, 1], scale_bias=float(gm.scale_bias),
                                              opacity_bias=float(gm.opacity_bias),
                                              min_kernel_size=synthetic.KERNEL_3D, scaling_activation=1)
            oattrs = {k: torch.from_numpy(oa[k]) for k in ("means3D", "scales", "rotations", "shs")}
            oattrs["opacities"] = torch.from_numpy(oa["opacities"])
            ref = oracle_render(oracle_lib, oattrs, cams[f], S, S, deg, mode=0 if use_mip else 1,
                                kernel_size=rend.pipe.kernel_size)
            # one activation arithmetic on both sides (round 6): the same rule as test_frame_matches_oracle -- every unflagged pixel <= 1e-3 --
            # and the instance count of upstream's binning (the oracle's default) equals the operator's with upstream_binning
            compare_images(n(out.rgb[f]), ref["color"], ref["flags"])


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("deg", [0, 2])
def test_shared_activation_equals_fused_path(cuda, mode, deg, bin_algo):
    """Frames of one call that select the same delta slice (the reference's loop: 128 cameras per timestep,
    utils/inference_utils.py:256-269) share ONE activation + 3-D covariance per (slice, Gaussian) (activate_cov_kernel ->
    preprocess_kernel<true>); every output must be the bits of the per-frame fused path (GVF_RAST_SHARED_ACT=0)."""
    from gvfdiffusion_amd import rasterizer as R, _lib
    # 9 frames x 256 tiles: enough workgroups for the heaviest-first blend order too; P = 30 003: the last quad of lanes of the quad-transposed
    # record store is partly past P
    P, S = 30_000 + 3 * (deg == 2), 256
    attrs = synthetic.random_gaussians(P, sh_degree=deg, seed=41 + deg, scale_lo=0.003, scale_hi=0.02)
    gm = synthetic.gaussian_model_from(attrs, deg, cuda)
    delta = synthetic.random_deltas(3, P, seed=9).to(cuda)
    idx = [0, 0, 0, 2, 2, -1, -1, 0, 2]                       # three slices (delta 0, delta 2, none) over nine frames
    cams = [camera_block(azi=37.0 * f, elev=4.0 * f - 10.0) for f in range(len(idx))]
    frames = [R.make_frame(c["viewmatrix"], c["projmatrix"], c["campos"], c["tanfovx"], c["tanfovy"], di) for c, di in zip(cams, idx)]
    st = R.make_settings(S, S, deg, mode, synthetic.KERNEL_2D, 1.0, synthetic.BG)
    raw = [t.contiguous().float() for t in (gm._xyz, gm.get_features, gm._scaling, gm._rotation, gm._opacity.reshape(-1))]
    act = gm.activation_struct()

    def run():
        before = int(_lib.lib().gvf_rast_shared_activation_calls())
        out = R.rasterize_batched(st, frames, act, *raw, delta=delta, want_alpha_depth=True, want_radii=True)
        torch.cuda.synchronize()
        took = int(_lib.lib().gvf_rast_shared_activation_calls()) - before
        # the call plan (host only, same switches) says the same as the counter
        assert bool(R.call_plan(st, frames, P, raw[1].shape[1], out["max_rendered"]).shared) == (took >= 1)
        return out, took

    old_env = os.environ.get("GVF_RAST_SHARED_ACT")
    try:
        os.environ["GVF_RAST_SHARED_ACT"] = "0"
        fused, n0 = run()
        os.environ["GVF_RAST_SHARED_ACT"] = "1"
        shared, n1 = run()
    finally:
        if old_env is None:
            os.environ.pop("GVF_RAST_SHARED_ACT", None)
        else:
            os.environ["GVF_RAST_SHARED_ACT"] = old_env
    assert n0 == 0
    # the radix binning keeps its buffers (the records live in one of them): per-frame form there
    assert (n1 >= 1) == (bin_algo == "bucket"), (n1, bin_algo)
    for k in ("color", "alpha", "depth", "radii", "num_rendered"):
        assert torch.equal(fused[k], shared[k]), f"{k}: shared activation differs from the fused path"
    assert int(shared["num_rendered"].sum()) > 0 and float(shared["color"].std()) > 0
    # shared activation in INDEX order (the default runs the per-frame launch over Morton slots when the call has a Morton order: records,
    # splat records and bin records contiguous, the blend looking the record index up per Gaussian id): the same bits again
    os.environ["GVF_RAST_SLOT_ORDER"] = "0"
    try:
        index_order, n2 = run()
    finally:
        os.environ.pop("GVF_RAST_SLOT_ORDER", None)
    assert (n2 >= 1) == (bin_algo == "bucket")
    for k in ("color", "alpha", "depth", "radii", "num_rendered"):
        assert torch.equal(index_order[k], shared[k]), f"{k}: slot order differs from index order"
    # the blend's dispatch order (heaviest tiles of a frame first, blend_order_kernel) is invisible in the outputs
    os.environ["GVF_RAST_BLEND_ORDER"] = "0"
    try:
        image_order, _ = run()
    finally:
        os.environ.pop("GVF_RAST_BLEND_ORDER", None)
    for k in ("color", "alpha", "depth", "radii", "num_rendered"):
        assert torch.equal(image_order[k], shared[k]), f"{k}: depends on the blend's dispatch order"
    # four distinct slices for four frames: not worth a second launch, the call stays fused
    before = int(_lib.lib().gvf_rast_shared_activation_calls())
    four = [R.make_frame(c["viewmatrix"], c["projmatrix"], c["campos"], c["tanfovx"], c["tanfovy"], di) for c, di in zip(cams, [0, 1, 2, -1])]
    out4 = R.rasterize_batched(st, four, act, *raw, delta=delta)
    assert int(_lib.lib().gvf_rast_shared_activation_calls()) == before
    plan4 = R.call_plan(st, four, P, raw[1].shape[1], out4["max_rendered"])
    assert plan4.shared == 0 and plan4.n_slices == 4


def test_blend_dispatch_order_heaviest_first_is_invisible(cuda):
    """blend_order_kernel: a frame that holds a tile of 2016+ instances has its blend workgroups dispatched heaviest tile first (a counting sort
    of the frame's tiles by count class).  The order must be a permutation of the tiles -- every pixel of every frame written exactly as in
    image order -- whatever the class populations: a crowded cluster (thousands of instances in a few tiles) in front of a thin background."""
    from gvfdiffusion_amd import rasterizer as R
    P, S, F = 40_000, 240, 10                                  # 225 tiles x 10 frames >= 2048 workgroups: the order launch runs
    attrs = synthetic.random_gaussians(P, sh_degree=0, seed=77, scale_lo=0.002, scale_hi=0.004)
    m = attrs["means3D"]
    m[: P - 4000] = m[: P - 4000] * 0.04                       # 36 000 of them inside a small cube at the origin, the rest spread out
    attrs["opacities"] = attrs["opacities"] * 0.05             # keep T above the cut so that every instance is composited
    gm = synthetic.gaussian_model_from(attrs, 0, cuda)
    cams = [camera_block(azi=36.0 * f, elev=3.0 * f) for f in range(F)]
    frames = [R.make_frame(c["viewmatrix"], c["projmatrix"], c["campos"], c["tanfovx"], c["tanfovy"], -1) for c in cams]
    st = R.make_settings(S, S, 0, 1, synthetic.KERNEL_2D, 1.0, synthetic.BG)
    raw = [t.contiguous().float() for t in (gm._xyz, gm.get_features, gm._scaling, gm._rotation, gm._opacity.reshape(-1))]
    act = gm.activation_struct()
    out = {}
    try:
        for mode in ("1", "0"):
            os.environ["GVF_RAST_BLEND_ORDER"] = mode
            out[mode] = R.rasterize_batched(st, frames, act, *raw, want_alpha_depth=True)
            torch.cuda.synchronize()
            if mode == "1":
                medium, huge = R.sort_class_counts()
                assert medium + huge > 0, "the scene is meant to put 2049+ instances into some tiles (the reorder path)"
    finally:
        os.environ.pop("GVF_RAST_BLEND_ORDER", None)
    for k in ("color", "alpha", "depth", "num_rendered"):
        assert torch.equal(out["1"][k], out["0"][k]), f"{k} depends on the blend's dispatch order"
    # ... and a frame rendered alone (too few workgroups for the order launch) is the same frame
    one = R.rasterize_batched(st, frames[3:4], act, *raw, want_alpha_depth=True)
    assert torch.equal(one["color"][0], out["1"]["color"][3]) and torch.equal(one["alpha"][0], out["1"]["alpha"][3])
    assert float(out["1"]["alpha"].max()) > 0.5


def test_full_size_frame_config2(cuda, oracle_lib, bin_algo):
    """BASELINE.json configs[1] shapes: 262144 Gaussians, 800x800, SH degree 2 -- the static frame and three of the 24 delta frames checked
    against the oracle under north_star's rule (every unflagged pixel <= 1e-3, instance counts exact), 24 frames checked through
    size-independent properties.  The radix-binning run of this test checks one delta frame only (the two algorithms' 24 frames are compared
    bit for bit by the bucket run below); the oracle's frames are computed once per session."""
    from gvfdiffusion_amd.renderers import GaussianRenderer
    P, deg, S = 262_144, 2, 800
    attrs = synthetic.random_gaussians(P, sh_degree=deg, seed=0, scale_lo=0.002, scale_hi=0.01)
    cam = camera_block(azi=15.0)
    full = bin_algo == "bucket"
    if full:
        ref = cached(("config2", "static"), lambda: oracle_render(oracle_lib, attrs, cam, S, S, deg, mode=0))
        color, radii = _run(_settings(cam, S, S, deg, 0, cuda), _to(cuda, attrs))
        assert np.array_equal(radii.cpu().numpy(), ref["radii"])
        e_clean, e_flag, frac = compare_images(color.cpu().numpy(), ref["color"], ref["flags"])
        print(f"config2 frame: D={ref['num_rendered']} max|d|={e_clean:.2e} flagged={frac:.4f}")

    gm = synthetic.gaussian_model_from(attrs, deg, cuda)
    delta = synthetic.random_deltas(24, P, seed=1).to(cuda)
    ext = torch.stack([camera_block(azi=15.0 * f)["extrinsics"] for f in range(24)]).to(cuda)
    K = cam["intrinsics"].to(cuda)
    white = GaussianRenderer({"resolution": S, "near": synthetic.NEAR, "far": synthetic.FAR, "bg_color": (1.0, 1.0, 1.0)})
    black = GaussianRenderer({"resolution": S, "near": synthetic.NEAR, "far": synthetic.FAR, "bg_color": (0.0, 0.0, 0.0)})
    for r in (white, black):
        r.pipe.use_mip_gaussian = True
    w = white.render_frames(gm, ext, K, delta_pc=delta, want_alpha_depth=True)
    assert torch.isfinite(w.rgb).all() and w.rgb.min() >= 0
    # delta frames against the oracle (activations with the frame's (P, 14) delta row + render on the CPU, ~1 s each): the fused activation
    # path at full size, not only the static frame above.  Since round 6 the activations' exp / log1p are ONE operation sequence on both
    # sides (act_expf / act_log1pf), so the instance count is EXACT and the frame is held to the same rule as test_frame_matches_oracle
    # (rounds 4-5: two libms, "a handful of radii may flip", |dD| <= 64 and a bounded share of unflagged pixels off by > 1e-3).
    frames = white.make_frames(ext, K, list(range(24)))
    for f in ((1, 11, 23) if full else (1,)):
        def make(f=f):
            oattrs = oracle_activated(oracle_lib, gm, delta[f], min_kernel_size=float(gm.mininum_kernel_size))
            return oracle_render(oracle_lib, oattrs, cam_from_frame(frames[f]), S, S, deg, mode=0, kernel_size=white.pipe.kernel_size,
                                 bg=(1.0, 1.0, 1.0), tight=True)
        ref_f = cached(("config2", "delta", f), make)
        assert int(w.num_rendered[f]) == ref_f["num_rendered"]
        e_clean, e_flag, frac = compare_images(w.rgb[f].cpu().numpy(), ref_f["color"], ref_f["flags"])
        print(f"config2 delta frame {f}: D={ref_f['num_rendered']} (device: equal) max|d|={e_clean:.2e} flagged={frac:.4f} (max {e_flag:.2e})")
    if not full:
        return
    b = black.render_frames(gm, ext, K, delta_pc=delta, want_alpha_depth=True)
    assert torch.equal(w.alpha, b.alpha) and torch.equal(w.num_rendered, b.num_rendered)
    # out = C + T*bg  =>  white - black == T == 1 - alpha  (compositing identity, size independent)
    assert ((w.rgb - b.rgb) - (1 - w.alpha)[:, None]).abs().max() < 2e-6
    assert w.alpha.min() >= 0 and w.alpha.max() <= 1 - 1e-4 + 1e-6      # T never drops below 1e-4
    # the two binning algorithms (Morton-ordered bucket passes vs radix on the tile bits) and upstream's 3-sigma
    # binning must give the same 24 frames bit for bit: the per-tile (depth, id) order is a total order
    from gvfdiffusion_amd import rasterizer as R, _lib
    this_algo = R.DEFAULT_BIN_ALGO
    R.DEFAULT_BIN_ALGO = _lib.RAST_BIN_RADIX if this_algo != _lib.RAST_BIN_RADIX else _lib.RAST_BIN_BUCKET
    try:
        w_other = white.render_frames(gm, ext, K, delta_pc=delta, want_alpha_depth=True)
    finally:
        R.DEFAULT_BIN_ALGO = this_algo
    assert torch.equal(w_other.rgb, w.rgb) and torch.equal(w_other.alpha, w.alpha) and torch.equal(w_other.depth, w.depth)
    assert torch.equal(w_other.num_rendered, w.num_rendered)
    del w_other
    # permuting the Gaussians changes a frame only where two splats of one pixel have bit-identical
    # depth (ties are broken by index, as upstream's stable sort does): with 262144 depths in [1.5,2.5]
    # (float spacing 1.2e-7) a few thousand exact ties exist, so allow a tiny fraction of pixels
    perm = torch.randperm(P, generator=torch.Generator().manual_seed(3))
    gm2 = synthetic.gaussian_model_from({k: v[perm] for k, v in attrs.items()}, deg, cuda)
    w2 = white.render_frames(gm2, ext[:2], K, delta_pc=delta[:2][:, perm.to(cuda)].contiguous(), want_alpha_depth=True)
    assert torch.equal(w2.num_rendered, w.num_rendered[:2])
    dperm = (w2.rgb - w.rgb[:2]).abs().amax(dim=1)
    assert float((dperm > 1e-5).float().mean()) < 2e-3 and float(dperm.max()) < 0.1


def test_live_shape_frame_matches_oracle(cuda, oracle_lib, bin_algo):
    """The reference's LIVE render shape (utils/inference_utils.py:240-297): 262 144 Gaussians, 512 x 512, SH degree 0, mip filter, a camera of
    the 128-view orbit, one (P, 14) delta row -- one frame against the oracle with the alpha-box binning and with upstream's 3-sigma
    binning.  At this shape a fifth of the tiles hold 2049-16384 keys, i.e. leave the one-workgroup register sort for the two LDS launches
    (tile_sort_kernel<3> / <1>): asserted from the sort's own class counters, so that this frame IS the parity case of those launches."""
    from gvfdiffusion_amd.renderers import GaussianRenderer
    from gvfdiffusion_amd.utils import orbit_cameras
    from gvfdiffusion_amd import rasterizer as R, _lib
    P, S = 262_144, 512
    attrs = synthetic.random_gaussians(P, sh_degree=0, seed=7)
    gm = synthetic.gaussian_model_from(attrs, 0, cuda)
    delta = (torch.randn((1, P, 14), generator=torch.Generator().manual_seed(11)) * 0.01).to(cuda)
    rend = GaussianRenderer({"resolution": S, "near": synthetic.NEAR, "far": synthetic.FAR, "ssaa": 1, "bg_color": (1, 1, 1)})
    rend.pipe.use_mip_gaussian = True
    rend.pipe.kernel_size = synthetic.KERNEL_2D
    ext, K = orbit_cameras(128)[37:38].to(cuda), synthetic.intrinsics().to(cuda)
    frames = rend.make_frames(ext, K, [0])
    oattrs = cached(("live", "activated"), lambda: oracle_activated(oracle_lib, gm, delta[0], min_kernel_size=float(gm.mininum_kernel_size)))
    images = {}
    for upstream in ((False, True) if bin_algo == "bucket" else (False,)):         # (the radix run: one frame; oracle frames cached per session)
        st = R.make_settings(S, S, 0, _lib.RAST_MODE_MIP, rend.pipe.kernel_size, 1.0, (1.0, 1.0, 1.0), upstream_binning=upstream)
        before = int(_lib.lib().gvf_rast_shared_activation_calls())
        out = R.rasterize_batched(st, frames, gm.activation_struct(), gm._xyz, gm.get_features, gm._scaling, gm._rotation, gm._opacity,
                                  delta=delta, want_radii=True)
        medium, huge = R.sort_class_counts(cuda)
        # one frame: the per-frame fused path, by the counter and by the call plan
        plan = R.call_plan(st, frames, P, gm.get_features.shape[1], out["max_rendered"])
        assert int(_lib.lib().gvf_rast_shared_activation_calls()) == before and plan.shared == 0
        assert plan.upstream_binning == int(upstream) and plan.bucket == int(bin_algo == "bucket")
        ref = cached(("live", 37, upstream), lambda: oracle_render(oracle_lib, oattrs, cam_from_frame(frames[0]), S, S, 0, mode=0,
                                                                 kernel_size=rend.pipe.kernel_size, bg=(1.0, 1.0, 1.0), tight=not upstream))
        n_dev = int(out["num_rendered"][0])
        assert medium > 0, "this frame is meant to exercise the 2049-16384-key sort launches"
        # one activation arithmetic on both sides (round 6): radii and the instance count are exact, the image under north_star's rule
        assert n_dev == ref["num_rendered"] and np.array_equal(out["radii"][0].cpu().numpy(), ref["radii"])
        e_clean, e_flag, frac = compare_images(out["color"][0].cpu().numpy(), ref["color"], ref["flags"])
        print(f"live shape, upstream_binning={upstream}: D={ref['num_rendered']} (device: equal), segments with 2049-16384 keys: {medium}, "
              f"larger: {huge}; max|d|={e_clean:.2e} flagged={frac:.4f} (max {e_flag:.2e}), radii exact")
        images[upstream] = out["color"].clone()
    if len(images) == 2:
        assert torch.equal(images[False], images[True])          # the alpha-box rule only drops instances the blend would have skipped


def test_live_shape_camera_batch_matches_oracle(cuda, oracle_lib, bin_algo):
    """The live job as the product runs it since round 5: SEVERAL cameras of one timestep in one call (utils/inference_utils.py:256-269) -- shared
    activation records, the per-frame launch over Morton slots, the blend dispatched heaviest tile first (512^2 tiles of 2-16 k instances) --
    at full size against the ORACLE, frame by frame (the single-frame test above never enters those paths)."""
    from gvfdiffusion_amd.renderers import GaussianRenderer
    from gvfdiffusion_amd.utils import orbit_cameras
    from gvfdiffusion_amd import rasterizer as R, _lib
    P, S, views = 262_144, 512, [5, 37, 70, 101]
    attrs = synthetic.random_gaussians(P, sh_degree=0, seed=7)
    gm = synthetic.gaussian_model_from(attrs, 0, cuda)
    delta = (torch.randn((1, P, 14), generator=torch.Generator().manual_seed(11)) * 0.01).to(cuda)
    rend = GaussianRenderer({"resolution": S, "near": synthetic.NEAR, "far": synthetic.FAR, "ssaa": 1, "bg_color": (1, 1, 1)})
    rend.pipe.use_mip_gaussian = True
    rend.pipe.kernel_size = synthetic.KERNEL_2D
    ext, K = orbit_cameras(128)[views].to(cuda), synthetic.intrinsics().to(cuda)
    frames = rend.make_frames(ext, K, [0] * len(views))
    oattrs = cached(("live", "activated"), lambda: oracle_activated(oracle_lib, gm, delta[0], min_kernel_size=float(gm.mininum_kernel_size)))
    st = R.make_settings(S, S, 0, _lib.RAST_MODE_MIP, rend.pipe.kernel_size, 1.0, (1.0, 1.0, 1.0))
    before = int(_lib.lib().gvf_rast_shared_activation_calls())
    out = R.rasterize_batched(st, frames, gm.activation_struct(), gm._xyz, gm.get_features, gm._scaling, gm._rotation, gm._opacity,
                              delta=delta, want_radii=True)
    medium, huge = R.sort_class_counts(cuda)
    took_shared = int(_lib.lib().gvf_rast_shared_activation_calls()) - before
    assert (took_shared >= 1) == (bin_algo == "bucket") and medium > 0
    plan = R.call_plan(st, frames, P, gm.get_features.shape[1], out["max_rendered"])
    assert bool(plan.shared) == (took_shared >= 1) and plan.slot_mode == plan.shared and plan.order_tiles == 1
    for f in (range(len(views)) if bin_algo == "bucket" else (1,)):                # (the radix run: one frame of the call)
        ref = cached(("live", views[f], False), lambda: oracle_render(oracle_lib, oattrs, cam_from_frame(frames[f]), S, S, 0, mode=0,
                                                                      kernel_size=rend.pipe.kernel_size, bg=(1.0, 1.0, 1.0), tight=True))
        assert int(out["num_rendered"][f]) == ref["num_rendered"] and np.array_equal(out["radii"][f].cpu().numpy(), ref["radii"])
        e_clean, e_flag, frac = compare_images(out["color"][f].cpu().numpy(), ref["color"], ref["flags"])
        print(f"live shape, camera {views[f]} of a {len(views)}-camera call: D={ref['num_rendered']} (device: equal), max|d|={e_clean:.2e} "
              f"flagged={frac:.4f} (max {e_flag:.2e}), radii exact")


@pytest.mark.parametrize("P,spread", [(6000, 0.02), (40_000, 0.01), (20_000, 0.012), (1500, 0.05)])
def test_crowded_tiles_exercise_every_sort_class(cuda, oracle_lib, P, spread):
    """Per-tile sort classes: <= 2048 keys (registers), <= 4096 and <= 16384 (LDS, two launches), larger (global): a cluster of Gaussians
    projected onto a handful of tiles puts thousands of splats into one segment; order must still be exact."""
    attrs = synthetic.random_gaussians(P, sh_degree=0, seed=P, scale_lo=0.002, scale_hi=0.004)
    attrs["means3D"] = attrs["means3D"] * spread * 2            # all inside a +-spread cube at the origin
    attrs["opacities"] = attrs["opacities"] * 0.05              # keep T above the 1e-4 cut so that deep order matters
    cam = camera_block(azi=33.0, elev=7.0)
    H = W = 96
    ref = oracle_render(oracle_lib, attrs, cam, H, W, 0, mode=1, tight=True)    # the binning the HIP path uses
    per_tile_max = ref["num_rendered"] / 36                                     # 6 x 6 tiles: busiest tile >= mean
    assert per_tile_max > {6000: 300, 40_000: 2048, 20_000: 1500, 1500: 10}[P]
    color, depth, _, alpha, radii, _ = _run(_settings(cam, H, W, 0, 1, cuda), _to(cuda, attrs))
    assert np.array_equal(radii.cpu().numpy(), ref["radii"])
    compare_images(color.cpu().numpy(), ref["color"], ref["flags"], max_flag_frac=0.2)
    compare_images(depth[0].cpu().numpy(), ref["depth"], ref["flags"], atol=2e-3, flagged_atol=2e-3, flip_atol=5e-2, max_flag_frac=0.2)
    print(f"P={P}: D={ref['num_rendered']} (~{per_tile_max:.0f}+ keys in the busiest tiles)")


def test_frames_to_uint8_matches_host_postprocess(cuda):
    from gvfdiffusion_amd.rasterizer import frames_to_uint8
    g = torch.Generator().manual_seed(0)
    x = (torch.rand((2, 3, 37, 41), generator=g) * 1.4 - 0.2)
    x.view(-1)[:6] = torch.tensor([0.0, 1.0, 0.5, 254.999 / 255, 1.0 / 255, -3.0])
    ref = (x.clamp(0.0, 1.0).numpy() * 255).astype("uint8")      # utils/inference_utils.py:280-286
    assert np.array_equal(frames_to_uint8(x.to(cuda)).cpu().numpy(), ref)


def test_uint8_frames_from_the_blend_epilogue_equal_the_two_step_form(cuda, bin_algo):
    """gvf_rast_forward_batched_u8 (round 6): the frames leave the compositing kernel as uint8 = the reference's post-process
    (utils/inference_utils.py:280-286) on the very float the fp32 entry point stores -- bit-identical to render + frames_to_uint8, through the C
    ABI, the renderer facade (as_uint8) and the sample driver (white background; SH offsets push colours above 1, so the upper clamp is
    exercised -- colours are clamped at 0 before compositing, the lower one cannot trigger); alpha / depth / radii cannot be asked for together with it."""
    from gvfdiffusion_amd import rasterizer as R, _lib
    from gvfdiffusion_amd.renderers import GaussianRenderer
    from gvfdiffusion_amd.utils import orbit_cameras, render_sample_frames
    P, S = 20_000, 208
    attrs = synthetic.random_gaussians(P, sh_degree=1, seed=77, scale_lo=0.004, scale_hi=0.03)
    attrs["shs"][:, 0] *= 1.8                                  # over-shooting colours
    gm = synthetic.gaussian_model_from(attrs, 1, cuda)
    delta = synthetic.random_deltas(3, P, seed=8).to(cuda)
    rend = GaussianRenderer({"resolution": S, "near": synthetic.NEAR, "far": synthetic.FAR, "ssaa": 1, "bg_color": (1, 1, 1)})
    rend.pipe.use_mip_gaussian = True
    ext, K = orbit_cameras(8).to(cuda), synthetic.intrinsics().to(cuda)
    f32 = rend.render_frames(gm, ext, K, delta_pc=delta, delta_index=[0, 0, 1, 1, 2, 2, -1, -1])
    u8 = rend.render_frames(gm, ext, K, delta_pc=delta, delta_index=[0, 0, 1, 1, 2, 2, -1, -1], as_uint8=True)
    want = R.frames_to_uint8(f32.rgb)
    assert u8.rgb.dtype == torch.uint8 and u8.rgb.shape == (8, 3, S, S)
    assert torch.equal(u8.rgb, want) and torch.equal(u8.num_rendered, f32.num_rendered)
    assert int((want == 255).sum()) > 0 and float(f32.rgb.max()) > 1.0 and int((want < 128).sum()) > 0      # the upper clamp is exercised
    # where the fused form does not apply the facade falls back to the two-step one: same bits
    u8_ad = rend.render_frames(gm, ext, K, delta_pc=delta, delta_index=[0, 0, 1, 1, 2, 2, -1, -1], as_uint8=True, want_alpha_depth=True)
    assert torch.equal(u8_ad.rgb, want) and u8_ad.alpha.shape == (8, S, S)
    with pytest.raises(_lib.GvfError):
        R.rasterize_batched(R.make_settings(S, S, 1, 0, synthetic.KERNEL_2D, 1.0, (1.0, 1.0, 1.0)), rend.make_frames(ext, K, [0] * 8), gm.activation_struct(),
                            gm._xyz, gm.get_features, gm._scaling, gm._rotation, gm._opacity, delta=delta, color_u8=True, want_radii=True)
    # the sample driver: fused (default) == GVF_RENDER_FUSED_U8=0
    got = {}
    for flag in ("1", "0"):
        os.environ["GVF_RENDER_FUSED_U8"] = flag
        try:
            got[flag] = torch.cat([fr for _, fr in render_sample_frames(rend, gm, delta, K, extrinsics=ext, chunk_frames=6, streams=2)])
        finally:
            os.environ.pop("GVF_RENDER_FUSED_U8", None)
    assert got["1"].dtype == torch.uint8 and got["1"].shape == (24, 3, S, S) and torch.equal(got["1"], got["0"])


@pytest.mark.skipif(not os.path.exists(os.path.join(os.path.dirname(__file__), "golden", "raster_cuda_golden.npz")),
                    reason="raster_cuda_golden.npz not generated yet (scripts/make_cuda_raster_golden.py on a CUDA box)")
def test_hip_matches_cuda_golden(cuda):
    """HIP rasteriser against frames of the reference's real CUDA packages (north star: 1e-3 max-abs per pixel)."""
    from test_oracle_rast import cuda_golden_scenes
    for (name, P, deg, seed, slo, shi, H, W, azi, elev), arr in cuda_golden_scenes():
        attrs = synthetic.random_gaussians(P, sh_degree=deg, seed=seed, scale_lo=slo, scale_hi=shi)
        cam = camera_block(azi=azi, elev=elev)
        crop = (slice(None), slice(272, 528), slice(272, 528)) if name.startswith("config1") else (slice(None),) * 3
        for mode, tag in ((0, "mip"), (1, "dilate")):
            ret = _run(_settings(cam, H, W, deg, mode, cuda), _to(cuda, attrs))
            color, radii = (ret[0], ret[1]) if mode == 0 else (ret[0], ret[4])
            assert np.array_equal(radii.cpu().numpy(), arr[f"{tag}.radii"])
            err = np.abs(color.cpu().numpy()[crop] - arr[f"{tag}.color"])
            print(f"{name}/{tag}: HIP vs CUDA max|d| {err.max():.2e}, > 1e-3 on {float((err.max(0) > 1e-3).mean()):.4f} of the pixels")
            assert float((err.max(0) > 1e-3).mean()) <= 0.03 and err.max() <= 2e-2


@pytest.mark.parametrize("mode", [0, 1])
def test_closed_form_scenes_on_the_device(cuda, oracle_lib, mode):
    """The hand-derived known answers of tests/test_oracle_rast_closed_form.py through the HIP operator: one isotropic Gaussian on the optical
    axis (pixel-centre convention, both dilation modes) and the stop rule of the front-to-back walk."""
    import math
    import test_oracle_rast_closed_form as cf
    H, W, BG = cf.H, cf.W, cf.BG
    z, s, op, col = 2.0, 0.08, 0.7, (0.9, 0.3, 0.1)
    cam, attrs, c = cf._scene([z], [s], [op], [col])
    rast = _settings(cam, H, W, 0, mode, cuda, kernel_size=0.1, bg=BG)
    ret = _run(rast, _to(cuda, attrs), shs=None, colors_precomp=c.to(cuda))
    img = ret[0].cpu().numpy()
    sig2, coef = cf._sigma2(cam, s, z, mode, 0.1)
    yy, xx = np.mgrid[0:H, 0:W]
    a = np.minimum(0.99, op * coef * np.exp(-0.5 * ((xx - 15.5) ** 2 + (yy - 15.5) ** 2) / sig2))
    a[a < 1.0 / 255.0] = 0.0
    exp_img = np.asarray(col)[:, None, None] * a[None] + np.asarray(BG)[:, None, None] * (1 - a[None])
    # (a pixel whose alpha is within float noise of 1/255 may go either way between v_exp_f32 and exp(): none in this scene)
    assert np.abs(np.abs(a - 1.0 / 255.0) < 1e-6).sum() == 0
    assert np.abs(img - exp_img).max() < 3e-6
    assert np.array_equal(img[:, 0, 0], np.asarray(BG, np.float32))
    if mode == 1:
        assert np.abs(ret[3][0].cpu().numpy() - a).max() < 3e-6
        cam, attrs, c = cf._scene([1.2, 1.6, 2.0, 2.4], [0.6, 0.8, 1.0, 1.2], [0.9, 1.0, 1.0, 1.0], [(1.0, 0, 0), (0, 1.0, 0), (0, 0, 1.0), (1.0, 1.0, 1.0)])
        rast = _settings(cam, H, W, 0, 1, cuda, bg=(0.0, 0.0, 0.0))
        ret = _run(rast, _to(cuda, attrs), shs=None, colors_precomp=c.to(cuda))
        g = math.exp(-0.25 / cf._sigma2(cam, 0.6, 1.2, 1, 0.1)[0])
        px = ret[0][:, 15, 15].cpu().numpy()
        assert abs(px[0] - 0.9 * g) < 3e-6 and abs(px[1] - 0.99 * (1 - 0.9 * g)) < 3e-6 and px[2] == 0.0

