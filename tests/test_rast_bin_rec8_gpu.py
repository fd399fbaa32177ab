"""8-byte bin records against the 16-byte form -- needs an MI355X.

The bucket binning keeps per (frame, Gaussian) the final tile rect and the depth bits: in 8 bytes when the tile grid is at most 255 x 255
(csrc/rast_plan.h: RastPlan::rec8), in 16 bytes on larger grids or with GVF_RAST_BIN_REC8=0.  Both forms are lossless, so every scene below,
rendered once with the switch unset and once with it set to "0", must give the same bits in every output: colour, alpha, depth, radii and
the per-frame instance counts.  The scenes cover the index-ordered count pass with the Morton-order gather, bin_kernel<false> (more tiles
than the count table holds), the shared-activation path in slot order and both sides of the 255 / 256 tile-column threshold."""
import pytest
import torch

from gvfdiffusion_amd import synthetic
from rast_util import camera_block

pytestmark = pytest.mark.gpu

OUTPUTS = ("color", "alpha", "depth", "radii", "num_rendered")


def _render(cuda, attrs, delta, idx, H, W, deg, cams=None):
    from gvfdiffusion_amd import rasterizer as R
    gm = synthetic.gaussian_model_from(attrs, deg, cuda)
    cams = cams or [camera_block(azi=41.0 * f, elev=5.0 * f - 12.0) for f in range(len(idx))]
    frames = [R.make_frame(c["viewmatrix"], c["projmatrix"], c["campos"], c["tanfovx"], c["tanfovy"], di) for c, di in zip(cams, idx)]
    st = R.make_settings(H, W, deg, 0, synthetic.KERNEL_2D, 1.0, synthetic.BG)
    raw = [t.contiguous().float() for t in (gm._xyz, gm.get_features, gm._scaling, gm._rotation, gm._opacity.reshape(-1))]
    out = R.rasterize_batched(st, frames, gm.activation_struct(), *raw, delta=delta.to(cuda), want_alpha_depth=True, want_radii=True)
    torch.cuda.synchronize()
    plan = R.call_plan(st, frames, attrs["means3D"].shape[0], raw[1].shape[1], out["max_rendered"])
    return out, plan, R.bin_record_bytes(st)


def _both_forms(monkeypatch, render, expect_default):
    """The scene with the switch unset (the record size must be expect_default) and with the 16-byte form forced: the same bits."""
    monkeypatch.delenv("GVF_RAST_BIN_REC8", raising=False)
    out, plan, nbytes = render()
    assert nbytes == expect_default
    monkeypatch.setenv("GVF_RAST_BIN_REC8", "0")
    out16, plan16, nbytes16 = render()
    assert nbytes16 == 16
    for k in OUTPUTS:
        assert torch.equal(out[k], out16[k]), f"{k}: {expect_default}-byte bin records differ from the forced 16-byte form"
    assert int(out["num_rendered"].sum()) > 0 and float(out["color"].std()) > 0
    return out, plan


@pytest.fixture(scope="module")
def scene():
    P, deg = 40_000, 1
    return dict(P=P, deg=deg, attrs=synthetic.random_gaussians(P, sh_degree=deg, seed=23, scale_lo=0.003, scale_hi=0.03),
                delta=synthetic.random_deltas(8, P, seed=31))


# (a) 256 x 256: 256 tiles, the index-ordered count pass and the Morton-order gather;  (b) 1088 x 1088: 4624 tiles exceed the count table,
# bin_kernel<false> counts.  Eight frames with eight delta slices: the fused path (no shared activation)
@pytest.mark.parametrize("S", [256, 1088])
def test_fused_path(cuda, monkeypatch, scene, S):
    out, plan = _both_forms(monkeypatch, lambda: _render(cuda, scene["attrs"], scene["delta"], list(range(8)), S, S, scene["deg"]), 8)
    assert plan.shared == 0 and plan.morton == 1 and plan.rec_gather == 1 and plan.wave_frames == 1
    assert plan.index_count == int(S == 256)


# (c) two slices over eight frames (the pattern of tests/test_rast_bin_layout_gpu.py): shared activation, records at the Morton slots
def test_shared_activation_in_slot_order(cuda, monkeypatch, scene):
    idx = [0, 0, 0, 1, 1, 1, 0, 1]
    out, plan = _both_forms(monkeypatch, lambda: _render(cuda, scene["attrs"], scene["delta"][:2], idx, 256, 256, scene["deg"]), 8)
    assert plan.shared == 1 and plan.slot_mode == 1 and plan.rec_gather == 0 and plan.index_count == 0


def _wide_scene():
    """A strip seen from the front (camera at (0, -2, 0), world x = image x, depth 2 in the plane y = 0): one Gaussian wide enough for its
    tile rect to span every tile column, six small ones within 0.1 %, 0.4 % and 1 % of the left and the right image edge, and a random
    fill.  4103 Gaussians: an odd count, so that odd frames start at odd positions of the record array."""
    deg, n_fill = 1, 4096
    fill = synthetic.random_gaussians(n_fill, sh_degree=deg, seed=5, scale_lo=0.003, scale_hi=0.03)
    tan = camera_block(azi=0.0)["tanfovx"]
    u = torch.tensor([-0.999, -0.996, -0.99, 0.99, 0.996, 0.999])                     # normalised image x of the edge Gaussians
    xyz = torch.zeros((7, 3))
    xyz[1:, 0] = u * 2.0 * tan
    scales = torch.full((7, 3), 0.004)
    scales[0] = torch.tensor([0.5, 0.01, 0.01])                                       # 3 sigma = 1.5 of the 0.91 half width
    rot = torch.zeros((7, 4)); rot[:, 0] = 1.0
    shs = torch.zeros((7, 4, 3)); shs[:, 0] = torch.tensor([[0.9, -0.6, 0.3]]) * torch.arange(1, 8)[:, None] / 4.0
    special = dict(means3D=xyz, scales=scales, rotations=rot, opacities=torch.full((7, 1), 0.99), shs=shs)
    attrs = {k: torch.cat([special[k], fill[k]]) for k in fill}
    return attrs, synthetic.random_deltas(4, n_fill + 7, seed=9, std=0.002), deg


# four frames from almost the same direction with four delta slices: the fused path with the Morton-order gather
def _wide_cams():
    return [camera_block(azi=0.0, elev=0.02 * f) for f in range(4)]


# (d) 4080 x 32 px: 255 tile columns, the largest grid of the 8-byte form; the wide Gaussian's rect is 0 .. 255
def test_grid_edge_255_columns_takes_8_bytes(cuda, monkeypatch):
    attrs, delta, deg = _wide_scene()
    out, plan = _both_forms(monkeypatch, lambda: _render(cuda, attrs, delta, [0, 1, 2, 3], 32, 4080, deg, _wide_cams()), 8)
    assert plan.gx == 255 and plan.rec_gather == 1 and plan.index_count == 1
    assert int(out["radii"][:, 0].min()) > 2100               # the wide Gaussian sits at x = 2040: its 3-sigma rect is 0 .. 255
    assert float(out["alpha"][:, :, :16].max()) > 0 and float(out["alpha"][:, :, 4064:].max()) > 0      # both edge tile columns hold content


# (e) 4096 x 32 px: 256 tile columns do not fit 8 bits; the 16-byte form by itself, and the rightmost column is rendered
def test_grid_edge_256_columns_keeps_16_bytes(cuda, monkeypatch):
    attrs, delta, deg = _wide_scene()
    out, plan = _both_forms(monkeypatch, lambda: _render(cuda, attrs, delta, [0, 1, 2, 3], 32, 4096, deg, _wide_cams()), 16)
    assert plan.gx == 256 and plan.rec_gather == 1 and plan.index_count == 1
    assert int(out["radii"][:, 0].min()) > 2100               # the wide Gaussian's 3-sigma rect is 0 .. 256
    last = slice(4080, 4096)
    assert float(out["alpha"][:, :, last].max()) > 0
    bg = torch.tensor(synthetic.BG, device=out["color"].device)[None, :, None, None]
    assert bool((out["color"][:, :, :, last] != bg).any()), "the rightmost tile column holds background only"
    # the edge Gaussians at 0.1 % from the right edge are binned there: radius > 0 in every frame
    assert bool((out["radii"][:, 6] > 0).all())
