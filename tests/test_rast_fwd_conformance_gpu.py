"""Stage-wise fp64 conformance of the rasteriser FORWARD (csrc/rast_front.hip, rast_sort.hip, rast_blend.hip) -- needs an MI355X.

The forward runs through the package (rasterizer._rasterize_impl / _rasterize_batched_impl with private_workspace=True, alpha and depth
asked for in both modes); what it left in its workspace -- the 64-byte splat records, the tile ranges, the sorted per-tile id lists, the
slot table and the layout word -- is read through the Python mirror of the workspace layout (tests/rast_fwd_ref.py; no C entry point serves
this test).  Every case runs once per binning algorithm, and per case and frame in three stages (measures and bar: rast_fwd_ref):

  stage A, projection   the unpacked records of the visible Gaussians against rast64_project, per column, bar 4 x rast32_project.  The
                        visible set (radii > 0) and the radii equal the oracle's exactly; Gaussians with FLAG_NEAR (<= 1 %) are excluded.
                        A finding of the first device run: the front end does not write the record of a visible Gaussian that the culled
                        binning drops from EVERY tile of its 3-sigma rect (its slot keeps whatever the workspace held; no list names it, so
                        nothing reads it: 41 of 532 and 22 of 347 visible Gaussians of the two wide scenes, one of nonsquare-40x72).
                        Which Gaussians those are comes from the fp32 oracle's binning rule (rast_oracle.c, shared with the device bit for
                        bit), not from the device; their records are not read here either.
  stage B, lists        exact: per tile no duplicates, sorted by (depth bits of the device's own record, id), members only inside the
                        oracle's 3-sigma rect -- and exactly the Gaussians the fp32 oracle's binning rule puts on that tile --, sum of the
                        lengths = num_rendered, and complete: rast64_blend over the device's records with the device's lists and with the
                        full 3-sigma lists agree to 1e-12 on every unflagged pixel (a pair the culled binning dropped may only ever have
                        contributed alpha < 1/255).
  stage C, blend        the device's colour, alpha and depth against rast64_blend of THE DEVICE'S OWN records over THE DEVICE'S OWN lists:
                        nothing discontinuous is left but the flagged decisions (alpha at 1/255 or at the 0.99 clamp, test_T at 1e-4, power
                        at 0; such pixels are excluded, <= 3 % asserted).  Bar: 4 x rast32_blend(form=1), the device's documented algorithm
                        in plain C.  The ratio against form 0 (upstream's expression) is printed and recorded, without a bar: the Cholesky
                        form trades accuracy for instructions by design.
Also per case: the call plan's fields (no case can silently take another path), the layout word, and a second launch with a workspace of
its own gives bit-identical records, radii, ranges, lists and images (the forward has no atomics in its outputs).

Cases: the eighteen single-frame scenes of the backward conformance (its SINGLE dict and rast_bwd_ref.make_case), `opaque` (added here:
rast_fwd_ref.opaque_case, the only scene whose alpha reaches the 0.99 clamp), the single-Gaussian closed form in both modes, and three
batched calls at 64 x 64 on the oracle's activated attributes (bit-exact with the device's activation,
test_rast_gpu.py::test_activation_kernel_matches_oracle): P = 300, F = 5 over five delta slices (the fused wave-frames launch, records at
the Gaussian's index); P = 5000, F = 8 over eight slices (Morton order, gathering bin pass); P = 5000, F = 8 over two slices (shared
activation, records in SLOT order, read through order_alt).  Of a batched call the frames of different waves / workgroups and loop trips and
the last frame are checked.  Depth ties: the single-frame scenes and the 300-Gaussian call have none (asserted); with 5000 Gaussians on 16
tiles a scene without pairs within 4 fp32 ulps does not exist (tests/test_rast_bwd_conformance_gpu.py found the same at 4096), and as there
the pixels at which both Gaussians of such a pair can be composited are left out of stage C together with the flagged ones, under the same
3 % cap -- stages A and B do not depend on the order of a tied pair (the lists are checked against the device's own depth bits).

Measured on an MI355X (device max/p99 : yardstick max/p99 of e, the column resp. channel with the worst ratio, the worse of the two binning
algorithms; the last column is the device against rast32_blend(form=0), upstream's expression, and carries no bar; `-s` prints every figure):
  case                              stage A, worst column  device : yardstick     ratio   stage C, worst channel  device : yardstick  ratio   form-0 ratio (colour/alpha/depth)
  narrow-mip-sh0                    conic_c  12.94/8.12 : 10.34/7.35              1.25    depth  78.27/29.57 : 78.27/28.91            1.02    3.80/1.41/4.24
  narrow-mip-sh1                    conic_a  13.61/7.19 : 12.71/7.32              1.07    depth  62.62/36.21 : 56.52/36.85            1.11    3.53/1.17/4.94
  narrow-mip-sh2                    conic_b  15.22/6.12 : 15.51/5.58              1.10    depth  51.86/32.86 : 52.50/30.17            1.09    4.10/1.02/4.94
  narrow-mip-sh3                    conic_b  10.87/6.49 : 10.02/6.60              1.09    color  31.50/5.56 : 31.50/5.45              1.02    6.19/1.72/6.85
  narrow-dilate-sh0                 conic_c  6.26/5.78 : 6.39/4.95                1.17    alpha  118.86/69.83 : 109.78/69.90          1.08    2.55/1.08/4.47
  narrow-dilate-sh1                 conic_a  7.43/5.46 : 5.63/5.09                1.32    depth  55.41/25.95 : 55.41/26.66            1.00    2.09/1.20/4.48
  narrow-dilate-sh2                 conic_c  8.29/5.33 : 7.49/4.96                1.11    depth  53.69/23.18 : 53.69/22.94            1.01    2.45/1.05/4.34
  narrow-dilate-sh3                 conic_a  7.79/4.94 : 6.91/4.51                1.13    depth  59.05/29.80 : 51.03/26.08            1.16    4.39/1.02/4.46
  p97                               conic_a  5.86/4.57 : 4.37/3.72                1.34    alpha  135.82/117.38 : 135.82/94.46         1.24    9.62/1.43/9.71
  p257                              conic_a  5.20/4.19 : 3.91/3.24                1.33    alpha  99.00/67.12 : 99.00/62.62            1.07    2.95/1.20/4.58
  wide-mip                          conic_b  93.91/27.77 : 93.46/27.36            1.01    alpha  2.73/1.50 : 2.59/1.50                1.05    1.00/1.03/0.92
  wide-dilate-sh3                   conic_c  35.71/19.22 : 35.28/19.68            1.01    color  8.97/4.69 : 7.62/4.73                1.18    1.13/0.96/1.04
  nonsquare-40x72                   conic_a  9.57/7.00 : 9.33/7.17                1.03    depth  98.86/35.42 : 97.22/31.53            1.12    2.55/1.12/5.42
  scale-modifier-1.3                conic_c  13.21/9.05 : 14.05/8.18              1.11    depth  61.80/23.15 : 48.50/25.40            1.27    2.13/1.20/3.39
  precomputed                       conic_b  10.11/6.85 : 10.25/5.98              1.14    color  20.98/5.50 : 19.44/5.40              1.08    4.46/1.03/3.97
  precomputed-dilate                conic_c  6.90/5.06 : 5.71/4.56                1.21    color  21.77/5.41 : 19.87/5.31              1.10    3.31/1.13/4.90
  subpixel                          conic_a  12.41/9.12 : 10.63/7.81              1.17    depth  216.60/88.02 : 216.60/83.71          1.05    1.01/1.00/1.15
  crowded                           conic_c  10.97/7.06 : 10.90/6.31              1.12    depth  21.72/14.04 : 21.21/12.91            1.09    0.94/0.97/0.98
  opaque                            conic_a  7.43/5.46 : 5.63/5.09                1.32    color  14.20/6.00 : 19.34/5.85              1.03    1.97/1.09/4.63
  single-gaussian-mode0             conic_c  3.23/3.23 : 2.49/2.49                1.30    depth  15.37/14.78 : 15.37/14.78            1.00    2.17/1.00/1.59
  single-gaussian-mode1             conic_c  3.21/3.21 : 2.23/2.23                1.44    color  6.61/1.59 : 6.61/2.37                1.00    5.18/1.03/5.61
  batched-fused-5-slices frame 0    conic_c  17.99/11.94 : 18.45/11.29            1.06    color  10.10/3.43 : 11.72/3.40              1.01    2.01/1.15/4.74
  batched-fused-5-slices frame 2    conic_c  12.48/7.95 : 12.80/7.27              1.09    color  10.38/3.29 : 11.09/3.05              1.08    1.96/1.00/4.88
  batched-fused-5-slices frame 4    conic_a  9.39/8.19 : 9.94/7.12                1.15    color  9.22/3.53 : 9.60/3.45                1.02    2.37/1.01/5.53
  batched-morton-8-slices frame 1   conic_c  17.28/7.68 : 16.67/7.31              1.05    depth  65.79/27.97 : 65.79/23.99            1.17    1.10/1.34/4.88
  batched-morton-8-slices frame 4   conic_c  17.00/7.67 : 16.33/7.24              1.06    depth  62.56/31.14 : 60.25/27.04            1.15    1.71/1.14/3.87
  batched-morton-8-slices frame 7   conic_b  18.24/7.05 : 16.91/6.97              1.08    color  16.10/7.36 : 16.10/7.40              1.00    1.11/0.99/2.84
  batched-shared-2-slices frame 0   conic_a  18.08/8.06 : 16.17/7.72              1.12    alpha  152.25/54.43 : 152.25/49.21          1.11    1.41/1.28/3.24
  batched-shared-2-slices frame 5   conic_a  22.56/8.07 : 22.45/7.56              1.07    color  15.06/7.28 : 13.16/7.13              1.14    1.24/1.02/3.88
  batched-shared-2-slices frame 7   conic_c  19.42/7.66 : 17.86/7.40              1.09    depth  50.85/20.48 : 41.10/20.93            1.24    1.88/1.20/4.10
Every ratio that carries a bar is <= 1.44 (stage A) and <= 1.27 (stage C).  Against upstream's expression the Cholesky form costs up to 9.7 x
in colour and depth (typically 2 .. 5 x; nothing where wide or crowded footprints make the conic form cancel as much), which is the
accuracy DESIGN says it trades.  The large alpha figures (both sides alike) are pixels of small coverage: alpha leaves as 1 - T, one
rounding of a number near 1, against a scale sum(alpha T) of a few 1e-3.  Depth-tied pairs in the checked frames of the 5000-Gaussian
calls: 8 .. 16 per frame, 0 .. 11 pixels left out for them.  Closed form (single Gaussian): max |d| 2.3e-7 (mode 0), 1.4e-7 (mode 1).
"""
import numpy as np
import pytest
import torch

import oracle
import rast_bwd_ref as R
import rast_fwd_ref as F
from gvfdiffusion_amd import _lib, synthetic
from gvfdiffusion_amd import rasterizer as _r
from rast_util import cached, camera_block, oracle_activated
from test_rast_bwd_conformance_gpu import SINGLE, _kw_from, _structs, _t

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True, params=["bucket", "radix"])
def bin_algo(request):
    """Every test of this file runs with both instance-binning algorithms (include/gvf_rast.h GVF_RAST_BIN_*)."""
    old = _r.DEFAULT_BIN_ALGO
    _r.DEFAULT_BIN_ALGO = _lib.RAST_BIN_BUCKET if request.param == "bucket" else _lib.RAST_BIN_RADIX
    yield request.param
    _r.DEFAULT_BIN_ALGO = old


def _images(fwd, f=None):
    pick = lambda t: (t if f is None else t[f]).cpu().numpy()
    return dict(color=pick(fwd["color"]), alpha=pick(fwd["alpha"]), depth=pick(fwd["depth"]))


def _same_bits(label, a, b):
    assert a.shape == b.shape and np.array_equal(np.ascontiguousarray(a).view(np.uint8), np.ascontiguousarray(b).view(np.uint8)), \
        f"{label}: a second launch gives other bits"


def _check_frame(label, ws, f, fwd_images, num_rendered, ref, kw, sub, slot_order, mask_ties):
    """The three stages on frame f of a call.  ref: rast_fwd_ref.reference() of the frame's inputs."""
    H, W, bg = kw["H"], kw["W"], kw["bg"]
    P = ref["vis"].shape[0]
    radii = ws["radii"][f][:P]
    assert np.array_equal(radii, ref["radii"]), f"{label}: the forward's radii differ from the oracle's"
    vis = radii > 0
    assert np.array_equal(vis, ref["vis"]), f"{label}: the visible set differs from the oracle's"
    # (the record of a Gaussian that the binning drops from every tile of its 3-sigma rect is never written and never read)
    rec, bits = F.unpack_records(ws["splats"][f][:P], vis & ref["binned"], ws["order_alt"][:P] if slot_order else None)
    report = F.projection_report(label, rec, ref["proj64"], ref["proj32"], H, W, binned=ref["binned"])
    ranges, ids = F.frame_lists(ws, f)
    ref64 = F.check_lists(label, rec, bits, ranges, ids, ref["rects"], num_rendered, bg=bg, H=H, W=W, sub=sub, binned_rects=ref["binned_rects"])
    rec32 = rec.astype(np.float32)
    yard1 = oracle.rast32_blend(rec32, form=1, ranges=ranges, ids=ids, subpixel_offset=sub, bg=bg, H=H, W=W)
    yard0 = oracle.rast32_blend(rec32, form=0, ranges=ranges, ids=ids, subpixel_offset=sub, bg=bg, H=H, W=W)
    exclude = None
    if mask_ties:
        exclude = F.tie_pixels(ref["ties"], ref["proj64"]["out"], H, W, sub)
        print(f"{label}: {len(ref['ties'])} depth-tied pairs, {int(exclude.sum())} pixels left out for them")
    else:
        assert not ref["ties"], f"{label}: visible Gaussians sharing a tile with depths within 4 fp32 ulps: {ref['ties']}"
    report += F.blend_report(label, fwd_images, ref64, yard1, bg, yard0=yard0, exclude=exclude)
    return report, rec, ref64


# ---- single frame -------------------------------------------------------------------------------------------------------------------
def _check_single(c, label, dev, bin_algo, min_clamped=0):
    st, fr = _structs(c)
    c.kw = _kw_from(st, fr)
    ref = cached(("rast_fwd_conformance", label), lambda: F.reference(c.ins, c.kw, c.sub))
    fl = ref["proj64"]["flags"]
    clamped = ((fl & oracle.FLAG_CLAMPED) != 0) & ref["vis"]
    assert clamped.sum() >= min_clamped, f"only {clamped.sum()} clamped visible Gaussians"
    tensors = tuple(_t(a, dev) for a in c.ins) + (_t(c.sub, dev),)
    m3, sh, col, op, sc, ro, c6, sub = tensors
    M = 0 if sh is None else sh.shape[1]
    run = lambda: _r._rasterize_impl(st, fr, m3, op, sh, col, sc, ro, c6, sub, True, private_workspace=True)
    fwd = run()
    plan = _r.call_plan(st, [fr], c.P, M, fwd["max_rendered"], fused=False, has_sh=sh is not None, has_colors_precomp=col is not None,
                        has_cov3D_precomp=c6 is not None, has_delta=False, has_subpixel_offset=sub is not None)
    assert plan.bucket == int(bin_algo == "bucket") and plan.shared == 0 and plan.slot_mode == 0 and plan.layout == 0 and plan.morton == 0
    assert plan.upstream_binning == int(sub is not None) and plan.index_count == plan.bucket and plan.n_slices == 1
    ws = F.read_workspace(fwd, c.P, 1, c.H, c.W)
    assert int(ws["mm"][F.LAYOUT_WORD]) == 0
    assert np.array_equal(fwd["radii"].cpu().numpy(), ws["radii"][0][:c.P])
    print(f"{label} [{bin_algo}]: P={c.P} {c.H}x{c.W} visible {ref['vis'].sum()} clamped {clamped.sum()} instances {fwd['num_rendered']}")
    report, rec, ref64 = _check_frame(label, ws, 0, _images(fwd), fwd["num_rendered"], ref, c.kw, c.sub, False, False)
    # a second launch, in a workspace of its own
    fwd2 = run()
    ws2 = F.read_workspace(fwd2, c.P, 1, c.H, c.W)
    vis = ref["vis"] & ref["binned"]
    _same_bits(label + " records", ws["splats"][0][:c.P][vis][:, :12], ws2["splats"][0][:c.P][vis][:, :12])
    _same_bits(label + " radii", ws["radii"], ws2["radii"])
    _same_bits(label + " ranges", ws["ranges"], ws2["ranges"])
    _same_bits(label + " lists", ws["ids"][:fwd["num_rendered"]], ws2["ids"][:fwd["num_rendered"]])
    assert fwd2["num_rendered"] == fwd["num_rendered"]
    for k in ("color", "alpha", "depth"):
        assert torch.equal(fwd[k], fwd2[k]), f"{label} {k}: a second launch gives other bits"
    F.assert_report(f"{label} [{bin_algo}]", report)
    return fwd, rec, ref64, ws


@pytest.mark.parametrize("name", list(SINGLE))
def test_single_frame(cuda, oracle_lib, bin_algo, name):
    c = R.make_case(**SINGLE[name])
    _, _, _, ws = _check_single(c, name, cuda, bin_algo, min_clamped=20 if name.startswith("wide") else 0)
    if name == "crowded":
        assert (ws["ranges"][0][:, 1] - ws["ranges"][0][:, 0]).max() > 512, "no tile of the crowded scene needs a second staging round"


def test_opaque_scene_reaches_the_clamp(cuda, oracle_lib, bin_algo):
    c = F.opaque_case()
    _, rec, ref64, ws = _check_single(c, "opaque", cuda, bin_algo)
    ranges, ids = F.frame_lists(ws, 0)
    assert F.clamp_active(rec, ranges, ids, bg=c.kw["bg"], H=c.H, W=c.W) >= 10, "no alpha of the scene reaches the 0.99 clamp"
    assert float(ref64["alpha"].max()) > 1.0 - 2e-4, "T does not run out anywhere in the scene"


@pytest.mark.parametrize("mode", [0, 1])
def test_single_gaussian_closed_form(cuda, oracle_lib, bin_algo, mode):
    """P = 1, the isotropic Gaussian on the optical axis of tests/test_oracle_rast_closed_form.py: colour = c a + bg (1 - a) with
    a = o coef exp(-d^2 / 2 sigma^2) where a >= 1/255, the exact background elsewhere.  Tolerance as in the backward's closed-form test:
    the closed form's own 1e-6 plus 64 roundings (the exponent is at most ln(0.7 * 255) = 5.2 and comes from a conic ~10 fp32 operations
    deep), of colour's scale c a + bg (1 - a) <= 1."""
    import test_oracle_rast_closed_form as cf
    c = R.make_case(P=1, H=cf.H, W=cf.W, deg=0, mode=mode, seed=1, single=True)
    fwd, _, _, _ = _check_single(c, f"single-gaussian-mode{mode}", cuda, bin_algo)
    yy, xx = np.mgrid[0:cf.H, 0:cf.W]
    d2 = (xx - 15.5) ** 2 + (yy - 15.5) ** 2
    sig2, coef = cf._sigma2(c.cam, 0.08, 2.0, mode, 0.1)
    a = 0.7 * coef * np.exp(-0.5 * d2 / sig2)
    edge = np.abs(a - 1.0 / 255.0) < 1e-3 / 255.0
    a = np.where(a >= 1.0 / 255.0, a, 0.0)
    col, bg = np.array([0.9, 0.3, 0.1]), np.array([0.2, 0.4, 0.6])
    want = col[:, None, None] * a[None] + bg[:, None, None] * (1.0 - a[None])
    got = fwd["color"].cpu().numpy().astype(np.float64)
    err = np.abs(got - want)[:, ~edge]
    print(f"single-gaussian-mode{mode}: closed form max |d| {err.max():.2e}")
    assert err.max() <= 1e-6 + 64 * R.U
    assert np.abs(fwd["alpha"].cpu().numpy() - a)[~edge].max() <= 1e-6 + 64 * R.U


# ---- batched ------------------------------------------------------------------------------------------------------------------------
BATCHED = {
    # fused wave-frames launch (bucket), records at the Gaussian's index: wave 0 trip 0, wave 2, and frame 4 = wave 0's second trip, the last
    "fused-5-slices": dict(P=300, deg=2, di=[0, 1, 2, 3, 4], check=[0, 2, 4], seed=81,
                           plan=dict(shared=0, wave_frames=1, index_count=1, morton=0, rec_gather=0, slot_mode=0, layout=0, n_slices=5)),
    # Morton order with the gathering bin pass: frames of three waves, of both trips, and the last
    "morton-8-slices": dict(P=5000, deg=1, di=[0, 1, 2, 3, 4, 5, 6, 7], check=[1, 4, 7], seed=82,
                            plan=dict(shared=0, wave_frames=1, index_count=1, morton=1, rec_gather=1, slot_mode=0, layout=0, n_slices=8)),
    # shared activation, slot order: both slices, both frame groups of the per-frame launch, and the last frame
    "shared-2-slices": dict(P=5000, deg=1, di=[0, 1, 0, 1, 0, 1, 0, 1], check=[0, 5, 7], seed=83,
                            plan=dict(shared=1, wave_frames=0, index_count=0, morton=1, rec_gather=0, slot_mode=1, layout=1, n_slices=2)),
}
RADIX_PLAN = dict(bucket=0, shared=0, wave_frames=0, index_count=0, morton=0, rec_gather=0, slot_mode=0, layout=0)


def _batched_scene(name):
    b = BATCHED[name]
    P, deg, S = b["P"], b["deg"], 64
    attrs = synthetic.random_gaussians(P, sh_degree=deg, seed=b["seed"], scale_lo=0.004, scale_hi=0.04)
    attrs["means3D"] = attrs["means3D"] * 0.8
    attrs["opacities"] = attrs["opacities"].clamp(0.02, 0.95)
    gm = synthetic.gaussian_model_from(attrs, deg, torch.device("cpu"))
    delta = synthetic.random_deltas(max(b["di"]) + 1, P, seed=b["seed"] + 1, std=0.01)
    cams = [camera_block(azi=360.0 * f / len(b["di"]) + 7.0, elev=10.0 - 3.0 * (f % 3)) for f in range(len(b["di"]))]
    return gm, delta, cams, S


@pytest.mark.parametrize("name", list(BATCHED))
def test_batched(cuda, oracle_lib, bin_algo, name):
    b = BATCHED[name]
    gm, delta, cams, S = _batched_scene(name)
    P, deg, nF = b["P"], b["deg"], len(b["di"])
    st = _r.make_settings(S, S, deg, _lib.RAST_MODE_MIP, synthetic.KERNEL_2D, 1.0, (0.3, 0.3, 0.3))
    frames = [_r.make_frame(c["viewmatrix"], c["projmatrix"], c["campos"], c["tanfovx"], c["tanfovy"], d) for c, d in zip(cams, b["di"])]

    def frame_reference(f):
        a = oracle_activated(oracle, gm, delta[b["di"][f]])
        n = lambda t: t.numpy()
        ins = (n(a["means3D"]), n(a["shs"]), None, n(a["opacities"]).reshape(-1), n(a["scales"]), n(a["rotations"]), None)
        kw = _kw_from(st, frames[f])
        return dict(kw=kw, **F.reference(ins, kw))

    refs = {f: cached(("rast_fwd_conformance_batched", name, f), lambda f=f: frame_reference(f)) for f in b["check"]}
    raw = [t.detach().contiguous().float().to(cuda) for t in (gm._xyz, gm.get_features, gm._scaling, gm._rotation, gm._opacity.reshape(-1))]
    dl = delta.to(cuda).contiguous()
    act = gm.activation_struct()
    lib = _lib.lib()

    def run():
        n0 = lib.gvf_rast_shared_activation_calls()
        out = _r._rasterize_batched_impl(st, frames, act, *raw, dl, True, True, private_workspace=True)
        return out, lib.gvf_rast_shared_activation_calls() - n0

    fwd, took = run()
    plan = _r.call_plan(st, frames, P, raw[1].shape[1], fwd["max_rendered"])
    want = dict(b["plan"], bucket=1) if bin_algo == "bucket" else dict(RADIX_PLAN, n_slices=b["plan"]["n_slices"])
    got = {k: getattr(plan, k) for k in want}
    assert got == want, f"the call took another path: {got}"
    assert (took > 0) == bool(want["shared"]), "gvf_rast_shared_activation_calls disagrees with the plan"
    ws = F.read_workspace(fwd, P, nF, S, S)
    slot_order = bool(int(ws["mm"][F.LAYOUT_WORD]) & F.LAYOUT_SLOT_ORDER)
    assert slot_order == bool(want["layout"]), "the layout word disagrees with the plan"
    if slot_order:
        assert np.array_equal(np.sort(ws["order_alt"][:P]), np.arange(P)), "order_alt is not a permutation of the slots"
        assert not np.array_equal(ws["order_alt"][:P], np.arange(P))
    nr = fwd["num_rendered"].cpu().numpy().astype(np.int64) & 0xFFFFFFFF
    assert np.array_equal(fwd["radii"].cpu().numpy(), ws["radii"][:, :P])
    report = []
    for f in b["check"]:
        label = f"batched-{name} frame {f}"
        ref = refs[f]
        r, _, _ = _check_frame(label, ws, f, _images(fwd, f), int(nr[f]), ref, ref["kw"], None, slot_order, mask_ties=P > 1000)
        report += [(f"frame {f} {row[0]}",) + row[1:] for row in r]
        print(f"{label} [{bin_algo}]: visible {ref['vis'].sum()} instances {int(nr[f])}")
    fwd2, _ = run()
    ws2 = F.read_workspace(fwd2, P, nF, S, S)
    assert torch.equal(fwd["num_rendered"], fwd2["num_rendered"])
    _same_bits(name + " radii", ws["radii"], ws2["radii"])
    _same_bits(name + " ranges", ws["ranges"], ws2["ranges"])
    _same_bits(name + " lists", ws["ids"][:int(nr.sum())], ws2["ids"][:int(nr.sum())])
    # (the slot table itself may differ between launches: the Morton counting sort hands out the slots of a bin by atomics; it is a
    # locality device, and each launch's records are read through its own table)
    for f in b["check"]:
        of = lambda w: w["order_alt"][:P] if slot_order else np.arange(P)
        v = refs[f]["vis"] & refs[f]["binned"]
        _same_bits(f"{name} frame {f} records", ws["splats"][f][of(ws)][v][:, :12], ws2["splats"][f][of(ws2)][v][:, :12])
    for k in ("color", "alpha", "depth"):
        assert torch.equal(fwd[k], fwd2[k]), f"{name} {k}: a second launch gives other bits"
    F.assert_report(f"batched-{name} [{bin_algo}]", report)
