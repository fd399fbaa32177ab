"""Stage-wise fp64 conformance of the rasteriser backward (csrc/rast_bwd.hip), per Gaussian -- needs an MI355X.

gvf_rast_backward / gvf_rast_backward_batched are called through ctypes on buffers of the test's own, after the package's forward
(rasterizer._rasterize_impl / _rasterize_batched_impl with private_workspace=True) left the workspace they read.  The backward works in two
steps, and each is held against the oracle (oracle/rast_bwd_oracle.c) separately, split at the accumulators:

  stage 1, blend backward    acc_dev against rast64_accumulators on the same inputs, element-wise:
                             e = |acc_dev - acc_ref| / (2^-24 * acc_abs), acc_abs = the sums over absolute per-(pixel, splat) terms.
                             Pixels the forward oracle flags (alpha or test_T within 2e-4 relative of 1/255 resp. 1e-4) get NO upstream
                             gradient, so a decision that falls the other way in fp32 contributes exactly zero on both sides.
  stage 2, chain rule        the device's outputs against rast64_chain(acc_dev.double()): the device's blend decisions are inside acc_dev,
                             nothing discontinuous is left but exact comparisons on the inputs, and the oracle flags the Gaussians
                             within 1e-5 relative of one (they are excluded; at most 1 % of the visible ones, asserted).  Per output tensor
                             and Gaussian row i:  e_i = ||got_i - ref_i||_2 / (2^-24 * scale_i),
                             scale_i = sum_k |acc_dev[i, k]| * ||chain(e_k)_i||_2 from the Jacobian columns; rows with scale_i = 0
                             (invisible Gaussians, SH coefficients above the active degree) must be exactly zero.
  batched                    per delta slice the reference sums rast64_chain(acc_dev[f]) over the slice's frames on the fp64-activated
                             values (rast_bwd_ref.activate64), applies the fp64 activation Jacobian (the slice's dL_ddelta row) and sums
                             into the raw-parameter gradients; the row scales go through the same Jacobian.

Accumulator layout (an implementation detail this test relies on, also stated in DESIGN.md): after the call returns, the caller's scratch
holds the accumulators in its first P * 10 floats as [P][10] -- [F][P][10] for the batched call -- in the order d/d(x, y) [pixels],
d/d(conic a, b, c), d/d(opacity_eff), d/d(r, g, b), d/d(depth).

Bar, both stages, per case and tensor: the device's maximum and 99th percentile of e are each <= 4 x those of the fp32 yardstick (the
oracle's formulas compiled in single precision, gvfo32_*) on the same inputs -- for stage 2 the yardstick gets the same acc_dev.  Why 4 x:
the project grants 2 x over the yardstick on block norms for "another summation order, not another algorithm"; element-wise maxima are
heavier-tailed than block norms, and the device adds hardware exp2 / log2 / reciprocal at about 1 ulp each and wave-reduced partial sums
before the atomics; like the yardstick it reconstructs T by dividing by 1 - alpha.  The bar is never measured against the device.

Conditions, all from the oracle alone and asserted: flagged pixels <= 3 %; the forward's radii equal the oracle's; no two visible
Gaussians that share a tile have depths within 4 fp32 ulps; flagged Gaussians <= 1 % of the visible ones; wide scenes hold >= 20 clamped
visible Gaussians; the crowded scene puts more than 512 instances on one tile.

Also per case: NaN guard rows around every output and a byte pattern around the scratch stay untouched; a second launch reproduces the
accumulators within the stage-1 bar (the atomics' order is free), and wherever a Gaussian's accumulators came out with identical bits in
the two launches its outputs have identical bits too (the chain rule is a fixed-order function of them: the library has no entry point
that runs the chain alone on a scratch snapshot, so this is checked row by row).

Measured on an MI355X (device max/p99 : yardstick max/p99, worst ratio over the tensors of the case; `-s` prints every figure):
  case                        stage 1 (acc) device : yardstick   ratio   stage 2, worst tensor  device : yardstick   ratio
  narrow-mip-sh0                 280.7/71.6 : 282.3/68.3         1.05    opacities      14.3/5.1 : 12.2/6.3          1.17
  narrow-mip-sh1                 430.4/67.5 : 427.8/69.2         1.01    shs             1.7/1.4 : 1.7/1.4           1.00
  narrow-mip-sh2                 953.5/75.8 : 949.6/73.0         1.04    opacities      17.2/8.6 : 17.2/7.1          1.21
  narrow-mip-sh3               43827/77.2   : 43828/75.0         1.03    scales         15.4/7.7 : 11.8/8.2          1.31
  narrow-dilate-sh0               78.4/39.0 : 80.9/38.7          1.01    means3D         3.3/2.4 : 3.3/2.4           1.00
  narrow-dilate-sh1               84.5/37.9 : 79.6/37.2          1.06    scales          7.2/5.8 : 7.8/5.5           1.04
  narrow-dilate-sh2              111.9/39.9 : 111.9/38.5         1.04    scales         11.3/6.5 : 10.8/7.6          1.05
  narrow-dilate-sh3               86.7/39.1 : 69.6/36.9          1.25    scales         10.6/5.9 : 10.6/5.3          1.12
  p97                           1800/69.4   : 1801/71.8          1.00    means3D         2.3/1.9 : 2.3/1.9           1.00
  p257                            86.5/25.5 : 87.9/23.6          1.08    rotations       6.9/5.8 : 6.9/5.5           1.06
  wide-mip                       224.7/25.2 : 231.8/27.1         0.97    scales         52.0/17.3 : 27.1/15.9        1.92
  wide-dilate-sh3                 99.7/15.3 : 95.6/15.6          1.04    means3D        19.9/7.3 : 10.3/5.2          1.94
  nonsquare-40x72               2096/102.0  : 2097/104.6         1.00    scales         18.8/10.4 : 18.8/8.4         1.23
  scale-modifier-1.3             345.0/58.9 : 349.9/56.6         1.04    opacities      10.5/6.7 : 7.6/5.5           1.39
  precomputed                   7906/70.8   : 7900/71.1          1.00    cov3D_precomp  13.6/9.9 : 19.4/6.0          1.66
  precomputed-dilate              83.4/38.2 : 77.3/35.9          1.08    means3D         3.5/2.7 : 3.5/2.7           1.00
  subpixel                      3228/84.2   : 3224/83.0          1.01    scales         12.7/10.7 : 12.6/8.6         1.25
  crowded                         29.9/11.1 : 25.2/10.9          1.19    rotations      10.5/8.1 : 10.5/7.5          1.07
  single-gaussian-mode0            7.4/7.3  : 4.2/4.0            1.83    means3D         2.6/2.6 : 2.6/2.6           1.00
  single-gaussian-mode1            0.7/0.7  : 3.8/3.7            0.19    means3D         2.2/2.2 : 2.2/2.2           1.00
  batched-softplus-sh0         21796/76.2   : 21796/75.3         1.01    opacity        11.9/5.6 : 12.3/5.0          1.12
  batched-softplus-sh2         21874/75.5   : 21873/73.5         1.03    delta.scale   780.0/20.7 : 780.3/18.3       1.13
  batched-exp-sh0               4027/83.4   : 4027/82.9          1.01    scaling        13.0/8.6 : 14.6/6.9          1.24
  batched-exp-sh2              52976/71.8   : 52980/69.9         1.03    delta.rgb     146.9/9.7 : 91.0/9.7          1.61
  batched-shared-activation   212366/88.9   : 212360/86.4        1.03    rotation      244.5/28.7 : 211.2/27.9       1.16
Every ratio is <= 1.94.  The large stage-1 maxima (both sides alike) are single elements where a Gaussian's centre lies within 1e-4 px of a
pixel row or column: dx = x - px cancels, and any fp32 evaluation of x is off by one rounding of a number ~30 while acc_abs counts |dx|.
Two launches: 75 .. 100 % of the Gaussians came out with bit-identical accumulators (26 % in the crowded scene), outputs identical there.
"""
import ctypes
import math

import numpy as np
import pytest
import torch

import oracle
import rast_bwd_ref as R
from gvfdiffusion_amd import _lib, synthetic
from gvfdiffusion_amd import rasterizer as _r
from rast_util import cached, camera_block

pytestmark = pytest.mark.gpu
GUARD = 64                         # NaN rows on either side of every output
PAD = 4096                         # pattern bytes on either side of the scratch
PATTERN = 0xA5


# ---- buffers ------------------------------------------------------------------------------------------------------------------------
class Guarded:
    """A (rows, width) fp32 output with GUARD NaN rows before and after it; the payload is NaN-filled too (every element must be written)."""

    def __init__(self, rows, width, dev):
        self.rows, self.width = rows, max(1, width)
        self.buf = torch.full(((rows + 2 * GUARD) * self.width,), float("nan"), dtype=torch.float32, device=dev)

    @property
    def payload(self):
        return self.buf[GUARD * self.width:(GUARD + self.rows) * self.width]

    def ptr(self):
        return ctypes.c_void_p(self.payload.data_ptr())

    def read(self):
        lo, hi = self.buf[:GUARD * self.width], self.buf[(GUARD + self.rows) * self.width:]
        assert bool(torch.isnan(lo).all()) and bool(torch.isnan(hi).all()), "a guard row was written"
        out = self.payload.cpu().numpy().reshape(self.rows, self.width)
        assert np.isfinite(out).all(), "an output element was left unwritten or is not finite"
        return out


class Scratch:
    def __init__(self, nbytes, dev):
        self.nbytes = nbytes
        self.buf = torch.full((nbytes + 2 * PAD + 256,), PATTERN, dtype=torch.uint8, device=dev)
        self.off = (-(self.buf.data_ptr() + PAD)) % 256 + PAD
        self.base = self.buf.data_ptr() + self.off

    def floats(self, n):
        raw = self.buf[self.off:self.off + 4 * n].cpu().numpy()
        return raw.view(np.float32).copy()

    def check_guards(self):
        assert bool((self.buf[:self.off] == PATTERN).all()) and bool((self.buf[self.off + self.nbytes:] == PATTERN).all()), \
            "the backward wrote outside the scratch size it reported"


def _t(a, dev):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(dev)


def _kw_from(st, fr):
    """The oracle's scene keywords read back from the structs the device gets (their fp32 fields, not the doubles they were set from)."""
    return dict(H=st.image_height, W=st.image_width, tanfovx=float(fr.tanfovx), tanfovy=float(fr.tanfovy), kernel_size=float(st.kernel_size),
                scale_modifier=float(st.scale_modifier), viewmatrix=np.array(list(fr.viewmatrix), np.float32),
                projmatrix=np.array(list(fr.projmatrix), np.float32), campos=np.array(list(fr.campos), np.float32),
                sh_degree=st.sh_degree, bg=np.array(list(st.bg), np.float32), mode=st.mode)


def _structs(c, delta_index=-1):
    kw = c.kw
    st = _r.make_settings(c.H, c.W, c.deg, c.mode, kw["kernel_size"], kw["scale_modifier"], [float(x) for x in kw["bg"]])
    fr = _r.make_frame(torch.from_numpy(np.asarray(kw["viewmatrix"], np.float32)), torch.from_numpy(np.asarray(kw["projmatrix"], np.float32)),
                       torch.from_numpy(np.asarray(kw["campos"], np.float32)), kw["tanfovx"], kw["tanfovy"], delta_index)
    return st, fr


# ---- the bar ------------------------------------------------------------------------------------------------------------------------
def _judge(label, tensor, dev_stats, yard_stats, report):
    ratio = max(dev_stats[0] / yard_stats[0] if yard_stats[0] > 0 else (0.0 if dev_stats[0] == 0 else math.inf),
                dev_stats[1] / yard_stats[1] if yard_stats[1] > 0 else (0.0 if dev_stats[1] == 0 else math.inf))
    print(f"{label} {tensor}: device max/p99 {dev_stats[0]:.2f}/{dev_stats[1]:.2f}  yardstick {yard_stats[0]:.2f}/{yard_stats[1]:.2f}  "
          f"ratio {ratio:.2f}")
    report.append((tensor, dev_stats, yard_stats, ratio))


def _assert_report(label, report):
    bad = [(t, d, y, r) for t, d, y, r in report if not R.within(d, y)]
    assert not bad, f"{label}: beyond {R.FACTOR} x the fp32 yardstick: " + "; ".join(
        f"{t} device {d[0]:.2f}/{d[1]:.2f} yardstick {y[0]:.2f}/{y[1]:.2f} ratio {r:.2f}" for t, d, y, r in bad)


def _stage1(label, acc_dev, A64, A32, report, tensor="acc"):
    ref, scale = A64["acc"], A64["acc_abs"]
    nz = scale > 0
    assert (acc_dev[~nz] == 0).all(), f"{label}: an accumulator no splat contributes to is not exactly zero"
    e_dev = np.abs(acc_dev.astype(np.float64) - ref)[nz] / (R.U * scale[nz])
    e_yard = np.abs(A32["acc"].astype(np.float64) - ref)[nz] / (R.U * scale[nz])
    if e_dev.size and e_dev.max() > R.FACTOR * e_yard.max():
        i, k = np.argwhere(nz)[int(np.argmax(e_dev))]
        print(f"{label}: worst accumulator element: Gaussian {i}, component {k}: device {acc_dev[i, k]!r} reference {ref[i, k]!r}")
    _judge(label, tensor, R.stats(e_dev), R.stats(e_yard), report)


# ---- single frame -------------------------------------------------------------------------------------------------------------------
def _launch_single(c, st, fr, dev, fwd, tensors):
    m3, sh, col, op, sc, ro, c6, sub = tensors
    P = c.P
    M = 0 if sh is None else sh.shape[1]
    nb = ctypes.c_size_t(0)
    _lib.check(_lib.lib().gvf_rast_backward_scratch_bytes(P, ctypes.byref(nb)), "gvf_rast_backward_scratch_bytes")
    scratch = Scratch(int(nb.value), dev)
    outs = dict(means3D=Guarded(P, 3, dev), means2D=Guarded(P, 2, dev), opacities=Guarded(P, 1, dev),
                shs=Guarded(P, M * 3, dev) if sh is not None else None, colors_precomp=Guarded(P, 3, dev) if col is not None else None,
                scales=Guarded(P, 3, dev) if sc is not None else None, rotations=Guarded(P, 4, dev) if ro is not None else None,
                cov3D_precomp=Guarded(P, 6, dev) if c6 is not None else None)
    p = lambda k: None if outs[k] is None else outs[k].ptr()
    base = (fwd["workspace"].data_ptr() + 255) // 256 * 256
    wc, wa, wd = _t(c.wc, dev), _t(c.wa, dev), _t(c.wd, dev)            # held until the call has finished
    rc = _lib.lib().gvf_rast_backward(
        ctypes.byref(st), ctypes.byref(fr), P, M, _lib.ptr(m3), _lib.ptr(sh), _lib.ptr(col), _lib.ptr(op), _lib.ptr(sc), _lib.ptr(ro),
        _lib.ptr(c6), _lib.ptr(sub), ctypes.c_void_p(base), fwd["workspace_bytes"], fwd["max_rendered"], _lib.ptr(wc),
        _lib.ptr(wa), _lib.ptr(wd), ctypes.c_void_p(scratch.base), scratch.nbytes, p("means3D"), p("means2D"),
        p("shs"), p("colors_precomp"), p("opacities"), p("scales"), p("rotations"), p("cov3D_precomp"), _lib.current_stream(dev))
    _lib.check(rc, "gvf_rast_backward")
    torch.cuda.synchronize(dev)
    scratch.check_guards()
    acc = scratch.floats(P * 10).reshape(P, 10)
    return acc, {k: v.read() for k, v in outs.items() if v is not None}


def _reference_single(c):
    """Everything that comes from the oracle alone, computed once per case: conditions, stage-1 reference and yardstick, Jacobian columns."""
    fl = R.pixel_flags(c)
    frac = R.zero_flagged(c, fl["flags"])
    A64 = oracle.rast64_accumulators(*c.ins, c.wc, c.wa, c.wd, subpixel_offset=c.sub, **c.kw)
    A32 = oracle.rast32_accumulators(*c.ins, c.wc, c.wa, c.wd, subpixel_offset=c.sub, **c.kw)
    proj = oracle.rast64_project(*c.ins, **c.kw)
    vis = (proj["flags"] & oracle.FLAG_VISIBLE) != 0
    ties = R.depth_ties(A64["rects"], proj["out"][:, 9], vis)
    cols = R.jacobian_columns(c.ins, c.kw)
    return dict(frac=frac, A64=A64, A32=A32, flags=proj["flags"], ties=ties, cols=cols, radii=fl["radii"])


def _check_single(c, label, dev, min_clamped=0):
    st, fr = _structs(c)
    c.kw = _kw_from(st, fr)
    ref = cached(("rast_bwd_conformance", label), lambda: _reference_single(c))
    c.wc, c.wa, c.wd = ref.setdefault("grads", (c.wc, c.wa, c.wd))        # the gradients with the flagged pixels zeroed
    fl = ref["flags"]
    vis, near, clamped = (fl & oracle.FLAG_VISIBLE) != 0, (fl & oracle.FLAG_NEAR) != 0, (fl & oracle.FLAG_CLAMPED) != 0
    # conditions, from the oracle alone
    assert ref["frac"] <= 0.03, f"{ref['frac']:.4f} of the pixels are threshold-flagged"
    assert not ref["ties"], f"visible Gaussians sharing a tile with depths within 4 fp32 ulps: {ref['ties']}"
    assert (near & vis).sum() <= 0.01 * vis.sum(), f"{(near & vis).sum()} of {vis.sum()} visible Gaussians sit at a threshold"
    assert np.array_equal(ref["A64"]["radii"], ref["A32"]["radii"]) and np.array_equal(ref["A64"]["radii"], ref["radii"])
    assert (clamped & vis).sum() >= min_clamped, f"only {(clamped & vis).sum()} clamped visible Gaussians"
    print(f"{label}: P={c.P} {c.H}x{c.W} visible {vis.sum()} clamped {(clamped & vis).sum()} flagged Gaussians {(near & vis).sum()} "
          f"flagged pixels {ref['frac']:.4f}")

    tensors = tuple(_t(a, dev) for a in c.ins) + (_t(c.sub, dev),)
    m3, sh, col, op, sc, ro, c6, sub = tensors
    fwd = _r._rasterize_impl(st, fr, m3, op, sh, col, sc, ro, c6, sub, c.mode == 1, private_workspace=True)
    assert np.array_equal(fwd["radii"].cpu().numpy(), ref["A64"]["radii"]), "the forward's radii differ from the oracle's"
    acc1, out1 = _launch_single(c, st, fr, dev, fwd, tensors)
    acc2, out2 = _launch_single(c, st, fr, dev, fwd, tensors)

    report = []
    _stage1(label, acc1, ref["A64"], ref["A32"], report)
    _stage1(label + " (second launch)", acc2, ref["A64"], ref["A32"], report)
    # stage 2 from the device's own accumulators
    want = oracle.rast64_chain(*c.ins, acc1.astype(np.float64), **c.kw)
    yard = oracle.rast32_chain(*c.ins, acc1, **c.kw)
    scale = R.row_scale(acc1, ref["cols"])
    keep = ~near
    for name, got in out1.items():
        e_dev, dead = R.row_err(got, want[name], scale[name])
        e_yard, _ = R.row_err(yard[name], want[name], scale[name])
        assert dead == 0.0, f"{label} {name}: a row without any contribution is not exactly zero"
        if name == "shs":                                               # coefficients above the active degree: exact zeros
            assert (got.reshape(c.P, -1, 3)[:, (c.deg + 1) ** 2:] == 0).all()
        sd, sy = R.stats(e_dev[keep]), R.stats(e_yard[keep])
        if not R.within(sd, sy):
            i = int(np.nanargmax(np.where(keep, e_dev, np.nan)))
            print(f"{label} {name}: worst row: Gaussian {i} e={e_dev[i]:.1f} device {got[i]} reference {np.asarray(want[name]).reshape(c.P, -1)[i]}")
        _judge(label, name, sd, sy, report)
    # identical accumulators -> identical outputs, bit for bit
    same = (acc1.view(np.uint32) == acc2.view(np.uint32)).all(axis=1)
    for name in out1:
        assert np.array_equal(out1[name].view(np.uint32)[same], out2[name].view(np.uint32)[same]), f"{label} {name}: not reproducible"
    print(f"{label}: {same.sum()} of {c.P} accumulator rows bit-identical across the two launches")
    _assert_report(label, report)
    return out1, acc1


SINGLE = {
    # narrow scenes (means3D x 0.8, scales 0.004 .. 0.04): every SH degree, both modes; mode 1 carries alpha and depth gradients
    "narrow-mip-sh0": dict(P=600, H=64, W=64, deg=0, mode=0, seed=5),
    "narrow-mip-sh1": dict(P=600, H=64, W=64, deg=1, mode=0, seed=27),
    "narrow-mip-sh2": dict(P=600, H=64, W=64, deg=2, mode=0, seed=7),
    "narrow-mip-sh3": dict(P=600, H=64, W=64, deg=3, mode=0, seed=8),
    "narrow-dilate-sh0": dict(P=600, H=64, W=64, deg=0, mode=1, seed=9),
    "narrow-dilate-sh1": dict(P=600, H=64, W=64, deg=1, mode=1, seed=10),
    "narrow-dilate-sh2": dict(P=600, H=64, W=64, deg=2, mode=1, seed=11),
    "narrow-dilate-sh3": dict(P=600, H=64, W=64, deg=3, mode=1, seed=32),
    # the last preprocess workgroup is partial
    "p97": dict(P=97, H=32, W=32, deg=1, mode=0, seed=13),
    "p257": dict(P=257, H=32, W=32, deg=2, mode=1, seed=14),
    # wide scenes (means3D x 2.4, scales 0.02 .. 0.25): the clamped EWA branch
    "wide-mip": dict(P=600, H=64, W=80, deg=1, mode=0, seed=15, wide=True),
    "wide-dilate-sh3": dict(P=400, H=48, W=48, deg=3, mode=1, seed=16, wide=True),
    "nonsquare-40x72": dict(P=600, H=40, W=72, deg=2, mode=0, seed=17),
    "scale-modifier-1.3": dict(P=600, H=64, W=64, deg=1, mode=0, seed=18, scale_modifier=1.3),
    "precomputed": dict(P=600, H=64, W=64, deg=0, mode=0, seed=19, precomp=True),
    "precomputed-dilate": dict(P=600, H=64, W=64, deg=0, mode=1, seed=20, precomp=True),
    "subpixel": dict(P=600, H=64, W=64, deg=1, mode=0, seed=21, subpixel=True),
    # 32 x 32, low opacity: more than 512 instances on one tile, three staging rounds in both phases of the blend backward
    "crowded": dict(P=700, H=32, W=32, deg=1, mode=0, seed=22, crowded=True),
}


@pytest.mark.parametrize("name", list(SINGLE))
def test_single_frame(cuda, oracle_lib, name):
    c = R.make_case(**SINGLE[name])
    if name == "crowded":
        tight = oracle.rast_render(*c.ins, tight=True, **c.kw)["num_rendered"]
        assert tight / 4 > 512, f"{tight} instances over 4 tiles"          # the fullest of the four tiles holds at least the mean
    _check_single(c, name, cuda, min_clamped=20 if name.startswith("wide") else 0)


@pytest.mark.parametrize("mode", [0, 1])
def test_single_gaussian_closed_form(cuda, oracle_lib, mode):
    """P = 1, the isotropic Gaussian on the optical axis of tests/test_oracle_rast_closed_form.py: colour = c a + bg (1 - a), a = o coef g(x),
    so dL/dc_k = sum_x w_k a and dL/do = sum_x sum_k w_k (c_k - bg_k) coef g over the pixels with a >= 1/255, and no pull on the mean for
    a symmetric weight.  Tolerance: the closed form's own 1e-6 (the CPU test of the oracle) plus 64 roundings of the absolute sum -- the
    exponent is at most ln(0.7 * 255) = 5.2 and comes from a conic ~10 fp32 operations deep (5.2 * 10 roundings), the rest is the alpha / T
    products and the sum."""
    import test_oracle_rast_closed_form as cf
    c = R.make_case(P=1, H=cf.H, W=cf.W, deg=0, mode=0 if mode == 0 else 1, seed=1, single=True)
    yy, xx = np.mgrid[0:cf.H, 0:cf.W]
    d2 = (xx - 15.5) ** 2 + (yy - 15.5) ** 2
    c.wc = np.stack([1.0 + 0.01 * d2, 2.0 - 0.02 * d2, 0.5 + 0.0 * d2]).astype(np.float32)
    c.wa = c.wd = None
    out, _ = _check_single(c, f"single-gaussian-mode{mode}", cuda)
    op, col, bg = 0.7, np.array([0.9, 0.3, 0.1]), np.array([0.2, 0.4, 0.6])
    sig2, coef = cf._sigma2(c.cam, 0.08, 2.0, mode, 0.1)
    a = op * coef * np.exp(-0.5 * d2 / sig2)
    reach = a >= 1.0 / 255.0
    w = c.wc.astype(np.float64)
    exp_dcol, abs_dcol = (w * (a * reach)[None]).sum(axis=(1, 2)), (np.abs(w) * (a * reach)[None]).sum(axis=(1, 2))
    terms = (w * (col - bg)[:, None, None]) * (coef * np.exp(-0.5 * d2 / sig2) * reach)[None]
    tol = 1e-6 + 64 * R.U
    assert (np.abs(out["colors_precomp"][0] - exp_dcol) <= tol * abs_dcol).all()
    assert abs(out["opacities"][0, 0] - terms.sum()) <= tol * np.abs(terms).sum()
    assert np.abs(out["means2D"][0]).max() <= tol * np.abs(terms).sum() * 0.5 * cf.W


# ---- batched ------------------------------------------------------------------------------------------------------------------------
RAW = ("xyz", "fdc", "scaling", "rotation", "opacity")
DELTA_PARTS = {"delta.xyz": slice(0, 3), "delta.scale": slice(3, 6), "delta.rot": slice(6, 10), "delta.rgb": slice(10, 13), "delta.op": slice(13, 14)}
ACT_ORDER = ("means3D", "shs", "opacities", "scales", "rotations")


def _batched_case(P, S, deg, activation, di, n_delta, seed, big_scales=0):
    attrs = synthetic.random_gaussians(P, sh_degree=deg, seed=seed, scale_lo=0.004, scale_hi=0.04)
    attrs["means3D"] = attrs["means3D"] * 0.8
    attrs["opacities"] = attrs["opacities"].clamp(0.02, 0.95)
    gm = synthetic.gaussian_model_from(attrs, deg, torch.device("cpu"), scaling_activation=activation)
    raw = dict(xyz=gm._xyz, fdc=gm._features_dc, scaling=gm._scaling, rotation=gm._rotation, opacity=gm._opacity)
    raw = {k: v.detach().float().contiguous().clone() for k, v in raw.items()}
    if big_scales:
        # a few raw scales above softplus' linear threshold of 20: blobs of ~20 world units that fill every frame.  All three axes, so that
        # the footprint stays well conditioned (a needle of 20 x 0.01 loses its 2-D determinant to cancellation in any fp32 evaluation), and
        # faint (opacity 0.03), so that the rest of the scene still shows through
        raw["scaling"][:big_scales] = 20.3 + torch.rand((big_scales, 3), generator=torch.Generator().manual_seed(seed)) - float(gm.scale_bias)
        raw["opacity"][:big_scales] = math.log(0.03 / 0.97) - float(gm.opacity_bias)
    delta = synthetic.random_deltas(n_delta, P, seed=seed + 1, std=0.01)
    cams = [camera_block(azi=360.0 * f / len(di) + 7.0, elev=10.0 - 3.0 * (f % 3)) for f in range(len(di))]
    g = np.random.default_rng(seed + 1000)
    wc = g.standard_normal((len(di), 3, S, S)).astype(np.float32)
    act_kw = dict(aabb=gm.aabb.tolist(), scale_bias=float(gm.scale_bias), opacity_bias=float(gm.opacity_bias),
                  min_kernel_size=float(gm.mininum_kernel_size), scaling_activation=activation)
    return dict(P=P, S=S, deg=deg, di=list(di), raw=raw, delta=delta, cams=cams, wc=wc, act_kw=act_kw, act_struct=gm.activation_struct(), gm=gm)


def _activated(b, prec):
    """Per delta slice (in order of first use, -1 = static): the activated values with autograd leaves.  prec 64: activate64 (the
    reference); prec 32: the package's own fp32 torch functions (the yardstick: a naive fp32 composition)."""
    dt = torch.float64 if prec == 64 else torch.float32
    leaves = {k: v.to(dt).clone().requires_grad_(True) for k, v in b["raw"].items()}
    dleaf = b["delta"].to(dt).clone().requires_grad_(True)
    slices = []
    for d in b["di"]:
        if d not in slices:
            slices.append(d)
    acts = {}
    for s in slices:
        drow = dleaf[s] if s >= 0 else None
        if prec == 64:
            acts[s] = R.activate64(leaves["xyz"], leaves["fdc"], leaves["scaling"], leaves["rotation"], leaves["opacity"], drow, **b["act_kw"])
        else:
            gm = b["gm"]
            gm._xyz, gm._features_dc, gm._scaling, gm._rotation, gm._opacity = (leaves[k] for k in RAW)
            z = torch.zeros((b["P"], 14)) if drow is None else drow
            acts[s] = dict(means3D=gm.get_xyz_with_delta(z[:, :3]), shs=gm.get_features_with_delta(z[:, 10:13].unsqueeze(1)),
                           opacities=gm.get_opacity_with_delta(z[:, 13:]), scales=gm.get_scaling_with_delta(z[:, 3:6]),
                           rotations=gm.get_rotation_with_delta(z[:, 6:10]))
    return leaves, dleaf, acts


def _ins_of(act):
    n = lambda t: t.detach().numpy()
    return (n(act["means3D"]), n(act["shs"]), None, n(act["opacities"]).reshape(-1), n(act["scales"]), n(act["rotations"]), None)


def _pull_back(b, prec, kws, frame_grads):
    """frame_grads(f, ins) -> the chain's dict for frame f on activated inputs `ins`; returns the gradients of the raw parameters and of the
    delta parts after the activation Jacobian, as fp64 numpy."""
    leaves, dleaf, acts = _activated(b, prec)
    outs, gouts = [], []
    for f, d in enumerate(b["di"]):
        act = acts[d]
        g = frame_grads(f, _ins_of(act))
        for k in ACT_ORDER:
            outs.append(act[k])
            gouts.append(torch.as_tensor(np.asarray(g[k]).reshape(act[k].shape), dtype=act[k].dtype))
    torch.autograd.backward(outs, gouts)
    res = {k: (leaves[k].grad if leaves[k].grad is not None else torch.zeros_like(leaves[k])).double().numpy().reshape(b["P"], -1) for k in RAW}
    dg = (dleaf.grad if dleaf.grad is not None else torch.zeros_like(dleaf)).double().numpy()
    for name, sl in DELTA_PARTS.items():
        res[name] = dg[:, :, sl].reshape(-1, sl.stop - sl.start)       # rows (slice, Gaussian)
    return res


def _reference_batched(b, st, frames, mask_ties=False):
    """mask_ties: instead of demanding a scene without depth ties, give no upstream gradient to the pixels at which both Gaussians of a
    tied pair can be composited (alpha >= 0.9 / 255 for both, in tiles they share) -- as for threshold-flagged pixels: whichever order the
    pair is blended in, it contributes exactly zero there; where only one of the two is composited their order does not matter."""
    F = len(b["di"])
    kws = [_kw_from(st, fr) for fr in frames]
    _, _, act64 = _activated(b, 64)
    _, _, act32 = _activated(b, 32)
    ref = dict(kws=kws, A64=[], A32=[], frac=[], ties=[], flags=[], radii=[])
    wc = b["wc"].copy()
    for f, d in enumerate(b["di"]):
        i64, i32 = _ins_of(act64[d]), _ins_of(act32[d])
        fl = oracle.rast_render(*i32, **kws[f])
        m = fl["flags"] != 0
        proj = oracle.rast64_project(*i64, **kws[f])
        vis = (proj["flags"] & oracle.FLAG_VISIBLE) != 0
        rects = oracle.rast64_accumulators(*i64, wc[f], **kws[f])["rects"] if mask_ties else None
        ties = R.depth_ties(rects, proj["out"][:, 9], vis) if mask_ties else []
        yy, xx = np.mgrid[0:kws[f]["H"], 0:kws[f]["W"]]
        for i, j in ties:
            both = np.ones(m.shape, bool)
            for g in (proj["out"][i], proj["out"][j]):
                dx, dy = g[0] - xx, g[1] - yy
                both &= g[5] * np.exp(np.minimum(0.0, -0.5 * (g[2] * dx * dx + g[4] * dy * dy) - g[3] * dx * dy)) >= 0.9 / 255.0
            m |= both
        wc[f][:, m] = 0.0
        ref["frac"].append(float(m.mean()))
        ref["radii"].append(fl["radii"])
        ref["A64"].append(oracle.rast64_accumulators(*i64, wc[f], **kws[f]))
        ref["A32"].append(oracle.rast32_accumulators(*i32, wc[f], **kws[f]))
        ref["flags"].append(proj["flags"])
        ref["ties"].append([] if mask_ties else R.depth_ties(ref["A64"][f]["rects"], proj["out"][:, 9], vis))
    ref["wc"] = wc
    ref["act_near"] = np.zeros(b["P"], bool)
    for a in act64.values():
        ref["act_near"] |= R.activation_flags(a)
    return ref


def _launch_batched(b, st, frames, dev, fwd, dt, wc, need):
    P, F, M = b["P"], len(b["di"]), b["raw"]["fdc"].shape[1]
    n_delta = b["delta"].shape[0]
    nb = ctypes.c_size_t(0)
    _lib.check(_lib.lib().gvf_rast_backward_batched_scratch_bytes(P, F, ctypes.byref(nb)), "gvf_rast_backward_batched_scratch_bytes")
    scratch = Scratch(int(nb.value), dev)
    widths = dict(xyz=3, fdc=M * 3, scaling=3, rotation=4, opacity=1)
    outs = {k: Guarded(P, w, dev) for k, w in widths.items()}
    outs["delta"] = Guarded(n_delta * P, 14, dev)
    p = lambda k: outs[k].ptr() if need[k] else None
    arr = (_lib.GvfRastFrame * F)(*frames)
    base = (fwd["workspace"].data_ptr() + 255) // 256 * 256
    rc = _lib.lib().gvf_rast_backward_batched(
        ctypes.byref(st), arr, F, ctypes.byref(b["act_struct"]), P, M, _lib.ptr(dt["xyz"]), _lib.ptr(dt["fdc"]), _lib.ptr(dt["scaling"]),
        _lib.ptr(dt["rotation"]), _lib.ptr(dt["opacity"]), _lib.ptr(dt["delta"]), n_delta, ctypes.c_void_p(base), fwd["workspace_bytes"],
        fwd["max_rendered"], _lib.ptr(wc), None, None, ctypes.c_void_p(scratch.base), scratch.nbytes, p("xyz"), p("fdc"), p("scaling"),
        p("rotation"), p("opacity"), p("delta"), _lib.current_stream(dev))
    _lib.check(rc, "gvf_rast_backward_batched")
    torch.cuda.synchronize(dev)
    scratch.check_guards()
    acc = scratch.floats(F * P * 10).reshape(F, P, 10)
    res = {}
    for k, gbuf in outs.items():
        if need[k]:
            res[k] = gbuf.read()
        else:                                                           # a null output: nothing of ours may have been touched
            assert bool(torch.isnan(gbuf.buf).all()), f"{k}: a buffer that was not passed was written"
    return acc, res


def _check_batched(b, label, dev, expect_shared=None, mask_ties=False):
    P, F, S, deg = b["P"], len(b["di"]), b["S"], b["deg"]
    st = _r.make_settings(S, S, deg, _lib.RAST_MODE_MIP, synthetic.KERNEL_2D, 1.0, (0.3, 0.3, 0.3))
    frames = [_r.make_frame(c["viewmatrix"], c["projmatrix"], c["campos"], c["tanfovx"], c["tanfovy"], d) for c, d in zip(b["cams"], b["di"])]
    ref = cached(("rast_bwd_conformance_batched", label), lambda: _reference_batched(b, st, frames, mask_ties))
    kws = ref["kws"]
    n_vis = n_near = 0
    for f in range(F):
        vis = (ref["flags"][f] & oracle.FLAG_VISIBLE) != 0
        near = ((ref["flags"][f] & oracle.FLAG_NEAR) != 0) | ref["act_near"]
        n_vis += int(vis.sum()); n_near += int((near & vis).sum())
        assert ref["frac"][f] <= 0.03 and not ref["ties"][f], (f, ref["frac"][f], ref["ties"][f])
        assert np.array_equal(ref["A64"][f]["radii"], ref["A32"][f]["radii"]) and np.array_equal(ref["A64"][f]["radii"], ref["radii"][f])
    assert n_near <= 0.01 * n_vis
    print(f"{label}: P={P} F={F} {S}x{S} visible (Gaussian, frame) pairs {n_vis}, flagged {n_near}, flagged pixels {max(ref['frac']):.4f}")

    dt = {k: v.to(dev) for k, v in b["raw"].items()}
    dt["opacity"] = dt["opacity"].reshape(-1).contiguous()
    dt["delta"] = b["delta"].to(dev).contiguous()
    wc = torch.from_numpy(ref["wc"]).to(dev)
    lib = _lib.lib()
    n0 = lib.gvf_rast_shared_activation_calls()
    fwd = _r._rasterize_batched_impl(st, frames, b["act_struct"], dt["xyz"], dt["fdc"], dt["scaling"], dt["rotation"], dt["opacity"], dt["delta"],
                                     False, True, private_workspace=True)
    if expect_shared is not None:
        assert (lib.gvf_rast_shared_activation_calls() > n0) == expect_shared, "the forward did not pick the expected record layout"
    radii = fwd["radii"].cpu().numpy()
    for f in range(F):
        assert np.array_equal(radii[f], ref["A64"][f]["radii"]), f"frame {f}: the forward's radii differ from the oracle's"
    everything = {k: True for k in RAW + ("delta",)}
    acc1, out1 = _launch_batched(b, st, frames, dev, fwd, dt, wc, everything)
    acc2, out2 = _launch_batched(b, st, frames, dev, fwd, dt, wc, everything)
    # detach_static: only the delta gradient is asked for; the other buffers stay untouched, the delta gradient is unchanged
    acc3, out3 = _launch_batched(b, st, frames, dev, fwd, dt, wc, {**{k: False for k in RAW}, "delta": True})
    same13 = (acc1.view(np.uint32) == acc3.view(np.uint32)).all(axis=(0, 2))
    assert np.array_equal(out1["delta"].reshape(-1, P, 14).view(np.uint32)[:, same13], out3["delta"].reshape(-1, P, 14).view(np.uint32)[:, same13])

    report = []
    stack = lambda key, which: dict(acc=np.concatenate([a["acc"] for a in ref[which]]), acc_abs=np.concatenate([a["acc_abs"] for a in ref[which]]))
    _stage1(label, acc1.reshape(F * P, 10), stack("acc", "A64"), stack("acc", "A32"), report)
    _stage1(label + " (second launch)", acc2.reshape(F * P, 10), stack("acc", "A64"), stack("acc", "A32"), report)

    # stage 2: reference, yardstick and row scales, all from the device's accumulators
    want = _pull_back(b, 64, kws, lambda f, ins: oracle.rast64_chain(*ins, acc1[f].astype(np.float64), **kws[f]))
    yard = _pull_back(b, 32, kws, lambda f, ins: oracle.rast32_chain(*ins, acc1[f], **kws[f]))
    scale = {}
    for k in range(10):
        for f in range(F):
            def one_hot(ff, ins, k=k, f=f):
                a = np.zeros((P, 10))
                if ff == f:
                    a[:, k] = 1.0
                    return oracle.rast64_chain(*ins, a, **kws[ff])
                return {n: np.zeros(s) for n, s in zip(ACT_ORDER, ((P, 3), (P, ins[1].shape[1], 3), (P,), (P, 3), (P, 4)))}
            col = _pull_back(b, 64, kws, one_hot)
            for name, v in col.items():
                w = np.abs(acc1[f, :, k].astype(np.float64))
                w = np.tile(w, v.shape[0] // P)
                scale[name] = scale.get(name, 0) + w * np.linalg.norm(v, axis=1)
    got = {k: out1[k] for k in RAW}
    dg = out1["delta"].reshape(-1, P, 14)
    used = sorted({d for d in b["di"] if d >= 0})
    for s in range(dg.shape[0]):
        if s not in used:
            assert (dg[s] == 0).all(), f"delta slice {s}, which no frame selects, is not exactly zero"
    for name, sl in DELTA_PARTS.items():
        got[name] = dg[:, :, sl].reshape(-1, sl.stop - sl.start)
    near_any = ref["act_near"].copy()
    for f in range(F):
        near_any |= (ref["flags"][f] & oracle.FLAG_NEAR) != 0
    for name, g in got.items():
        keep = ~np.tile(near_any, g.shape[0] // P)
        e_dev, dead = R.row_err(g, want[name], scale[name])
        e_yard, _ = R.row_err(yard[name], want[name], scale[name])
        assert dead == 0.0, f"{label} {name}: a row without any contribution is not exactly zero"
        _judge(label, name, R.stats(e_dev[keep]), R.stats(e_yard[keep]), report)
    assert (out1["fdc"].reshape(P, -1, 3)[:, (deg + 1) ** 2:] == 0).all()
    same = (acc1.view(np.uint32) == acc2.view(np.uint32)).all(axis=(0, 2))
    for k in RAW:
        assert np.array_equal(out1[k].view(np.uint32)[same], out2[k].view(np.uint32)[same]), f"{label} {k}: not reproducible"
    assert np.array_equal(out1["delta"].reshape(-1, P, 14).view(np.uint32)[:, same], out2["delta"].reshape(-1, P, 14).view(np.uint32)[:, same])
    print(f"{label}: {same.sum()} of {P} Gaussians with bit-identical accumulators in every frame across the two launches")
    _assert_report(label, report)


BATCHED = {
    # F = 5 over three delta slices, one of them (2) unused, two static frames
    "softplus-sh0": dict(P=600, S=64, deg=0, activation="softplus", di=[0, 1, 0, -1, -1], n_delta=3, seed=71, big_scales=3),
    "softplus-sh2": dict(P=600, S=64, deg=2, activation="softplus", di=[0, 1, 0, -1, -1], n_delta=3, seed=62, big_scales=3),
    "exp-sh0": dict(P=600, S=64, deg=0, activation="exp", di=[0, 1, 0, -1, -1], n_delta=3, seed=73),
    "exp-sh2": dict(P=600, S=64, deg=2, activation="exp", di=[0, 1, 0, -1, -1], n_delta=3, seed=34),
}


@pytest.mark.parametrize("name", list(BATCHED))
def test_batched(cuda, oracle_lib, name):
    _check_batched(_batched_case(**BATCHED[name]), "batched-" + name, cuda)


def test_batched_shared_activation_layout(cuda, oracle_lib):
    """P >= 4096 with F >= 2 x the number of slices: the forward activates once per slice and writes its records in slot order; the backward
    reads `rec_of` there.  With 4096 Gaussians on 16 tiles a scene without depth ties does not exist (about eight tied pairs per frame,
    none of 40 seeds was free of them), so here the pixels at which both Gaussians of a tied pair can be composited are masked out of the
    loss instead, like the flagged pixels;
    the 3 % limit on pixels without gradient holds for both together."""
    b = _batched_case(P=4096, S=64, deg=1, activation="softplus", di=[0, 1, 0, 1], n_delta=2, seed=35)
    _check_batched(b, "batched-shared-activation", cuda, expect_shared=True, mask_ties=True)
