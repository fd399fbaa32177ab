"""Host tests of the two-stage rasteriser-backward oracle (oracle/rast_bwd_oracle.c: gvfo64_accumulators -> gvfo64_chain, their fp32
yardstick gvfo32_*, gvfo64_project) and of the fp64 activation restatement in rast_bwd_ref.py -- the references that
tests/test_rast_bwd_conformance_gpu.py holds the device against.  No GPU.

What pins what:
  * chain(accumulators()) IS rast64_backward, bit for bit (which tests/test_oracle_rast_bwd.py pins by finite differences end to end);
  * chain is linear in the accumulators, so chain(one-hot k) is column k of its Jacobian (the row scales of the conformance bar);
  * chain at FIXED accumulators is the derivative of <acc, project(params)>: central differences of the exported per-Gaussian forward, in a
    wide scene where clamped Gaussians are present.  The three upstream conventions: a clamped view coordinate gets no gradient (project
    holds it fixed: txty_fixed), means2D is in NDC units (checked in closed form), and the gradient passes through the 0.99 alpha clamp
    (that one lives in stage 1: test_gradient_passes_through_the_alpha_clamp);
  * seven one-line mutants of the chain rule each land outside the conformance bar (4 x the fp32 yardstick, per Gaussian row).

Why the old criterion was not enough (test_mutants_land_outside_the_new_bar asserts these figures' side of 2e-3): whole-tensor relative L2
of the means3D gradient, mutant against original, in the scene of test_gradients_match_double_oracle[0-3-64-64-500]
    one SH basis derivative wrong (db[6][2]: 4z -> 2z)   2.4e-4   passes 2e-3 by 8 x
    tx, ty terms of dtz dropped                          1.9e-3   passes
    clamp multipliers xmul / ymul ignored                0        passes (no Gaussian of that scene is clamped)
while the worst per-Gaussian row is off by 3e-2 .. 1.5e-1 of its own scale.  Per row, in units of 2^-24 * scale_i, the fp32 yardstick
stays below ~10 and the mutants reach 1e4 .. 1e7 (printed with -s).
"""
import numpy as np
import pytest
import torch

import oracle
import rast_bwd_ref as R
from gvfdiffusion_amd import synthetic

rel = lambda a, b: float(np.linalg.norm(np.asarray(a, np.float64) - b) / max(1e-30, np.linalg.norm(b)))

CASES = [dict(P=300, H=48, W=48, deg=0, mode=0, seed=5), dict(P=300, H=48, W=48, deg=1, mode=1, seed=6),
         dict(P=300, H=48, W=40, deg=2, mode=0, seed=7), dict(P=300, H=48, W=48, deg=3, mode=1, seed=8),
         dict(P=300, H=48, W=48, deg=0, mode=0, seed=9, precomp=True), dict(P=300, H=48, W=48, deg=0, mode=1, seed=10, precomp=True)]


@pytest.mark.parametrize("case", CASES, ids=lambda c: "-".join(f"{k}{v}" for k, v in c.items() if k not in ("P", "H")))
def test_backward_is_the_composition_of_its_stages(case):
    c = R.make_case(**case)
    whole = oracle.rast64_backward(*c.ins, c.wc, c.wa, c.wd, **c.kw)
    A = oracle.rast64_accumulators(*c.ins, c.wc, c.wa, c.wd, **c.kw)
    parts = oracle.rast64_chain(*c.ins, A["acc"], **c.kw)
    for k, v in whole.items():
        if v is None:
            assert parts[k] is None
        else:
            assert np.array_equal(v.view(np.uint64), parts[k].view(np.uint64)), k
    vis = (parts["flags"] & oracle.FLAG_VISIBLE) != 0
    assert (A["radii"] > 0).sum() == vis.sum() > 100
    # acc_abs bounds acc term by term, and is zero exactly where no splat was composited
    assert (np.abs(A["acc"]) <= A["acc_abs"] * (1 + 1e-12)).all() and (A["acc_abs"] >= 0).all()
    assert (A["acc_abs"][~vis] == 0).all()


def test_chain_is_linear_in_the_accumulators():
    c = R.make_case(P=400, H=48, W=48, deg=2, mode=0, seed=3, wide=True)
    g = np.random.default_rng(0)
    a1, a2 = g.standard_normal((c.P, 10)), g.standard_normal((c.P, 10))
    o1, o2 = oracle.rast64_chain(*c.ins, a1, **c.kw), oracle.rast64_chain(*c.ins, a2, **c.kw)
    o12 = oracle.rast64_chain(*c.ins, 0.75 * a1 - 2.0 * a2, **c.kw)
    cols = R.jacobian_columns(c.ins, c.kw)
    for k in ("means3D", "means2D", "shs", "opacities", "scales", "rotations", "cov3D_precomp"):
        lin = 0.75 * o1[k] - 2.0 * o2[k]
        assert np.abs(o12[k] - lin).max() <= 1e-12 * max(1.0, np.abs(lin).max()), k
        # the one-hot responses are the Jacobian's columns: J a1 reassembles chain(a1)
        ja = np.einsum("ik,kin->in", a1, cols[k]).reshape(o1[k].shape)
        assert np.abs(ja - o1[k]).max() <= 1e-12 * max(1.0, np.abs(o1[k]).max()), k


_EPS_FLOOR = dict(means3D=1.0, shs=1.0, colors_precomp=1.0, opacities=1.0, scales=1e-2, rotations=1.0, cov3D_precomp=1e-4)


@pytest.mark.parametrize("mode,deg,precomp", [(0, 2, False), (1, 3, False), (0, 0, True)])
def test_chain_is_the_derivative_of_the_projection_at_fixed_accumulators(mode, deg, precomp):
    c = R.make_case(P=600, H=64, W=80, deg=deg, mode=mode, seed=12 + deg, wide=True, precomp=precomp, scale_modifier=1.3)
    ins = [None if v is None else v.astype(np.float64) for v in c.ins]
    acc = np.random.default_rng(4).standard_normal((c.P, 10))
    base = oracle.rast64_project(*ins, **c.kw)
    fl = base["flags"]
    vis, clamped = (fl & oracle.FLAG_VISIBLE) != 0, (fl & oracle.FLAG_CLAMPED) != 0
    assert (vis & clamped).sum() >= 20, "the wide scene holds no clamped, visible Gaussians"
    got = oracle.rast64_chain(*ins, acc, **c.kw)
    cols = R.jacobian_columns(tuple(ins), c.kw)
    scale = R.row_scale(acc, cols)
    L = lambda p: (acc * p["out"]).sum(axis=1)                      # one value per Gaussian: the rows are independent
    checked = 0
    for t, name in enumerate(R.ORDER):
        if ins[t] is None:
            continue
        x = ins[t].reshape(c.P, -1)
        g = got[name].reshape(c.P, -1)
        worst = 0.0
        for j in range(x.shape[1]):
            old = x[:, j].copy()
            eps = 1e-6 * np.maximum(np.abs(old), _EPS_FLOOR[name])
            x[:, j] = old + eps; hi = oracle.rast64_project(*ins, txty_fixed=base["txty"], **c.kw)
            x[:, j] = old - eps; lo = oracle.rast64_project(*ins, txty_fixed=base["txty"], **c.kw)
            x[:, j] = old
            fd = (L(hi) - L(lo)) / (2 * eps)
            # rows whose visibility, clamp state or threshold margin changes inside the interval say nothing about the derivative
            ok = vis & (hi["flags"] == fl) & (lo["flags"] == fl) & ((fl & oracle.FLAG_NEAR) == 0) & (scale[name] > 0)
            # a symmetric cov3D stores each off-diagonal entry once: the chain reports the derivative w.r.t. that one stored number
            # fd carries the round-off of the two evaluations of L, 2^-53 * sum |acc * out| each (a few roundings), divided by the step
            noise = 8 * 2.0 ** -53 * (np.abs(acc * base["out"]).sum(axis=1) / eps)
            err = np.maximum(0.0, np.abs(fd - g[:, j]) - noise)[ok] / scale[name][ok]
            worst = max(worst, float(err.max()))
            checked += int(ok.sum())
        print(f"mode={mode} deg={deg} {name}: worst |fd - chain| / row scale = {worst:.1e}")
        # central differences in fp64 at a relative step of 1e-6: truncation ~1e-12 x third derivative, round-off ~1e-16 / 1e-6
        assert worst <= 1e-6, (name, worst)
    assert checked > 5000
    # the screen-space gradient in NDC units: d/d(ndc) = d/d(pixel) * W / 2 resp. H / 2, zero for invisible Gaussians
    exp = acc[:, :2] * np.array([0.5 * c.W, 0.5 * c.H]) * vis[:, None]
    assert np.array_equal(got["means2D"], exp)


def test_gradient_passes_through_the_alpha_clamp():
    """One huge opaque splat (alpha = 0.99 wherever exp() is close enough to 1): d colour / d opacity_eff is G (c - bg) at EVERY pixel the
    splat reaches, clamped or not -- upstream's convention, which stage 1 keeps."""
    import test_oracle_rast_closed_form as cf
    cam, attrs, col = cf._scene([2.0], [0.8], [1.0], [(0.9, 0.3, 0.1)])
    kw = R.scene_kw(cam, cf.H, cf.W, 0, 1, bg=(0.2, 0.4, 0.6))
    n = lambda t: t.double().numpy()
    ins = (n(attrs["means3D"]), None, n(col), n(attrs["opacities"]).reshape(-1), n(attrs["scales"]), n(attrs["rotations"]), None)
    w = np.ones((3, cf.H, cf.W))
    A = oracle.rast64_accumulators(*ins, w, **kw)
    p = oracle.rast64_project(*ins, **kw)["out"][0]
    yy, xx = np.mgrid[0:cf.H, 0:cf.W]
    dx, dy = p[0] - xx, p[1] - yy
    G = np.exp(-0.5 * (p[2] * dx * dx + p[4] * dy * dy) - p[3] * dx * dy)
    assert (p[5] * G > 0.99).sum() >= 10                                 # the clamp is active on part of the footprint
    exp = float((G * (n(col)[0] - kw["bg"].astype(np.float64)).sum()).sum())       # the fp32-rounded colours the oracle was given
    assert abs(A["acc"][0, 5] - exp) <= 1e-9 * abs(exp)


# (mutant, the tensor it corrupts, case).  Narrow scene = that of test_gradients_match_double_oracle[0-3-64-64-500].
_NARROW = dict(P=500, H=64, W=64, deg=3, mode=0, seed=8)
_MUTANTS = [(1, "means3D", _NARROW, "SH view-direction term of means3D dropped"),
            (2, "means3D", _NARROW, "db[6][2]: 4z -> 2z"),
            (3, "means3D", _NARROW, "tx, ty terms of dtz dropped"),
            (4, "means3D", dict(P=600, H=64, W=80, deg=1, mode=0, seed=13, wide=True), "clamp multipliers xmul / ymul ignored"),
            (5, "means3D", dict(P=600, H=64, W=64, deg=1, mode=1, seed=6), "depth path, y component dropped"),
            (6, "scales", _NARROW, "mip coefficient: dd1 term dropped"),
            (7, "rotations", _NARROW, "one sign flipped in gq[0]")]
_OLD_BAR = 2e-3


@pytest.mark.parametrize("mutant,tensor,case,what", _MUTANTS, ids=[f"m{m[0]}" for m in _MUTANTS])
def test_mutants_land_outside_the_new_bar(mutant, tensor, case, what):
    c = R.make_case(**case)
    A = oracle.rast64_accumulators(*c.ins, c.wc, c.wa, c.wd, **c.kw)
    acc = A["acc"].astype(np.float32)                                   # what a device would hand to its chain rule
    ref = oracle.rast64_chain(*c.ins, acc, **c.kw)
    yard = oracle.rast32_chain(*c.ins, acc, **c.kw)
    mut = oracle.rast32_chain(*c.ins, acc, mutant=mutant, **c.kw)
    keep = (ref["flags"] & oracle.FLAG_NEAR) == 0
    scale = R.row_scale(acc, R.jacobian_columns(c.ins, c.kw))[tensor]
    ey, _ = R.row_err(yard[tensor], ref[tensor], scale)
    em, _ = R.row_err(mut[tensor], ref[tensor], scale)
    sy, sm = R.stats(ey[keep]), R.stats(em[keep])
    old = rel(mut[tensor], ref[tensor])
    print(f"mutant {mutant} ({what}), {tensor}: per-row e max/p99 yardstick {sy[0]:.1f}/{sy[1]:.1f}, mutant {sm[0]:.2e}/{sm[1]:.2e}; "
          f"old whole-tensor rel L2 {old:.1e}")
    assert R.within(sy, sy) and not R.within(sm, sy), "the mutant passes the new bar"
    assert sm[0] > 100 * R.FACTOR * sy[0]                               # and not by a hair
    if case is _NARROW and mutant in (2, 3):
        assert old < _OLD_BAR, "this mutant was expected to pass the old criterion"
    # the unmutated yardstick itself sits far inside the old bar
    assert rel(yard[tensor], ref[tensor]) < 1e-5


def test_clamp_mutant_is_invisible_in_the_narrow_scenes():
    """Row four of the table: without a clamped Gaussian the mutant IS the original; the wide scene is what exercises the branch."""
    c = R.make_case(**_NARROW)
    acc = oracle.rast64_accumulators(*c.ins, c.wc, c.wa, c.wd, **c.kw)["acc"].astype(np.float32)
    yard = oracle.rast32_chain(*c.ins, acc, **c.kw)
    mut = oracle.rast32_chain(*c.ins, acc, mutant=4, **c.kw)
    assert (yard["flags"] & oracle.FLAG_CLAMPED).sum() == 0
    assert all(np.array_equal(yard[k], mut[k]) for k in ("means3D", "scales", "rotations", "shs", "opacities"))
    assert not hasattr(oracle.lib(), "gvfo64_set_mutant"), "the mutant switch leaked into the fp64 build"


def test_yardstick_follows_the_reference():
    """The fp32 build is the same formulas: stage 1 within a few hundred roundings of the largest term (the exponent amplifies the rounding
    of the conic and the centre), stage 2 within a few tens per row."""
    c = R.make_case(P=600, H=64, W=64, deg=2, mode=1, seed=8)
    frac = R.zero_flagged(c, R.pixel_flags(c)["flags"])
    assert frac <= 0.03
    A64 = oracle.rast64_accumulators(*c.ins, c.wc, c.wa, c.wd, **c.kw)
    A32 = oracle.rast32_accumulators(*c.ins, c.wc, c.wa, c.wd, **c.kw)
    assert np.array_equal(A64["radii"], A32["radii"]) and np.array_equal(A64["rects"], A32["rects"])
    nz = A64["acc_abs"] > 0
    e = np.abs(A32["acc"] - A64["acc"])[nz] / (R.U * A64["acc_abs"][nz])
    print(f"yardstick accumulators: e max {e.max():.1f} p99 {np.percentile(e, 99):.1f}")
    assert e.max() < 2000 and (A32["acc"][~nz] == 0).all()


@pytest.mark.parametrize("activation", ["exp", "softplus"])
def test_activation_restatement_matches_the_package(activation):
    """rast_bwd_ref.activate64 against GaussianModel.get_*_with_delta (fp32) on random raw parameters, values and gradients; a few raw
    scales sit above softplus' linear threshold of 20."""
    P, deg = 500, 1
    g = torch.Generator().manual_seed(3)
    gm = synthetic.gaussian_model_from(synthetic.random_gaussians(P, sh_degree=deg, seed=2), deg, torch.device("cpu"), scaling_activation=activation)
    raw = {k: (getattr(gm, k).detach() + 0.3 * torch.randn(getattr(gm, k).shape, generator=g)) for k in ("_xyz", "_features_dc", "_scaling", "_rotation", "_opacity")}
    if activation == "softplus":
        raw["_scaling"][:7] = 20.5 - gm.scale_bias + torch.rand((7, 3), generator=g)
    else:
        raw["_scaling"] = raw["_scaling"].clamp(max=1.0)
    for k, v in raw.items():
        setattr(gm, k, v.clone().requires_grad_(True))
    delta = (0.05 * torch.randn((P, 14), generator=g)).requires_grad_(True)
    pk = [gm.get_xyz_with_delta(delta[:, :3]), gm.get_features_with_delta(delta[:, 10:13].unsqueeze(1)), gm.get_opacity_with_delta(delta[:, 13:]),
          gm.get_scaling_with_delta(delta[:, 3:6]), gm.get_rotation_with_delta(delta[:, 6:10])]
    r64 = {k: v.detach().double().requires_grad_(True) for k, v in raw.items()}
    d64 = delta.detach().double().requires_grad_(True)
    act = R.activate64(r64["_xyz"], r64["_features_dc"], r64["_scaling"], r64["_rotation"], r64["_opacity"], d64, aabb=gm.aabb.tolist(),
                       scale_bias=float(gm.scale_bias), opacity_bias=float(gm.opacity_bias), min_kernel_size=gm.mininum_kernel_size,
                       scaling_activation=activation)
    mine = [act[k] for k in ("means3D", "shs", "opacities", "scales", "rotations")]
    ws = [torch.randn(t.shape, generator=g) for t in pk]
    for a, b in zip(pk, mine):
        assert a.shape == b.shape
        assert (a.detach().double() - b.detach()).abs().max() <= 4e-6 * max(1.0, float(b.detach().abs().max()))
    torch.autograd.backward(pk, ws)
    torch.autograd.backward(mine, [w.double() for w in ws])
    for k in raw:
        a, b = getattr(gm, k).grad.double(), r64[k].grad
        assert (a - b).abs().max() <= 2e-5 * max(1.0, float(b.abs().max())), k
    assert (delta.grad.double() - d64.grad).abs().max() <= 2e-5 * max(1.0, float(d64.grad.abs().max()))
    assert not R.activation_flags(act).any()
