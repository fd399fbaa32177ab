"""Helpers of the two-stage conformance check of the rasteriser backward (tests/test_rast_bwd_ref.py on the host,
tests/test_rast_bwd_conformance_gpu.py on the device): scenes, the per-row and per-element error measures, the Jacobian columns of the
oracle's chain rule, the depth-tie condition and the fp64 restatement of the GaussianModel activations.

The measures (U = 2^-24, the unit roundoff of fp32):
  stage 1, element-wise      e = |acc - acc_ref| / (U * acc_abs)          acc_abs: the sums over absolute per-(pixel, splat) terms
  stage 2, per Gaussian row  e_i = ||got_i - ref_i||_2 / (U * scale_i)    scale_i = sum_k |acc[i, k]| * ||chain(e_k)_i||_2
Both are "errors in units of one rounding of the largest term", so the same bar holds at every magnitude; the bar itself is 4 x what the
fp32 yardstick (the oracle's own formulas in single precision) reaches on the same inputs.
"""
import math
from types import SimpleNamespace

import numpy as np
import torch

import oracle
from gvfdiffusion_amd import synthetic
from rast_util import camera_block

U = 2.0 ** -24
FACTOR = 4.0                      # device <= FACTOR x yardstick, maximum and 99th percentile
SR_OUTPUTS = ("means3D", "means2D", "shs", "colors_precomp", "opacities", "scales", "rotations", "cov3D_precomp")
ORDER = ("means3D", "shs", "colors_precomp", "opacities", "scales", "rotations", "cov3D_precomp")


def scene_kw(cam, H, W, deg, mode, scale_modifier=1.0, bg=(0.1, 0.4, 0.8), kernel_size=synthetic.KERNEL_2D):
    n = lambda t: t.numpy() if torch.is_tensor(t) else np.asarray(t)
    return dict(H=H, W=W, tanfovx=cam["tanfovx"], tanfovy=cam["tanfovy"], kernel_size=kernel_size, scale_modifier=scale_modifier,
                viewmatrix=n(cam["viewmatrix"]), projmatrix=n(cam["projmatrix"]), campos=n(cam["campos"]), sh_degree=deg,
                bg=np.asarray(bg, np.float32), mode=mode)


def gaussians(P, deg, seed, spread=0.8, scale_lo=0.004, scale_hi=0.04, op_lo=0.02, op_hi=0.95):
    """fp32 numpy attributes.  spread 0.8 with scales 0.004 .. 0.04: the narrow scenes of the existing backward tests; spread 2.4 with
    scales 0.02 .. 0.25: wide scenes in which some visible Gaussians sit beyond 1.3 tan(fov) (the clamped EWA branch)."""
    a = synthetic.random_gaussians(P, sh_degree=deg, seed=seed, scale_lo=scale_lo, scale_hi=scale_hi)
    a["means3D"] = a["means3D"] * spread
    a["opacities"] = a["opacities"].clamp(op_lo, op_hi)
    return {k: v.numpy().astype(np.float32) for k, v in a.items()}


def cov6_of(scales, rotations):
    r, x, y, z = np.asarray(rotations, np.float64).T
    P = r.shape[0]
    R = np.stack([1 - 2 * (y * y + z * z), 2 * (x * y - r * z), 2 * (x * z + r * y), 2 * (x * y + r * z), 1 - 2 * (x * x + z * z),
                  2 * (y * z - r * x), 2 * (x * z - r * y), 2 * (y * z + r * x), 1 - 2 * (x * x + y * y)], 1).reshape(P, 3, 3)
    L = R * np.asarray(scales, np.float64)[:, None, :]
    S = L @ L.transpose(0, 2, 1)
    return np.stack([S[:, 0, 0], S[:, 0, 1], S[:, 0, 2], S[:, 1, 1], S[:, 1, 2], S[:, 2, 2]], 1).astype(np.float32)


def make_case(P, H, W, deg, mode, seed, *, wide=False, azi=None, elev=8.0, scale_modifier=1.0, precomp=False, subpixel=False,
              crowded=False, single=False):
    """One single-frame case: c.ins (the seven operator inputs in ORDER, fp32 numpy or None), c.kw (the oracle's scene keywords), c.cam,
    upstream gradients c.wc (3,H,W), c.wa, c.wd (H,W; None outside mode 1) and c.sub ((H,W,2) or None)."""
    if single:
        import test_oracle_rast_closed_form as cf
        cam, attrs, col = cf._scene([2.0], [0.08], [0.7], [(0.9, 0.3, 0.1)])
        a = {k: v.numpy().astype(np.float32) for k, v in attrs.items()}
        ins = dict(means3D=a["means3D"], shs=None, colors_precomp=col.numpy(), opacities=a["opacities"].reshape(-1), scales=a["scales"],
                   rotations=a["rotations"], cov3D_precomp=None)
        kw = scene_kw(cam, H, W, 0, mode, bg=(0.2, 0.4, 0.6), kernel_size=0.1)
    else:
        if crowded:
            # every Gaussian within ~1 px of the image centre, where the four tiles of a 32 x 32 image meet, wide enough (sigma 2 .. 5 px) to
            # reach all four at alpha >= 1/255 and faint enough that hundreds composite before T runs out; strung out along the viewing
            # axis (world y for the azi = 0 camera) so that no two depths tie
            a = gaussians(P, deg, seed, spread=1.0, scale_lo=0.1, scale_hi=0.3, op_lo=0.01, op_hi=0.05)
            a["means3D"][:, [0, 2]] *= 0.12
            azi, elev = 0.0, 0.0
        elif wide:
            a = gaussians(P, deg, seed, spread=2.4, scale_lo=0.02, scale_hi=0.25)
        else:
            a = gaussians(P, deg, seed)
        cam = camera_block(azi=30.0 + 20 * deg if azi is None else azi, elev=elev)
        ins = dict(means3D=a["means3D"], shs=a["shs"], colors_precomp=None, opacities=a["opacities"].reshape(-1), scales=a["scales"],
                   rotations=a["rotations"], cov3D_precomp=None)
        if precomp:
            ins.update(shs=None, colors_precomp=np.random.default_rng(seed).random((P, 3)).astype(np.float32),
                       cov3D_precomp=cov6_of(a["scales"], a["rotations"]), scales=None, rotations=None)
        kw = scene_kw(cam, H, W, deg, mode, scale_modifier=scale_modifier)
    g = np.random.default_rng(seed + 1000)
    wc = g.standard_normal((3, H, W)).astype(np.float32)
    wa = g.standard_normal((H, W)).astype(np.float32) if mode == 1 else None
    wd = g.standard_normal((H, W)).astype(np.float32) if mode == 1 else None
    sub = ((g.random((H, W, 2)) - 0.5) * 0.5).astype(np.float32) if subpixel else None
    return SimpleNamespace(P=P, H=H, W=W, deg=deg, mode=mode, ins=tuple(ins[k] for k in ORDER), kw=kw, cam=cam, wc=wc, wa=wa, wd=wd, sub=sub)


def zero_flagged(c, flags):
    """No upstream gradient at threshold-flagged pixels: such a pixel contributes exactly zero to every accumulator on both sides,
    whichever way its decision fell.  Returns the flagged share."""
    m = flags != 0
    c.wc[:, m] = 0.0
    if c.wa is not None:
        c.wa[m] = 0.0
        c.wd[m] = 0.0
    return float(m.mean())


def pixel_flags(c):
    """The forward oracle's per-pixel threshold flags (alpha or test_T within 2e-4 relative of 1/255 resp. 1e-4, power within 1e-6 of 0)."""
    m3, sh, col, op, sc, ro, c6 = c.ins
    kw = {k: v for k, v in c.kw.items()}
    return oracle.rast_render(m3, sh, col, op, sc, ro, c6, subpixel_offset=c.sub, **kw)


def jacobian_columns(ins, kw, chain=None):
    """cols[name][k] = chain(e_k) for the one-hot accumulator e_k set in every row at once (the chain rule is per Gaussian)."""
    chain = chain or oracle.rast64_chain
    P = ins[0].shape[0]
    cols = {}
    for k in range(10):
        acc = np.zeros((P, 10)); acc[:, k] = 1.0
        out = chain(*ins, acc, **kw)
        for name in SR_OUTPUTS:
            if out[name] is not None:
                cols.setdefault(name, []).append(np.asarray(out[name], np.float64).reshape(P, -1))
    return {name: np.stack(v) for name, v in cols.items()}          # [10, P, n]


def row_scale(acc, cols):
    """scale_i = sum_k |acc[i, k]| * ||chain(e_k)_i||_2 per output tensor."""
    a = np.abs(np.asarray(acc, np.float64))
    return {name: np.einsum("ik,ki->i", a, np.linalg.norm(c, axis=2)) for name, c in cols.items()}


def row_err(got, ref, scale):
    """(e over the rows with scale > 0, the largest |got| over the rows with scale == 0)."""
    P = scale.shape[0]
    d = np.linalg.norm(np.asarray(got, np.float64).reshape(P, -1) - np.asarray(ref, np.float64).reshape(P, -1), axis=1)
    nz = scale > 0
    dead = np.abs(np.asarray(got, np.float64).reshape(P, -1)[~nz])
    e = np.full(P, np.nan)
    e[nz] = d[nz] / (U * scale[nz])
    return e, (float(dead.max()) if dead.size else 0.0)


def stats(e):
    e = e[np.isfinite(e)]
    return (float(e.max()), float(np.percentile(e, 99))) if e.size else (0.0, 0.0)


def within(dev, yard, factor=FACTOR):
    """dev = (max, p99) of the candidate, yard = the yardstick's: each within factor x."""
    return dev[0] <= factor * yard[0] and dev[1] <= factor * yard[1]


def depth_ties(rects, depth, visible, ulps=4):
    """Pairs of visible Gaussians whose tile rectangles overlap and whose fp32 depths lie within `ulps` units in the last place: the order
    of such a pair may differ between an fp32 and an fp64 evaluation of the depth."""
    idx = np.flatnonzero(visible)
    d = np.asarray(depth, np.float32)[idx]
    order = np.argsort(d, kind="stable")
    idx, d = idx[order], d[order]
    bits = d.view(np.int32).astype(np.int64)
    ties = []
    for a in range(len(idx)):
        b = a + 1
        while b < len(idx) and bits[b] - bits[a] <= ulps:
            ra, rb = rects[idx[a]], rects[idx[b]]
            if max(ra[0], rb[0]) < min(ra[2], rb[2]) and max(ra[1], rb[1]) < min(ra[3], rb[3]):
                ties.append((int(idx[a]), int(idx[b])))
            b += 1
    return ties


# ---- the GaussianModel activations (get_*_with_delta) restated in fp64 torch --------------------------------------------------------
def activate64(xyz, fdc, scaling, rotation, opacity, delta, *, aabb, scale_bias, opacity_bias, min_kernel_size, scaling_activation):
    """fp64 restatement of GaussianModel.get_{xyz,scaling,rotation,features,opacity}_with_delta on raw parameters (torch, differentiable).
    delta: (P, 14) [xyz3 | scale3 | rot4 | rgb3 | op1] or None.  scaling_activation: 'exp' | 'softplus' (linear above 20)."""
    t = lambda v: v if torch.is_tensor(v) else torch.as_tensor(np.asarray(v), dtype=torch.float64)
    xyz, fdc, scaling, rotation, opacity = (t(v).double() for v in (xyz, fdc, scaling, rotation, opacity))
    ab = t(aabb).double()
    d = torch.zeros((xyz.shape[0], 14), dtype=torch.float64) if delta is None else t(delta).double()
    means = xyz * ab[None, 3:] + ab[None, :3] + d[:, 0:3]
    x = scaling + float(scale_bias) + d[:, 3:6]
    act = torch.exp(x) if scaling_activation == "exp" else torch.where(x > 20.0, x, torch.log1p(torch.exp(torch.clamp(x, max=20.0))))
    scales = torch.sqrt(act * act + float(min_kernel_size) ** 2)
    q = rotation + torch.tensor([1.0, 0.0, 0.0, 0.0], dtype=torch.float64)[None] + d[:, 6:10]
    rots = q / torch.clamp(q.norm(dim=1, keepdim=True), min=1e-12)
    shs = fdc + d[:, None, 10:13]
    opac = torch.sigmoid(opacity.reshape(-1, 1) + float(opacity_bias) + d[:, 13:14])
    return dict(means3D=means, shs=shs, opacities=opac, scales=scales, rotations=rots, pre_scale=x, qnorm=q.norm(dim=1))


def activation_flags(act, rel=1e-5):
    """Gaussians whose activation sits within `rel` of a branch threshold: pre-activation scale vs 20, |q| vs 1e-12."""
    x, n = act["pre_scale"].detach().numpy(), act["qnorm"].detach().numpy()
    return (np.abs(x - 20.0) <= rel * 20.0).any(axis=1) | (np.abs(n - 1e-12) <= rel * 1e-12)
