"""Float64 oracle of the SSIM / L1 image loss (utils/loss_util.py:ssim semantics), written as explicit window sums rather than as
the reference's conv2d calls, and differentiable through torch autograd (so that device tests can take its gradient).

Window: the one the reference convolves with -- the 1-D taps exp(-(x-5)^2 / 4.5) rounded to fp32 and normalised by their fp32 sum,
their outer product rounded to fp32 -- then applied in float64.  The HIP kernels apply the 1-D taps separably; the products differ
from this window by at most 1 fp32 ulp per weight.

Also: `ssim_torch32`, the same formula as an fp32 torch composition (depthwise conv2d) on the host, the yardstick the device tests
calibrate their bars with.

Stage-wise conformance (second half of the file; tests/test_image_loss_conformance_ref.py on the host and
tests/test_image_loss_conformance_gpu.py on the device use it).  Everything after the five window moments is a pixel-wise function of
them, so first-order bounds come from float64 autograd.  u = 2^-24, the unit roundoff of fp32; every rounding is |e| <= u relative
to its own result.  The window of the stage references is the 1-D taps applied separably in float64 (their products are exact in
float64), which is the kernels' window; it is not ssim_map64's rounded 11 x 11 window.

  moments   m = (G*p, G*g, G*pp, G*gg, G*pg).  A term w_i w_j x of a moment goes through C_M = 23 roundings in image_loss_fwd_kernel:
            the product w*p (1), 11 adds / fmas of the horizontal pass (the first, onto 0, rounds the product for pp, gg, pg and is
            exact for p, g: 11 covers both), 11 fmas of the vertical pass.  Every partial sum is at most G*|x| in magnitude, so
            |m32 - m| <= C_M u G*|x| to first order (x = p, g, pp, gg, pg; G*|pg| for the mixed one).
  stage A   the saved maps a, b, c and S.  The closing arithmetic is restated operation by operation in float64 with a relative
            perturbation (1 + e_k) at every fp32 operation of the kernel (`closing`: 15 up to S, 26 up to a; divisions are the
            correctly rounded ones hipcc emits without fast-math, one rounding each) and (1 + e) on C1, C2 with weight 3 (the kernel's
            0.01f * 0.01f: the literal's rounding twice, the product's once).  bound(q) = SECOND * (sum_i |dq/dm_i| C_M u G*|x_i| +
            sum_k |dq/de_k| n_k u), the Jacobians from autograd at e = 0: every rounding is carried through the cancellations of
            s1 = G*pp - mu1^2 etc. rather than charged to |q| alone.  SECOND = (1 - r)^-4, r = bound(B1) / B1 + bound(B2) / B2: the
            maps are rational in (m, e) with denominators B1^i B2^j, i + j <= 3; a relative error r of a denominator factor enlarges
            the linear term of 1 / B^k by at most (1 - r)^-(k+1) (the remainder of its Taylor series), and the fourth power has room
            for the products of two roundings inside a numerator, which are u times a first-order term.  r >= 1/2 gives an infinite
            bound (no judgement).
  stage B   the gradient from the maps the device itself saved: k_l1 sign(p - g) + k_ss (G*a + 2p G*b + g G*c) in float64 with
            coef_of's k_l1, k_ss computed exactly as the kernel does (fp32 1/n, fp32 products and sum, one rounding each: torch fp32
            on the host).  C_B = 27 roundings for a term of the SSIM part: 11 + 11 fmas of the two passes, the product with 2p or g
            (1), the two adds of ds (2), the product with k_ss (1), the closing add (1); the L1 term, exact as a product (+-k_l1 or 0),
            sees the closing add only:  bound = C_B u |k_ss| (G*|a| + 2|p| G*|b| + |g| G*|c|) + u |k_l1 sign(p - g)|.
  stage C   mean L1: |p - g| is rounded once and a thread adds four of them in fp32 (3 roundings; the first add is onto 0), the
            rest is double: 4 u mean|p - g|, and the closing conversion to fp32 one more u.  Mean SSIM: the mean of stage A's bound
            on S, 3 u mean|S| for the four-term partial sums, u |mean| for the conversion.  The double sums add n 2^-53 relative.
            The loss is checked against the device's own double sums of the two terms (the per-workgroup partials at the head of the
            scratch) to the one fp32 rounding of its conversion.

`emulate_forward` / `emulate_backward` restate the kernels in torch fp32 on the host (separable taps, the kernel's grouping of
operations, fmaf as a float64 product-sum rounded to fp32) and take the mutations the host test feeds the measure with."""
import math

import torch
import torch.nn.functional as F

WIN, RAD = 11, 5
C1, C2 = 0.01 ** 2, 0.03 ** 2


def taps32() -> torch.Tensor:
    g = torch.tensor([math.exp(-((x - RAD) ** 2) / (2 * 1.5 ** 2)) for x in range(WIN)], dtype=torch.float32)
    return g / g.sum()


def window32() -> torch.Tensor:
    g = taps32()
    return torch.outer(g, g)          # each weight one fp32 rounding of the product


def _as4d(x: torch.Tensor) -> torch.Tensor:
    return x.unsqueeze(0) if x.dim() == 3 else x


def _wsum(x: torch.Tensor, w: torch.Tensor) -> torch.Tensor:
    """sum_{i,j} w[i,j] x[y+i-5, x+j-5] with zero padding, per plane, as 121 shifted slices (float64)."""
    H, W = x.shape[-2:]
    xp = F.pad(x, (RAD, RAD, RAD, RAD))
    out = torch.zeros_like(x)
    for i in range(WIN):
        for j in range(WIN):
            out = out + w[i, j] * xp[..., i:i + H, j:j + W]
    return out


def ssim_map64(img1: torch.Tensor, img2: torch.Tensor) -> torch.Tensor:
    p, g = _as4d(img1).double(), _as4d(img2).double()
    w = window32().double().to(p.device)
    mu1, mu2 = _wsum(p, w), _wsum(g, w)
    s1 = _wsum(p * p, w) - mu1 * mu1
    s2 = _wsum(g * g, w) - mu2 * mu2
    s12 = _wsum(p * g, w) - mu1 * mu2
    return (2 * mu1 * mu2 + C1) * (2 * s12 + C2) / ((mu1 * mu1 + mu2 * mu2 + C1) * (s1 + s2 + C2))


def ssim64(img1: torch.Tensor, img2: torch.Tensor) -> torch.Tensor:
    return ssim_map64(img1, img2).mean()


def loss64(pred: torch.Tensor, target: torch.Tensor, l1_weight: float = 1.0, ssim_weight: float = 0.2) -> torch.Tensor:
    p, g = pred.double(), target.double()
    return l1_weight * (p - g).abs().mean() + ssim_weight * (1 - ssim64(p, g))


def ssim_torch32(img1: torch.Tensor, img2: torch.Tensor) -> torch.Tensor:
    """The same SSIM as an fp32 torch composition: five depthwise 11 x 11 conv2d calls (what a user would write).  Computed on host
    copies of its inputs and returned on the host (autograd carries the gradient back to a device input): the device tests compare
    on the host, and no device tensor reaches a library convolution."""
    p, g = _as4d(img1).float().cpu(), _as4d(img2).float().cpu()
    C = p.shape[1]
    w = window32().expand(C, 1, WIN, WIN).contiguous()
    conv = lambda x: F.conv2d(x, w, padding=RAD, groups=C)  # noqa: E731
    mu1, mu2 = conv(p), conv(g)
    s1 = conv(p * p) - mu1 * mu1
    s2 = conv(g * g) - mu2 * mu2
    s12 = conv(p * g) - mu1 * mu2
    return ((2 * mu1 * mu2 + C1) * (2 * s12 + C2) / ((mu1 * mu1 + mu2 * mu2 + C1) * (s1 + s2 + C2))).mean()


def loss_torch32(pred: torch.Tensor, target: torch.Tensor, l1_weight: float = 1.0, ssim_weight: float = 0.2) -> torch.Tensor:
    """On the host as well (see ssim_torch32)."""
    pred, target = pred.cpu(), target.cpu()
    return l1_weight * F.l1_loss(pred, target) + ssim_weight * (1 - ssim_torch32(pred, target))


# ---- stage-wise conformance (module docstring) -------------------------------------------------------------------------------------
U32 = 2.0 ** -24                       # unit roundoff of fp32
C_M = 23                               # roundings on a term of a window moment: 1 (w*p) + 11 (horizontal) + 11 (vertical)
C_B = 27                               # ... of the gradient's SSIM part: 11 + 11 (passes) + 1 (times 2p or g) + 2 (ds) + 1 (k_ss) + 1 (sum)
C_CONST = 3                            # C1, C2 as 0.01f * 0.01f: the literal's rounding counted twice, the product's once
C_L1 = 4                               # |p - g| (1) and a thread's four-term fp32 sum (3; the first add is onto 0)
C_SSUM = 3                             # a thread's four-term fp32 sum of S
S_LEVEL = 1e-4                         # the level the bound on S stays under on textured inputs (asserted by the device test)
TILE_W, TILE_H, ROWS_PER_THREAD = 64, 16, 4


def rounds(k: int) -> float:
    """(1 + u)^k - 1 <= k u (1 + 32 u) for k <= 32: the relative error k roundings can add up to."""
    assert k <= 32
    return k * U32 * (1.0 + 32.0 * U32)


def excess(out: torch.Tensor, ref: torch.Tensor, bnd: torch.Tensor):
    """(number of elements outside the bound, largest |out - ref| / bound); NaN counts as outside.  As gemm_ref.excess, but an element
    with err = bound = 0 has ratio 0."""
    d = (out.double() - ref).abs()
    bad = ~(d <= bnd)
    ratio = torch.where(d == 0, torch.zeros_like(d), d / bnd.clamp_min(1e-300))
    return int(bad.sum()), float(torch.nan_to_num(ratio, nan=float("inf")).max()) if ratio.numel() else 0.0


def wsep64(x: torch.Tensor) -> torch.Tensor:
    """G*x per plane in float64: the 1-D taps along W, then along H, zero padding 5 (the kernels' window, exact products)."""
    x = x.double()
    t = taps32().double()
    H, W = x.shape[-2:]
    xp = F.pad(x, (RAD, RAD, RAD, RAD))
    h = sum(t[k] * xp[..., :, k:k + W] for k in range(WIN))
    return sum(t[k] * h[..., k:k + H, :] for k in range(WIN))


class _Roundings:
    """r(x) = x (1 + e) with a fresh zero-valued e per call: one fp32 operation of the kernel.  `weight`: how many u that e may be."""

    def __init__(self, like):
        self.like, self.e, self.w = like, [], []

    def __call__(self, x, weight=1):
        e = torch.zeros_like(self.like, requires_grad=True)
        self.e.append(e)
        self.w.append(weight)
        return x * (1 + e)


def closing(m, r=lambda x, weight=1: x):
    """image_loss_fwd_kernel after the moments, operation by operation (csrc/loss.hip; formulas in include/gvf_loss.h).  With the
    default r it is the plain float64 formula; with a _Roundings every fp32 operation carries its perturbation."""
    mu1, mu2, m11, m22, m12 = m
    c1, c2 = r(C1 + 0 * mu1, C_CONST), r(C2 + 0 * mu1, C_CONST)
    mu1mu2, mu1sq, mu2sq = r(mu1 * mu2), r(mu1 * mu1), r(mu2 * mu2)
    s1, s2, s12 = r(m11 - mu1sq), r(m22 - mu2sq), r(m12 - mu1mu2)
    A1, A2 = r(2 * mu1mu2 + c1), r(2 * s12 + c2)                       # 2 x is exact
    B1, B2 = r(r(mu1sq + mu2sq) + c1), r(r(s1 + s2) + c2)
    D = r(B1 * B2)
    S = r(r(A1 * A2) / D)                                              # 15 operations up to here
    dmu1 = r(r(r(2 * mu2 * A2) / D) - r(r(2 * mu1 * S) / B1))
    b = r(-S / B2)
    c = r(2 * A1 / D)
    a = r(r(dmu1 - r(2 * mu1 * b)) - r(mu2 * c))                       # 26 up to here
    return dict(S=S, a=a, b=b, c=c, B1=B1, B2=B2)


def stage_a(p: torch.Tensor, g: torch.Tensor):
    """(ref, bound): dicts S, a, b, c of float64 (planes, H, W) tensors for fp32 inputs p, g (planes, H, W) on the host."""
    p, g = p.double(), g.double()
    xs = (p, g, p * p, g * g, p * g)
    dm = [rounds(C_M) * wsep64(x.abs()) for x in xs]
    m = [wsep64(x).requires_grad_(True) for x in xs]
    r = _Roundings(m[0])
    q = closing(m, r)
    lin = {}
    for name, v in q.items():
        grads = torch.autograd.grad(v.sum(), m + r.e, retain_graph=True, allow_unused=True)      # pixel-wise: the sum's gradient is the Jacobian
        tot = torch.zeros_like(p)
        for j, w in zip(grads, dm + [k * U32 for k in r.w]):
            if j is not None:
                tot = tot + j.abs() * w
        lin[name] = tot
    rr = lin["B1"] / q["B1"].detach() + lin["B2"] / q["B2"].detach()
    second = torch.where(rr < 0.5, (1 - rr.clamp_max(0.5)) ** -4, torch.full_like(rr, float("inf")))
    ref = {k: q[k].detach() for k in "Sabc"}
    return ref, {k: second * lin[k] for k in "Sabc"}


def coef32(gterms, w_l1: float, w_ssim: float, n: int):
    """coef_of of csrc/loss.hip in torch fp32 on the host, operation by operation: (k_l1, k_ss) as Python floats."""
    t = torch.as_tensor(gterms).detach().cpu().float()
    f = lambda v: torch.tensor(v, dtype=torch.float32)  # noqa: E731
    inv_n = f(1.0) / torch.tensor(n, dtype=torch.int64).float()
    return float((t[0] * f(w_l1) + t[1]) * inv_n), float((t[2] - t[0] * f(w_ssim)) * inv_n)


def stage_b(p, g, maps, gterms, w_l1, w_ssim, n=None):
    """(ref, bound) of the gradient given the saved maps (a, b, c) -- the device's own, read back, or the test's."""
    p, g = p.double(), g.double()
    a, b, c = (x.double() for x in maps)
    k1, ks = coef32(gterms, w_l1, w_ssim, p.numel() if n is None else n)
    sg = torch.sign(p - g)
    ref = k1 * sg + ks * (wsep64(a) + 2 * p * wsep64(b) + g * wsep64(c))
    bnd = rounds(C_B) * abs(ks) * (wsep64(a.abs()) + 2 * p.abs() * wsep64(b.abs()) + g.abs() * wsep64(c.abs())) + U32 * abs(k1) * sg.abs()
    return ref, bnd


def stage_c(p, g, S_ref, S_bnd):
    """(ref, bound) as float64 tensors [mean L1, mean SSIM] of the two fp32 terms."""
    d = (p.double() - g.double()).abs()
    n = d.numel()
    dbl = n * 2.0 ** -53
    l1 = d.mean()
    e_l1 = (rounds(C_L1) + dbl) * l1
    s = S_ref.mean()
    e_s = S_bnd.mean()
    e_s = e_s + (rounds(C_SSUM) + dbl) * (S_ref.abs().mean() + e_s)
    return torch.stack([l1, s]), torch.stack([e_l1 + U32 * (l1 + e_l1), e_s + U32 * (s.abs() + e_s)])


def loss_of_sums(ml: float, ms: float, w_l1: float, w_ssim: float):
    """(ref, bound) of the fp32 loss given the double means the device formed: the reducer's double expression (weights are fp32
    arguments widened), converted once; 2^-50 covers its three double operations."""
    wl, ws = float(torch.tensor(w_l1, dtype=torch.float32)), float(torch.tensor(w_ssim, dtype=torch.float32))
    v = wl * ml + ws * (1.0 - ms)
    mag = abs(wl * ml) + abs(ws) * (1.0 + abs(ms))
    return v, U32 * abs(v) + 2.0 ** -50 * mag


def judge(p, g, cand, gterms, w_l1, w_ssim, n=None):
    """cand: maps (a, b, c), grad, terms (3 fp32), ml, ms (the double means behind terms[1], terms[2]).  -> ({stage: (failures, worst
    err / bound)}, share of pixels whose bound on S exceeds S_LEVEL).  Stage B takes cand's own maps."""
    ref, bnd = stage_a(p, g)
    cat = lambda d: torch.stack([d[k] for k in "abc"])  # noqa: E731
    out = {"A": excess(torch.stack([x.double().cpu() for x in cand["maps"]]), cat(ref), cat(bnd))}
    out["B"] = excess(cand["grad"].cpu(), *stage_b(p, g, [x.cpu() for x in cand["maps"]], gterms, w_l1, w_ssim, n))
    t = cand["terms"].double().cpu()
    rc, bc = stage_c(p, g, ref["S"], bnd["S"])
    sums = torch.tensor([cand["ml"], cand["ms"]], dtype=torch.float64)
    lv, lb = loss_of_sums(cand["ml"], cand["ms"], w_l1, w_ssim)
    # the two terms against float64, their double sums likewise (less the conversion), the fp32 terms one rounding from their sums, the loss
    got = torch.cat([t[1:], sums, t[1:], t[:1]])
    want = torch.cat([rc, rc, sums, torch.tensor([lv], dtype=torch.float64)])
    # (1 + 2^-20): the caller's sum of the partials may add in another order than the reducer (n 2^-53 relative, far inside)
    bar = torch.cat([bc, bc, U32 * (1.0 + 2.0 ** -20) * sums.abs(), torch.tensor([lb], dtype=torch.float64)])
    out["C"] = excess(got, want, bar)
    return out, float((bnd["S"] > S_LEVEL).double().mean())


# ---- inputs of the conformance tests -------------------------------------------------------------------------------------------------
SHAPES = [(1, 1, 1), (2, 1, 70), (2, 67, 3), (3, 5, 7), (2, 11, 11), (2, 15, 63), (2, 16, 64), (3, 17, 65), (2, 21, 69), (2, 22, 70),
          (3, 33, 129), (2, 37, 53)]                      # (planes, H, W): the tile is 64 x 16, its halo 5, a thread owns 4 rows
KINDS = ("noise", "const", "ties", "spikes", "wide")
TEXTURED = ("noise", "wide")                             # the inputs whose bound on S must stay under S_LEVEL at every pixel


def make_inputs(kind: str, shape, seed: int = 0):
    """(pred, gt): fp32 (planes, H, W) on the host.  noise: the pair of tests/test_image_loss_gpu.py:_pair; const: noise against a
    constant per plane; ties: a noise pair equal on the first rows of plane 0; spikes: a flat image with one bright pixel in each
    corner and on both sides of each tile seam, against noise; wide: a noise pair in [-0.5, 1.5]."""
    P, H, W = shape
    gen = torch.Generator().manual_seed(1000 * seed + 7 * P + 31 * H + 131 * W + KINDS.index(kind))
    a = torch.rand(shape, generator=gen)
    b = (a + 0.15 * torch.randn(shape, generator=gen)).clamp(0, 1)
    if kind == "noise":
        return a, b
    if kind == "const":
        return a, (0.25 + 0.2 * torch.arange(P, dtype=torch.float32)).view(P, 1, 1).expand(shape).contiguous()
    if kind == "ties":
        b[0, :min(4, (H + 1) // 2)] = a[0, :min(4, (H + 1) // 2)]
        return a, b
    if kind == "spikes":
        x = (0.2 + 0.1 * torch.arange(P, dtype=torch.float32)).view(P, 1, 1).expand(shape).contiguous()
        ys = sorted({0, H - 1, H // 2} | {y for y in (TILE_H - 1, TILE_H, 2 * TILE_H - 1, 2 * TILE_H) if y < H})
        xs = sorted({0, W - 1, W // 2} | {c for c in (TILE_W - 1, TILE_W, 2 * TILE_W - 1, 2 * TILE_W) if c < W})
        for k in range(P):
            for i, y in enumerate(ys):
                for j, c in enumerate(xs):
                    if (i + j + k) % 2 == 0 or (y in (0, H - 1) and c in (0, W - 1)):
                        x[k, y, c] = 1.0
        return x, b
    if kind == "wide":
        a = 2 * a - 0.5
        return a, (a + 0.3 * torch.randn(shape, generator=gen)).clamp(-0.5, 1.5)
    raise ValueError(kind)


# ---- the kernels restated in torch fp32 on the host (the stand-in candidate of the host test) ----------------------------------------
MUTATIONS = ("replicate", "seam_x", "seam_y", "plane", "half_b", "sign0", "n_hw", "no_c2", "tap")


def _fma(a, b, c):
    """fmaf: the float64 product is exact; the sum is rounded to 53 bits and then to 24 (a double rounding, far below any bar here)."""
    return (a.double() * b.double() + c.double()).float()


def _emu_taps(mut):
    t = taps32().clone()
    if "tap" in mut:
        t[RAD] = t[RAD] * (1.0 + 1e-4)
    return t


def _emu_pad(x, mut):
    return F.pad(x, (RAD, RAD, RAD, RAD), mode="replicate") if "replicate" in mut else F.pad(x, (RAD, RAD, RAD, RAD))


def _seam(n: int, tile: int, d: int, halo: int) -> torch.Tensor:
    """1 where output i may see input i + d: inside its tile's staged region [t0 - halo, t0 + tile + halo)"""
    i = torch.arange(n)
    t0 = tile * (i // tile)
    return ((i + d >= t0 - halo) & (i + d < t0 + tile + halo)).float()


def _emu_vpass(h, t, H, mut):
    acc = torch.zeros_like(h[..., :H, :])
    for k in range(WIN):
        mk = _seam(H, TILE_H, k - RAD, 4 if "seam_y" in mut else RAD).view(-1, 1)
        acc = _fma(t[k], h[..., k:k + H, :] * mk, acc)
    return acc


def _thread_sums(x):
    """a thread's fp32 sum over its four rows (rows 4q .. 4q + 3: tiles start at multiples of 16), then everything in double"""
    P, H, W = x.shape
    x = F.pad(x, (0, 0, 0, -H % ROWS_PER_THREAD)).view(P, -1, ROWS_PER_THREAD, W)
    s = x[:, :, 0]
    for j in range(1, ROWS_PER_THREAD):
        s = s + x[:, :, j]
    return float(s.double().sum())


def emulate_forward(p, g, w_l1, w_ssim, mut=()):
    """image_loss_fwd_kernel<true> + the reducer -> dict maps (a, b, c), S, terms, ml, ms"""
    p, g = p.float(), g.float()
    P, H, W = p.shape
    if "plane" in mut:                                   # the tile's plane base one plane low
        p, g = p.roll(1, 0), g.roll(1, 0)
    t = _emu_taps(mut)
    pp, gp = _emu_pad(p, mut), _emu_pad(g, mut)
    h = [torch.zeros((P, H + 2 * RAD, W)) for _ in range(5)]
    for k in range(WIN):
        mk = _seam(W, TILE_W, k - RAD, 4 if "seam_x" in mut else RAD)
        pv, gv = pp[..., k:k + W] * mk, gp[..., k:k + W] * mk
        wp, wg = t[k] * pv, t[k] * gv
        h = [h[0] + wp, h[1] + wg, _fma(wp, pv, h[2]), _fma(wg, gv, h[3]), _fma(wp, gv, h[4])]
    mu1, mu2, m11, m22, m12 = (_emu_vpass(x, t, H, mut) for x in h)
    c = torch.tensor(0.01, dtype=torch.float32)
    c1 = c * c
    c = torch.tensor(0.03, dtype=torch.float32)
    c2 = c * c
    mu1mu2, mu1sq, mu2sq = mu1 * mu2, mu1 * mu1, mu2 * mu2
    s1, s2, s12 = m11 - mu1sq, m22 - mu2sq, m12 - mu1mu2
    A1 = 2 * mu1mu2 + c1
    A2 = 2 * s12 if "no_c2" in mut else 2 * s12 + c2
    B1, B2 = mu1sq + mu2sq + c1, s1 + s2 + c2
    D = B1 * B2
    S = (A1 * A2) / D
    dmu1 = (2 * mu2 * A2) / D - (2 * mu1 * S) / B1
    ds1 = -S / B2
    ds12 = (2 * A1) / D
    da = dmu1 - 2 * mu1 * ds1 - mu2 * ds12
    n = H * W if "n_hw" in mut else P * H * W
    ml, ms = _thread_sums((p - g).abs()) / n, _thread_sums(S) / n
    wl, ws = float(torch.tensor(w_l1, dtype=torch.float32)), float(torch.tensor(w_ssim, dtype=torch.float32))
    terms = torch.tensor([wl * ml + ws * (1.0 - ms), ml, ms], dtype=torch.float64).float()
    return dict(maps=(da, ds1, ds12), S=S, terms=terms, ml=ml, ms=ms)


def emulate_backward(p, g, maps, gterms, w_l1, w_ssim, mut=()):
    """image_loss_bwd_kernel on the given maps -> the gradient"""
    p, g = p.float(), g.float()
    P, H, W = p.shape
    k1, ks = (torch.tensor(v, dtype=torch.float32) for v in coef32(gterms, w_l1, w_ssim, H * W if "n_hw" in mut else P * H * W))
    t = _emu_taps(mut)
    m = []
    for x in maps:
        xp = _emu_pad(x.float(), mut)
        h = torch.zeros((P, H + 2 * RAD, W))
        for k in range(WIN):
            h = _fma(t[k], xp[..., k:k + W] * _seam(W, TILE_W, k - RAD, 4 if "seam_x" in mut else RAD), h)
        m.append(_emu_vpass(h, t, H, mut))
    ds = m[0] + ((p if "half_b" in mut else 2 * p) * m[1]) + g * m[2]
    d = p - g
    sg = torch.where(d == 0, torch.ones_like(d), torch.sign(d)) if "sign0" in mut else torch.sign(d)
    return k1 * sg + ks * ds


def emulate(p, g, gterms, w_l1, w_ssim, mut=()):
    """forward, then the backward on the forward's maps: the candidate `judge` takes"""
    cand = emulate_forward(p, g, w_l1, w_ssim, mut)
    cand["grad"] = emulate_backward(p, g, cand["maps"], gterms, w_l1, w_ssim, mut)
    return cand
