"""fp64 reference and per-element error bound of the training kernels of csrc/dit_train.hip (include/gvf_dit_train.h): the backward of the
LayerNorm + (affine | adaLN), the gated residual forward and backward, the multi-head RMSNorm forward and backward, and the column-sum
finaliser they share.  Built on tests/dit_train_ref.py (the float64 formulas: every reference value below is ln_mod / gate / rms at
torch.float64), tests/gemm_ref.py (r16, _round_bound, excess, U32) and the LayerNorm counts of tests/rowblock_ref.py (kernel "elem").
Every model returns, per output, (reference, bound); for a 16-bit output the bound is the interval form of gemm_ref: the stored value lies
in [R16(a - e), R16(a + e)] and the bound is the distance from the reference to the farther end.  The LayerNorm forward y is elem.hip's
kernel and is held by tests/test_elem_conformance_gpu.py; it is not modelled here.

Rounding points, read from dit_train.hip, and the count behind every term (U = 2^-24, one fp32 rounding; first order, 1e-3 added for the
second).  The file is built with the compiler's default contraction, so a product and the add after it may or may not be fused: the unfused
form is counted (fusing only removes roundings).  A product with a factor that is exactly 1 (no scale, no affine pair, no gate) is exact and
not counted.  A "depth" counts the adds a term passes through, the first add (to zero) included although it is exact.

  * LayerNorm statistics.  Vector kernel (C = 256 VPL <= 1024): a lane owns columns 4 (lane + 64 i) .. + 3, sums them as (a + b) + (c + d)
    and adds that to its running sum (depth 2 + VPL), then the 64-lane tree (6): depth_s = VPL + 8; one more for the squares:
    depth_q = VPL + 9.  Generic kernel: a lane owns columns lane + 64 i in sequence (ceil(C / 64)), the tree: depth_s = ceil(C / 64) + 6,
    depth_q one more.  (These are rowblock_ref.ln_model's counts for the forward kernel "elem", which sums the same way.)  A true division by
    (float)C: one rounding of the mean, of mean_lo, of the variance.
    The mean is a two-term sum: mean' = fl(sum / C) is off by e_m1 = depth_s U sum|x| / C + U |mean|; the centred values fl(x - mean') are
    summed again (one rounding each, then the same depth) and mean_lo' = fl(r / C), so that mean' + mean_lo' is off by
    e_m2 = (depth_s + 1) U sum(|d| + e_m1) / C + U e_m1 only -- of the order of U times the row's SPREAD, whatever its offset.
    v = fl(fl(x - mean') - mean_lo') = d - (error of the two-term mean) + two roundings: e_d = e_m2 + 2 U (|d| + e_m1).  Sum of squares as in
    rowblock_ref (sum d = 0 exactly, so the part of the error that is common to the row enters as C e_m2^2 only), with two element-wise
    roundings in v instead of one: e_q = (depth_q + 4.1) U Q + C e_m2^2, Q = sum (|d| + e_d)^2.  rstd = rsqrtf(fl(q / C) + eps): rowblock_ref's
    count, relative d_r = (e_q / C + U var) / (2 (var + eps)) + 3 U.  xh = fl(v rstd): e_xh = |d| rstd d_r + rstd e_d + U |xh|.
    Constant rows are in range: there d = 0 and xh = 0 exactly, rstd = eps^-1/2, and e_xh is rstd times second-order terms.
  * LayerNorm dx.  m = fl(1 + scale) and gm = fl(dy m): e_gm = 2 U |gm|; g = fl(gm w): e_g = e_gm + U |g|.  c1 = sum g / C and
    c2 = sum fl(g xh) / C: the lane adds its values IN SEQUENCE here (sg += ..., 4 VPL adds in the vector kernel, ceil(C / 64) in the generic
    one), then the tree and the division: depth_g = 4 VPL + 6 resp. ceil(C / 64) + 6;
    e_c1 = depth_g U sum|g| / C + sum e_g / C + U |c1|; the products p = g xh carry e_p = |xh| e_g + |g| e_xh + U |p|, and
    e_c2 = depth_g U sum|p| / C + sum e_p / C + U |c2|.  inner = (g - c1) - fl(xh c2):
    e_in = e_g + e_c1 + |xh| e_c2 + |c2| e_xh + U (|xh c2| + |g - c1| + |inner|) -- e_xh is carried through c2 and through xh c2.
    dx = dres + fl(rstd inner): rstd (e_in + d_r |inner|) + U |rstd inner| + U |dx| (the last only with dres) -- the relative error of rstd
    is carried through the whole term.
  * Column sums (dshift, dscale, dw, db, dgate, dgamma).  Terms: dshift dy (exact); dscale fl(dy a), a = fl(fl(xh w) + b):
    e_a = |w| e_xh + U |xh w| + U |a|, term error |dy| e_a + U |dy a|; dw fl(gm xh): |xh| e_gm + |gm| e_xh + U |gm xh|; db gm: e_gm;
    dgate fl(dout h): U |dout h|; dgamma fl(dy xt): |dy| e_xt + U |dy xt|.
    Vector kernels: wave w of a workgroup takes rows s0 + w + 4 i of each segment (group x workgroup) [s0, s1): ceil(len / 4) <= 4 adds for a
    per-group sum; the four waves in order, 3 adds.  dw / db are NOT per group: a wave keeps adding across the segments of its workgroup,
    sum over the segments of ceil(len / 4) adds -- up to 16 when every row is its own group (all rows then go to wave 0).  Generic kernels: a
    thread adds the up to 16 rows of a segment (dw / db: of the workgroup) in sequence.  The finaliser: thread k adds slots lo + k, lo + k + 4,
    ...: ceil(slots / 4) adds, then (0 + 1) + (2 + 3): 2, then * factor (exact for factor 1 and 8).  The bound of a sum is
    depth U sum|term| + sum(term errors), the depth per path and per group.  Slots of a group, from the layout documented in
    include/gvf_dit_train.h (slot of workgroup wg for group g: wg + g): last_row / 16 - first_row / 16 + 1; outputs that are not per group
    have one slot per workgroup.
  * Gate.  out = x + fl(gate h): U |gate h| + U |out|.  dh = R16(fl(gate dout)): one fp32 rounding U |gate dout|, then the 16-bit interval.
  * RMSNorm.  Nothing in gvfdiffusion_amd/_build.py turns on fast-math for dit_train.hip, so sqrtf and the divisions are the correctly
    rounded ones (U each).  ss: 8 squares (1 each; exact for 16-bit inputs, still counted) added in sequence (8), then 2 (d = 32) or 3
    (d = 64) exchange levels: all terms positive, relative error depth_ss U with depth_ss = 11 / 12 (rowblock_ref._rms16 counts the same
    sum as depth 11).  den = max(sqrtf(ss), 1e-12f): relative d_den = (depth_ss / 2 + 1) U, which also covers the floor (1e-12f against
    1e-12).  The fp32 constant 5.656854249492381f is off from sqrt(32) by up to U: c = 1 for d = 32, 0 for d = 64 (8 is exact).
    y = ((x / den) gamma) sqrt_d: relative d_den + 3 U + c U.  xt = x / den: e_xt = (d_den + U) |xt|; u = (dy gamma) sqrt_d:
    e_u = (2 + c) U |u|; dot: 8 products (e_p = |u| e_xt + |xt| e_u + U |u xt|) added in sequence plus the exchange:
    e_dot = (8 + levels) U sum|u xt| + sum e_p; dx = (u - fl(xt dot)) / den:
    (e_u + |dot| e_xt + |xt| e_dot + U |xt dot| + U |u - xt dot|) / den + (d_den + U) |dx|.  dgamma: the column sum above (4 + 3 +
    finaliser) times sqrt_d: (1 + c) U |dgamma| more.
  * 16-bit outputs (dh, RMSNorm y and dx): the interval form.  check16() holds an element to its interval [R16(a - e), R16(a + e)] itself
    (an infinite end compares as a number, so that an fp16 overflow must have the right sign) and reports excess()'s ratio over the
    elements with a finite bound.

Nothing above was fitted to the kernels.  tests/test_dit_train_conformance_ref.py checks on the CPU that an fp32 emulation of every kernel,
in the kernel's order and in another legal one, lies inside these bounds, and that each small bug they exist to catch lies outside.

Measured on the MI355X (tests/test_dit_train_conformance_gpu.py; largest |err| / bound over all cases, bf16 and fp16, no element outside):
  LayerNorm backward, vector kernels (VPL 1 / 2 / 3 / 4): dx 0.25 without dres and 0.997 / 0.991 / 0.990 / 0.993 with it (the last add's half
  ulp of dres + dx is most of that bound); dshift 0.11 / 0.13 / 0.22 / 0.12, dscale 0.16 / 0.10 / 0.16 / 0.09, dw 0.08 / 0.11 / 0.08 / 0.09,
  db 0.16 / 0.20 / 0.14 / 0.22.  Generic kernel: dx 0.29 / 0.992, dshift 0.20, dscale 0.20, dw 0.05, db 0.11.  (The column sums' depths are
  worst cases; their rounding errors add like a square root.)
  Gate (VPL 1 / 2 / 3 / 4 / generic): out 0.997 / 0.977 / 0.986 / 0.972 / 0.992 (two roundings, one of them the output's own), dgate 0.35 /
  0.23 / 0.30 / 0.27 / 0.30; dh 1.00 by construction -- a 16-bit store is within its interval, whose far end is what the bound measures.
  RMSNorm (H d <= 512 / <= 1024 / 1280 / 2048, contiguous and packed): y and dx 1.00 by construction, dgamma 0.12 / 0.15 / 0.16 / 0.21.
  Share of 16-bit outputs whose interval holds two values (the reference alone, plain inputs; test_dit_train_conformance_ref.py prints
  them): dh under 0.02 % (bf16) / 0.04 % (fp16); RMSNorm y 0.03 % / 0.25 %, dx 0.3 % / 1.7 % at the most.
Everything here runs on torch CPU tensors in float64; pass .cpu() copies of device tensors."""
import numpy as np
import torch

import dit_train_ref as R
from gemm_ref import U32, r16, _round_bound, excess            # noqa: F401  (re-exported for the tests)

SECOND = 1.0 + 1e-3
RPW = 16                                                         # GVF_TRAIN_ROWS_PER_WG (include/gvf_dit_train.h)
F64 = torch.float64
RMS_FLOOR = 1e-12


def vec_path(C):
    return C % 256 == 0 and C <= 1024


def ln_depths(C):
    """(depth_s, depth_q, depth_g) of the module docstring."""
    if vec_path(C):
        v = C // 256
        return v + 8, v + 9, 4 * v + 6
    n = (C + 63) // 64
    return n + 6, n + 7, n + 6


# ---- the column-sum layout ----------------------------------------------------------------------------------------------------------------

def segments(rows, rpg):
    """[(workgroup, group, s0, s1)] in row order: the rows [s0, s1) of group g inside workgroup wg."""
    out = []
    for wg in range((rows + RPW - 1) // RPW):
        r0, r1 = wg * RPW, min(rows, wg * RPW + RPW)
        for g in range(r0 // rpg, (r1 - 1) // rpg + 1):
            out.append((wg, g, max(r0, g * rpg), min(r1, (g + 1) * rpg)))
    return out


def group_slots(rows, rpg):
    """(lo, hi) int64 arrays over the groups: the finaliser adds slots lo .. hi of group g (slot of (wg, g): wg + g)."""
    G = (rows + rpg - 1) // rpg
    g = np.arange(G, dtype=np.int64)
    last = np.minimum((g + 1) * rpg, rows) - 1
    return (g * rpg) // RPW + g, last // RPW + g


def colsum_depth(rows, rpg, vec, per_group):
    """Adds a term passes through: float64 tensor (G, 1) for a per-group output, (1, 1) for one that is not."""
    if per_group:
        lo, hi = group_slots(rows, rpg)
        seg = min(RPW, rpg, rows)
        in_wg = (seg + 3) // 4 + 3 if vec else seg
        slots = torch.from_numpy(hi - lo + 1).double()[:, None]
    else:
        if vec:
            per_wg = {}
            for wg, _, s0, s1 in segments(rows, rpg):
                per_wg[wg] = per_wg.get(wg, 0) + (s1 - s0 + 3) // 4            # wave 0's rows
            in_wg = max(per_wg.values()) + 3
        else:
            in_wg = min(RPW, rows)
        slots = torch.full((1, 1), float((rows + RPW - 1) // RPW), dtype=F64)
    return in_wg + torch.ceil(slots / 4) + 2


def _gsum(t, rpg):
    rows = t.shape[0]
    G = (rows + rpg - 1) // rpg
    return torch.zeros((G, t.shape[1]), dtype=F64).index_add_(0, torch.arange(rows) // rpg, t)


def colsum(ref, terms, e_terms, rows, rpg, vec, per_group):
    """(ref, bound) of a column sum whose fp32 terms (float64 values) are known to within e_terms."""
    if per_group:
        S, E = _gsum(terms.abs(), rpg), _gsum(e_terms, rpg)
    else:
        S, E = terms.abs().sum(0, keepdim=True), e_terms.sum(0, keepdim=True)
    bnd = (colsum_depth(rows, rpg, vec, per_group) * U32 * S + E) * SECOND
    return ref.reshape(bnd.shape), bnd


# ---- a. LayerNorm + adaLN backward --------------------------------------------------------------------------------------------------------

def ln_bwd(x, dy, dres=None, w=None, b=None, scale=None, rpg=None, eps=1e-6):
    """x (rows, C) fp32, dy (rows, C) 16-bit values, dres optional fp32, w / b (C,), scale (G, C) -> {name: (reference, bound)} for dx and,
    where the call has them, dshift, dscale (G, C), dw, db (1, C).  (shift enters no gradient.)"""
    rows, C = x.shape
    vec = vec_path(C)
    ds, dq, dg = ln_depths(C)
    shift = None if scale is None else torch.zeros_like(scale)
    ref = R.ln_mod(x, dy.float(), dres=dres, w=w, b=b, shift=shift, scale=scale, rpg=rpg, eps=eps)
    x, dy = x.double(), dy.double()
    mean = x.mean(1, keepdim=True)
    d = x - mean
    var = (d * d).mean(1, keepdim=True)
    rstd = 1.0 / torch.sqrt(var + eps)
    xh = d * rstd
    e_m1 = ds * U32 * x.abs().sum(1, keepdim=True) / C + U32 * mean.abs()
    abs_c = d.abs() + e_m1
    e_m2 = (ds + 1) * U32 * abs_c.sum(1, keepdim=True) / C + U32 * e_m1
    e_d = e_m2 + 2.0 * U32 * abs_c
    Q = ((d.abs() + e_d) ** 2).sum(1, keepdim=True)
    e_q = (dq + 4.1) * U32 * Q + C * e_m2 ** 2
    d_r = 0.5 * (e_q / C + U32 * var) / (var + eps) + 3.0 * U32
    e_xh = d.abs() * rstd * d_r + rstd * e_d + U32 * xh.abs()

    if scale is not None:
        m = 1.0 + scale.double()[torch.arange(rows) // rpg]
        gm = dy * m
        e_gm = 2.0 * U32 * gm.abs()
    else:
        gm, e_gm = dy, torch.zeros_like(dy)
    if w is not None:
        g = gm * w.double()
        e_g = e_gm + U32 * g.abs()
    else:
        g, e_g = gm, e_gm
    c1 = g.mean(1, keepdim=True)
    e_c1 = dg * U32 * g.abs().mean(1, keepdim=True) + e_g.mean(1, keepdim=True) + U32 * c1.abs()
    p = g * xh
    e_p = xh.abs() * e_g + g.abs() * e_xh + U32 * p.abs()
    c2 = p.mean(1, keepdim=True)
    e_c2 = dg * U32 * p.abs().mean(1, keepdim=True) + e_p.mean(1, keepdim=True) + U32 * c2.abs()
    inner = g - c1 - xh * c2
    e_in = e_g + e_c1 + xh.abs() * e_c2 + c2.abs() * e_xh + U32 * ((xh * c2).abs() + (g - c1).abs() + inner.abs())
    t = rstd * inner
    e_dx = rstd * (e_in + d_r * inner.abs()) + U32 * t.abs()
    if dres is not None:
        e_dx = e_dx + U32 * ref["dx"].abs()
    out = {"dx": (ref["dx"], e_dx * SECOND)}
    if scale is not None:
        if w is not None:
            a = xh * w.double() + b.double()
            e_a = w.double().abs() * e_xh + U32 * (xh * w.double()).abs() + U32 * a.abs()
        else:
            a, e_a = xh, e_xh
        ta = dy * a
        out["dshift"] = colsum(ref["dshift"], dy, torch.zeros_like(dy), rows, rpg, vec, True)
        out["dscale"] = colsum(ref["dscale"], ta, dy.abs() * e_a + U32 * ta.abs(), rows, rpg, vec, True)
    if w is not None:
        tw = gm * xh
        seg_rpg = rpg if scale is not None else rows
        out["dw"] = colsum(ref["dw"], tw, xh.abs() * e_gm + gm.abs() * e_xh + U32 * tw.abs(), rows, seg_rpg, vec, False)
        out["db"] = colsum(ref["db"], gm, e_gm, rows, seg_rpg, vec, False)
    return out


# ---- b. gated residual ----------------------------------------------------------------------------------------------------------------------

def gate_fwd_bwd(x, h, dout, gate=None, rpg=None, dt=None):
    """x, dout (rows, C) fp32, h (rows, C) 16-bit values, gate (G, C) -> {out, dh, dgate: (reference, bound)}; dt: the 16-bit type of dh."""
    rows, C = x.shape
    ref = R.gate(x, h.float(), dout, gate, rpg)
    x, h, dout = x.double(), h.double(), dout.double()
    gh = ref["out"] - x
    out = {"out": (ref["out"], (U32 * gh.abs() + U32 * ref["out"].abs()) * SECOND)}
    if gate is None:
        out["dh"] = (ref["dh"], _round_bound(ref["dh"], torch.zeros_like(dout), dt))
        return out
    out["dh"] = (ref["dh"], _round_bound(ref["dh"], U32 * ref["dh"].abs() * SECOND, dt))
    t = dout * h
    out["dgate"] = colsum(ref["dgate"], t, U32 * t.abs(), rows, rpg, vec_path(C), True)
    return out


# ---- c. multi-head RMSNorm --------------------------------------------------------------------------------------------------------------------

def rms_fwd_bwd(x, dy, gamma, dt):
    """x, dy (rows, H, d) 16-bit values, gamma (H, d) fp32 -> {y, dx: (reference, E, bound), dgamma: (reference, bound)}: for the 16-bit outputs
    E bounds the fp32 value before the store and bound is the interval form."""
    rows, H, d = x.shape
    ref = R.rms(x.float(), dy.float(), gamma)
    x, dy, gm = x.double(), dy.double(), gamma.double()
    levels = 2 if d == 32 else 3
    c = 1.0 if d == 32 else 0.0
    d_den = (0.5 * (9 + levels) + 1.0) * U32
    den = torch.sqrt((x * x).sum(2, keepdim=True)).clamp_min(RMS_FLOOR)
    xt = x / den
    sq = float(d) ** 0.5
    E_y = ref["y"].abs() * (d_den + (3.0 + c) * U32) * SECOND
    u = dy * gm * sq
    e_xt = (d_den + U32) * xt.abs()
    e_u = (2.0 + c) * U32 * u.abs()
    p = u * xt
    e_p = u.abs() * e_xt + xt.abs() * e_u + U32 * p.abs()
    dot = p.sum(2, keepdim=True)
    e_dot = (8 + levels) * U32 * p.abs().sum(2, keepdim=True) + e_p.sum(2, keepdim=True)
    inner = u - xt * dot
    E_dx = ((e_u + dot.abs() * e_xt + xt.abs() * e_dot + U32 * (xt * dot).abs() + U32 * inner.abs()) / den + (d_den + U32) * ref["dx"].abs()) * SECOND
    t = (dy * xt).reshape(rows, H * d)
    e_t = (dy.abs() * e_xt + U32 * (dy * xt).abs()).reshape(rows, H * d)
    _, b_sum = colsum(ref["dgamma"].reshape(1, H * d) / sq, t, e_t, rows, rows, True, False)
    dgam = ref["dgamma"].reshape(1, H * d)
    return {"y": (ref["y"], E_y, _round_bound(ref["y"], E_y, dt)), "dx": (ref["dx"], E_dx, _round_bound(ref["dx"], E_dx, dt)),
            "dgamma": (dgam, sq * b_sum + (1.0 + c) * U32 * dgam.abs() * SECOND)}


def check16(out, ref, E, dt):
    """(elements outside [R16(ref - E), R16(ref + E)], largest |out - ref| / bound over the elements whose bound is finite)."""
    o, ref = out.double().reshape(ref.shape), ref
    lo, hi = r16(ref - E, dt), r16(ref + E, dt)
    bad = ~((o >= lo) & (o <= hi))
    bnd = torch.maximum((hi - ref).abs(), (lo - ref).abs())
    fin = torch.isfinite(bnd) & torch.isfinite(o)
    ratio = excess(o[fin], ref[fin], bnd[fin])[1] if bool(fin.any()) else 0.0
    return int(bad.sum()), ratio


def ambiguous_share(ref, E, dt):
    """Share of 16-bit outputs whose interval spans more than one value (from the reference alone)."""
    return float((r16(ref + E, dt) != r16(ref - E, dt)).double().mean())


# ---- test data: the matrix of tests/test_dit_train_conformance_gpu.py, shared with tests/test_dit_train_conformance_ref.py ------------------

# C, rows, rows_per_group
LN_CASES = [(256, 37, 10), (768, 50, 7), (1024, 33, 33), (512, 163, 81), (256, 4099, 2050), (256, 1100, 1), (512, 20, 48), (100, 163, 81),
            (1028, 41, 7), (64, 1100, 1)]
# rows, H, d
RMS_CASES = [(37, 2, 32), (130, 16, 32), (19, 17, 32), (41, 12, 64), (41, 16, 64), (19, 40, 32), (19, 32, 64)]
RMS_PACKED = [(130, 16, 32), (41, 12, 64), (19, 32, 64)]         # one case of each NCH through the packed [q | k | v] layout
MODES = ["affine", "adaln", "both", "neither"]
NAN = float("nan")


def adversarial_rows(C, rows, g):
    """the rows of tests/test_dit_train_ops_gpu.py::_ln_rows (a common offset of 100 sigma, constant rows, huge elements)"""
    x = torch.randn((rows, C), generator=g) * 2 + 0.5
    x[0:3] += 200.0
    for r, v in zip(range(3, min(6, rows)), (3.0, -0.37, 0.0)):
        x[r] = v
    x[6:8, 1::29] = 1e4
    return x


def _row_scales(rows, g):
    return 10.0 ** (-4.0 * torch.rand((rows, 1), generator=g))


def make_ln(C, rows, rpg, dt, plain=False):
    """Inputs of one LayerNorm-backward case; the modulation table is [4 | shift C | 4 | scale C | 4] with NaN in the padding.  plain: no
    adversarial rows, no 1 + scale = 0 columns, no zero or scaled-down gradient."""
    g = torch.Generator().manual_seed(C * 7 + rows + 1000 * rpg)
    G = (rows + rpg - 1) // rpg
    x = torch.randn((rows, C), generator=g) * 2 + 0.5 if plain else adversarial_rows(C, rows, g)
    ld = 2 * C + 12
    mod = torch.full((G, ld), NAN)
    mod[:, 4:4 + C] = torch.randn((G, C), generator=g) * 0.3
    mod[:, 8 + C:8 + 2 * C] = torch.randn((G, C), generator=g) * 0.3
    dy = torch.randn((rows, C), generator=g)
    if not plain:
        mod[-1, 8 + C:8 + C + C // 2] = -1.0                       # 1 + scale = 0 in half of the last group's columns
        dy = dy * _row_scales(rows, g)                           # small rows are judged on their own magnitude
        dy[:, 5:9] = 0                                           # columns whose four sums are zero in exact arithmetic
    return dict(C=C, rows=rows, rpg=rpg, G=G, x=x, dy=dy.to(dt), dres=torch.randn((rows, C), generator=g), mod=mod, ld=ld, scale_off=8 + C,
                scale=mod[:, 8 + C:8 + 2 * C], w=1 + 0.1 * torch.randn((C,), generator=g), b=0.1 * torch.randn((C,), generator=g))


def ln_args(d, mode, with_dres):
    has_mod, has_aff = mode in ("adaln", "both"), mode in ("affine", "both")
    return dict(dres=d["dres"] if with_dres else None, w=d["w"] if has_aff else None, b=d["b"] if has_aff else None,
                scale=d["scale"] if has_mod else None, rpg=d["rpg"] if has_mod else None)


def make_gate(C, rows, rpg, dt, plain=False):
    """the gate table is [4 | gate C | 4] with NaN in the padding"""
    g = torch.Generator().manual_seed(C * 3 + rows + 1000 * rpg)
    G = (rows + rpg - 1) // rpg
    ld = C + 8
    tab = torch.full((G, ld), NAN)
    tab[:, 4:4 + C] = torch.randn((G, C), generator=g)
    x, dout = torch.randn((rows, C), generator=g), torch.randn((rows, C), generator=g)
    h = (torch.randn((rows, C), generator=g) * 3).to(dt)
    if not plain:
        dout = dout * _row_scales(rows, g)
        dout[:, 2:4] = 0                                         # dgate columns that are zero in exact arithmetic
    return dict(C=C, rows=rows, rpg=rpg, G=G, x=x, h=h, dout=dout, tab=tab, ld=ld, gate=tab[:, 4:4 + C])


def rms_special(rows, H):
    """{name: (row, head)} of the planted heads, and the planted all-zero row."""
    return dict(big=(1, 0), small=(2, H - 1), one=(3, 0), zero=(4, H - 1)), rows // 2


def make_rms(rows, H, d, dt, plain=False, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(rows * 5 + H + d + 100 * seed)
    gamma = 1 + 0.2 * torch.randn((H, d), generator=g)
    dy = torch.randn((rows, H, d), generator=g)
    x = torch.randn((rows, H, d), generator=g) * scale
    heads, zero_row = rms_special(rows, H)
    if not plain:
        sc = _row_scales(rows, g)
        sc[zero_row] = 1.0                                       # the all-zero row keeps the exact-value check of the existing test
        dy = dy * sc[:, :, None]
        x[heads["big"]] = (torch.randn((d,), generator=g) * 1e4).clamp(-6e4, 6e4)
        x[heads["small"]] = torch.randn((d,), generator=g) * 1e-3
        x[heads["one"]] = 0
        x[heads["one"]][d // 3] = -1.7
        x[heads["zero"]] = 0
        x[zero_row] = 0                                          # dx = u / 1e-12 there
    return dict(rows=rows, H=H, d=d, x=x.to(dt), dy=dy.to(dt), gamma=gamma, zero_row=None if plain else zero_row)
