"""Helpers of the stage-wise conformance check of the rasteriser FORWARD (tests/test_rast_fwd_ref.py on the host,
tests/test_rast_fwd_conformance_gpu.py on the device): a Python mirror of the workspace layout (gvf_rast::carve, csrc/rast.hip) through which
the tests read what the forward left behind -- no C entry point is added for them --, the unpacking of the 64-byte splat record
(DESIGN 2.2), and the three stages' measures.

  stage A, projection   the ten per-Gaussian quantities of the record against rast64_project, per column:
                        e = |got - ref| / (2^-24 * s);  s = |ref| for conic a, conic c, opacity_eff, depth;  max(|x|, W/2) resp. max(|y|, H/2)
                        for x, y;  sqrt(a c) for conic b;  max(|ref|, 0.5) for r, g, b
  stage B, lists        integer work, exact: no duplicates, sorted by (fp32 depth bits of the candidate's own record, id), members only inside
                        the oracle's tile rect, sum of the lengths = num_rendered, and COMPLETE: rast64_blend of the candidate's records over
                        the candidate's lists and over the full 3-sigma lists agree to 1e-12 on every unflagged pixel
  stage C, blend        colour, alpha, depth against rast64_blend of the candidate's own records over the candidate's own lists:
                        e = |got - ref| / (2^-24 * s) with the oracle's scales (sum of the absolute terms); s = 0 -> exactly bg / 0
Bar of A and C: the candidate's maximum and 99th percentile of e are each <= FACTOR = 4 x those of the fp32 yardstick on the same inputs
(rast32_project; rast32_blend(form=1), the device's documented algorithm in plain C) -- rast_bwd_ref.within, the project's rule for
"another operation order, not another algorithm".  The yardstick, never the candidate, sets the bar.  (For stage C the yardstick gets the
device's records as this file unpacks them, rounded to fp32, and scales the conic again: one or two roundings of the conic that the device
does not have -- ~1e-7 of the exponent, against the ~1e-6 the tile-relative Cholesky evaluation itself costs.)
"""
import ctypes
import math

import numpy as np

import oracle
import rast_bwd_ref as R
from gvfdiffusion_amd import _lib

U = R.U
COLS = ("x", "y", "conic_a", "conic_b", "conic_c", "opacity", "r", "g", "b", "depth")
MAX_FLAGGED_PIXELS = 0.03
MAX_FLAGGED_GAUSSIANS = 0.01
COMPLETE_ATOL = 1e-12

# ---- the workspace layout: gvf_rast::carve restated (csrc/rast.hip; constants of csrc/rast_plan.h) ----------------------------------
TILE = 16
PRE_THREADS = 256
SCAN_CHUNK = 4096
MORTON_BINS = 1 << 15
LAYOUT_WORD = 6
LAYOUT_SLOT_ORDER = 1
ALIGN = 256


def carve(P, F, H, W, max_rendered):
    """(layout, total): layout[name] = (byte offset, element count, element bytes) in the order carve() takes them -- every take starts at
    the next multiple of 256 --, total = the carved size rounded up to 256 = gvf_rast_workspace_bytes(...) - 256."""
    nb = (P + PRE_THREADS - 1) // PRE_THREADS
    ntiles = ((W + TILE - 1) // TILE) * ((H + TILE - 1) // TILE)
    FP = F * max(P, 1)
    D = max(int(max_rendered), 1)
    Pp = max(P, 1)
    takes = [("frames", F, ctypes.sizeof(_lib.GvfRastFrame)), ("splats", 4 * FP, 16), ("tiles_touched", FP, 4), ("radii", FP, 4),
             ("block_sums", F * max(nb, 1), 4), ("frame_base", F + 1, 4), ("total", 1, 4), ("keys", D, 8), ("keys_alt", D, 8),
             ("vals", D, 4), ("vals_alt", D, 4), ("ids", D, 4), ("ranges", F * ntiles, 8), ("cls", 2 + 2 * F * ntiles, 4),
             ("tile_count", F * ntiles, 4), ("cursor", F * ntiles, 4), ("partial", (F * ntiles + SCAN_CHUNK - 1) // SCAN_CHUNK + 1, 4),
             ("order", Pp, 4), ("order_alt", Pp, 4), ("mhist", MORTON_BINS, 4), ("mm", 8, 4), ("binrec", FP, 16),
             ("sort_tmp", int(_lib.lib().gvf_sort_tmp_bytes(D)), 1)]
    layout, off = {}, 0
    for name, count, size in takes:
        start = (off + ALIGN - 1) // ALIGN * ALIGN
        layout[name] = (start, count, size)
        off = start + count * size
    return layout, (off + ALIGN - 1) // ALIGN * ALIGN


def library_workspace_bytes(P, F, H, W, max_rendered):
    out = ctypes.c_size_t(0)
    _lib.check(_lib.lib().gvf_rast_workspace_bytes(P, F, H, W, max_rendered, ctypes.byref(out)), "gvf_rast_workspace_bytes")
    return int(out.value)


def read_workspace(fwd, P, F, H, W):
    """numpy views of what a forward call with private_workspace=True left in its workspace: splats[F, P, 16] (fp32), radii[F, P],
    ranges[F, ntiles, 2], ids[D], order_alt[P], mm[8] (mm[LAYOUT_WORD] bit 0: the record of Gaussian id sits at order_alt[id])."""
    layout, total = carve(P, F, H, W, fwd["max_rendered"])
    assert total + 256 == fwd["workspace_bytes"], "the workspace mirror disagrees with the call's workspace size"
    ws = fwd["workspace"]
    raw = ws.cpu().numpy()[(-ws.data_ptr()) % 256:]
    ntiles = ((W + TILE - 1) // TILE) * ((H + TILE - 1) // TILE)

    def view(name, dtype):
        start, count, size = layout[name]
        return raw[start:start + count * size].view(dtype)

    return dict(splats=view("splats", np.float32).reshape(F, max(P, 1), 16), radii=view("radii", np.int32).reshape(F, max(P, 1)),
                ranges=view("ranges", np.uint32).astype(np.int64).reshape(F, ntiles, 2), ids=view("ids", np.uint32).astype(np.int64),
                order_alt=view("order_alt", np.uint32).astype(np.int64), mm=view("mm", np.uint32))


# the record holds the conic pre-scaled for the blend: (a', b', c') = (-0.5 log2e a, -log2e b, -0.5 log2e c)
CONIC_IK1 = -2.0 * math.log(2.0)
CONIC_IK2 = -math.log(2.0)


def unpack_records(splats, visible, rec_of=None):
    """splats[P, 16] of one frame -> (rec[P, 10] float64 in rast64_project's order, depth_bits[P] uint32): the conic un-scaled by the exact
    float64 values -2 ln 2 and -ln 2.  rec_of: the record of Gaussian id sits at splats[rec_of[id]] (slot order).  Records of invisible
    Gaussians are not read: their rows are zero."""
    s = splats if rec_of is None else splats[rec_of]
    rec = np.zeros((s.shape[0], 10))
    bits = np.zeros((s.shape[0],), np.uint32)
    v = np.asarray(visible, bool)
    d = s[v].astype(np.float64)
    rec[v] = np.stack([d[:, 0], d[:, 1], d[:, 2] * CONIC_IK1, d[:, 3] * CONIC_IK2, d[:, 4] * CONIC_IK1, d[:, 5], d[:, 6], d[:, 7], d[:, 8],
                       d[:, 9]], 1)
    bits[v] = np.ascontiguousarray(s[v, 9]).view(np.uint32)
    return rec, bits


# ---- stage A -------------------------------------------------------------------------------------------------------------------------
def projection_scales(ref, H, W):
    a = np.abs(ref)
    s = a.copy()
    s[:, 0] = np.maximum(a[:, 0], 0.5 * W)
    s[:, 1] = np.maximum(a[:, 1], 0.5 * H)
    s[:, 3] = np.sqrt(a[:, 2] * a[:, 4])
    s[:, 6:9] = np.maximum(a[:, 6:9], 0.5)
    return s


def projection_report(label, got, proj64, proj32, H, W, binned=None):
    """Per column (name, candidate (max, p99), yardstick (max, p99), ratio) over the visible Gaussians without FLAG_NEAR -- of a device's
    records only those the oracle bins to at least one tile (`binned`): the front end leaves the record of a Gaussian that the culled
    binning drops from every tile of its 3-sigma rect unwritten (zeros), and nothing reads it.  Asserts the share of flagged Gaussians and
    that a quantity whose reference is exactly zero (a mip coefficient of 0) comes out exactly zero."""
    ref, fl = proj64["out"], proj64["flags"]
    vis, near = (fl & oracle.FLAG_VISIBLE) != 0, (fl & oracle.FLAG_NEAR) != 0
    assert (near & vis).sum() <= MAX_FLAGGED_GAUSSIANS * vis.sum(), f"{label}: {(near & vis).sum()} of {vis.sum()} visible Gaussians sit at a threshold"
    keep = vis & ~near if binned is None else vis & ~near & binned
    s = projection_scales(ref, H, W)[keep]
    got, yard, ref = np.asarray(got, np.float64)[keep], np.asarray(proj32["out"], np.float64)[keep], ref[keep]
    report = []
    for k, name in enumerate(COLS):
        nz = s[:, k] > 0
        assert (got[~nz, k] == 0).all(), f"{label} {name}: not exactly zero where the reference is"
        e_dev = np.abs(got[nz, k] - ref[nz, k]) / (U * s[nz, k])
        e_yard = np.abs(yard[nz, k] - ref[nz, k]) / (U * s[nz, k])
        report.append(judge(label, "A " + name, R.stats(e_dev), R.stats(e_yard)))
    return report


# ---- stage B -------------------------------------------------------------------------------------------------------------------------
def full_lists(rects, depth_bits, H, W):
    """The 3-sigma lists: per tile every Gaussian whose rect covers it, sorted by (depth bits, id) -> (ranges[ntiles, 2], ids)."""
    gx, gy = (W + TILE - 1) // TILE, (H + TILE - 1) // TILE
    key = (depth_bits.astype(np.int64) << 32) | np.arange(len(depth_bits), dtype=np.int64)
    ranges, ids = np.zeros((gx * gy, 2), np.int64), []
    n = 0
    for ty in range(gy):
        for tx in range(gx):
            m = np.flatnonzero((rects[:, 0] <= tx) & (tx < rects[:, 2]) & (rects[:, 1] <= ty) & (ty < rects[:, 3]))
            m = m[np.argsort(key[m], kind="stable")]
            ranges[ty * gx + tx] = (n, n + len(m))
            ids.append(m)
            n += len(m)
    return ranges, (np.concatenate(ids) if ids else np.zeros((0,), np.int64))


def check_lists(label, rec, depth_bits, ranges, ids, rects, num_rendered, *, bg, H, W, sub=None, binned_rects=None):
    """Stage B on one frame; ranges index `ids` (already rebased to the frame).  binned_rects[P, 4] (a device's lists): the tile rects of
    the fp32 oracle's binning rule, which the device shares bit for bit -- every tile's list must then hold exactly the
    Gaussians whose binned rect covers it.  Returns the fp64 blend over the candidate's lists (stage C's reference)."""
    gx = (W + TILE - 1) // TILE
    key = (depth_bits.astype(np.int64) << 32) | np.arange(len(depth_bits), dtype=np.int64)
    for t, (b, e) in enumerate(ranges):
        lst = ids[b:e]
        tx, ty = t % gx, t // gx
        assert len(np.unique(lst)) == len(lst), f"{label}: tile {t} lists a Gaussian twice"
        assert (np.diff(key[lst]) > 0).all(), f"{label}: tile {t} is not sorted by (depth bits, id)"
        r = rects[lst]
        assert ((r[:, 0] <= tx) & (tx < r[:, 2]) & (r[:, 1] <= ty) & (ty < r[:, 3])).all(), f"{label}: tile {t} lists a Gaussian whose rect does not cover it"
        if binned_rects is not None:
            q = binned_rects
            want = np.flatnonzero((q[:, 0] <= tx) & (tx < q[:, 2]) & (q[:, 1] <= ty) & (ty < q[:, 3]))
            assert np.array_equal(np.sort(lst), want), f"{label}: tile {t} does not hold the Gaussians the oracle's binning rule puts there"
    total = int((ranges[:, 1] - ranges[:, 0]).sum())
    assert total == num_rendered, f"{label}: the lists hold {total} instances, the call reported {num_rendered}"
    mine = oracle.rast64_blend(rec, ranges=ranges, ids=ids, subpixel_offset=sub, bg=bg, H=H, W=W)
    full = oracle.rast64_blend(rec, rects=rects, subpixel_offset=sub, bg=bg, H=H, W=W)
    clean = (mine["flags"] == 0) & (full["flags"] == 0)
    for k in ("color", "alpha", "depth"):
        d = np.abs(mine[k] - full[k])[..., clean]
        assert d.size == 0 or d.max() <= COMPLETE_ATOL, \
            f"{label}: {k} over the lists differs from {k} over the full 3-sigma lists by {d.max():.3e}: a contributing (Gaussian, tile) pair is missing"
    return mine


# ---- stage C -------------------------------------------------------------------------------------------------------------------------
def blend_report(label, got, ref, yard, bg, yard0=None, exclude=None):
    """got / yard / yard0: dicts with color[3,H,W], alpha[H,W], depth[H,W]; ref: rast64_blend's dict.  Per channel group (name, candidate
    stats, yardstick stats, ratio[, ratio against yard0, which carries no bar]).  Flagged pixels -- and those of `exclude`, the pixels of
    depth-tied pairs -- are left out (together at most 3 % of the image, asserted)."""
    clean = ref["flags"] == 0
    if exclude is not None:
        clean &= ~exclude
    frac = 1.0 - float(clean.mean())
    assert frac <= MAX_FLAGGED_PIXELS, f"{label}: {frac:.4f} of the pixels are threshold-flagged"
    bgv = np.asarray(bg, np.float32)
    report = []
    for name, key, skey in (("C color", "color", "s_color"), ("C alpha", "alpha", "s_alpha"), ("C depth", "depth", "s_depth")):
        s = ref[skey]
        g, r = np.asarray(got[key], np.float64), ref[key]
        nz = (s > 0) & clean
        dead = (s == 0) & clean
        want = np.broadcast_to(bgv.astype(np.float64)[:, None, None], s.shape) if key == "color" else np.zeros(s.shape)
        assert (g[dead] == want[dead]).all(), f"{label} {key}: a pixel nothing contributes to is not exactly the background / zero"
        e = lambda x: np.abs(np.asarray(x[key], np.float64) - r)[nz] / (U * s[nz])
        sd, sy = R.stats(e(got)), R.stats(e(yard))
        row = judge(label, name, sd, sy)
        if yard0 is not None:
            s0 = R.stats(e(yard0))
            row = row + (ratio_of(sd, s0),)
            print(f"{label} {name}: form-0 yardstick {s0[0]:.2f}/{s0[1]:.2f}  ratio {row[-1]:.2f} (no bar)")
        report.append(row)
    return report


# ---- the bar -------------------------------------------------------------------------------------------------------------------------
def ratio_of(dev, yard):
    one = lambda d, y: d / y if y > 0 else (0.0 if d == 0 else math.inf)
    return max(one(dev[0], yard[0]), one(dev[1], yard[1]))


def judge(label, name, dev, yard):
    ratio = ratio_of(dev, yard)
    print(f"{label} {name}: candidate max/p99 {dev[0]:.2f}/{dev[1]:.2f}  yardstick {yard[0]:.2f}/{yard[1]:.2f}  ratio {ratio:.2f}")
    return (name, dev, yard, ratio)


def beyond(report):
    return [row for row in report if not R.within(row[1], row[2])]


def assert_report(label, report):
    bad = beyond(report)
    assert not bad, f"{label}: beyond {R.FACTOR} x the fp32 yardstick: " + "; ".join(
        f"{row[0]} candidate {row[1][0]:.2f}/{row[1][1]:.2f} yardstick {row[2][0]:.2f}/{row[2][1]:.2f} ratio {row[3]:.2f}" for row in bad)


# ---- a frame's lists out of the workspace, tied pairs, the scene that reaches the clamp -------------------------------------------------
def frame_lists(ws, f):
    """(ranges[ntiles, 2], ids) of frame f, rebased to the frame's own part of the workspace's id array; an empty tile is (0, 0)."""
    r = ws["ranges"][f]
    full = r[:, 1] > r[:, 0]
    if not full.any():
        return np.zeros_like(r), np.zeros((0,), np.int64)
    lo, hi = int(r[full, 0].min()), int(r[full, 1].max())
    out = np.where(full[:, None], r - lo, 0)
    return out, ws["ids"][lo:hi]


def tie_pixels(ties, rec, H, W, sub=None):
    """Pixels at which both Gaussians of a depth-tied pair can be composited (alpha >= 0.9 / 255 for both): the only place where the order
    of such a pair shows."""
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float64)
    if sub is not None:
        xx, yy = xx + sub[..., 0], yy + sub[..., 1]
    m = np.zeros((H, W), bool)
    for i, j in ties:
        both = np.ones((H, W), bool)
        for g in (rec[i], rec[j]):
            dx, dy = g[0] - xx, g[1] - yy
            both &= g[5] * np.exp(np.minimum(0.0, -0.5 * (g[2] * dx * dx + g[4] * dy * dy) - g[3] * dx * dy)) >= 0.9 / 255.0
        m |= both
    return m


def opaque_case():
    """The narrow diff_gauss scene of the backward conformance (narrow-dilate-sh1) with every third opacity raised to 1: without the mip
    coefficient opacity_eff is 1 there, so alpha reaches the 0.99 clamp around those centres and T runs out behind two or three of them --
    the scenes of rast_bwd_ref keep every opacity <= 0.95 and never reach the clamp."""
    c = R.make_case(P=600, H=64, W=64, deg=1, mode=1, seed=10)
    op = c.ins[3].copy()
    op[::3] = 1.0
    c.ins = c.ins[:3] + (op,) + c.ins[4:]
    return c


def clamp_active(rec, ranges, ids, *, bg, H, W, sub=None):
    """(list entry, pixel) pairs at which opacity * G exceeds 0.99 (fp64, over the whole lists; whole tiles only)."""
    assert H % TILE == 0 and W % TILE == 0
    p = oracle.rast64_blend(rec, ranges=ranges, ids=ids, subpixel_offset=sub, bg=bg, H=H, W=W, want_power=True)["power"]
    return int((np.asarray(rec)[ids, 5][:, None, None] * 2.0 ** p > 0.99).sum())


# ---- what comes from the oracle alone, per frame ------------------------------------------------------------------------------------
def reference(ins, kw, sub=None):
    """proj64 / proj32 (rast*_project), rects[P, 4] and radii[P] (the 3-sigma tile rects and integer radii), the depth ties, and
    binned_rects[P, 4] / binned[P]: the tile rect the fp32 oracle (rast_oracle.c) bins each Gaussian to -- the culled rect, or the 3-sigma
    rect under per-pixel sub-pixel offsets, which switch the culling off -- and whether it is non-empty."""
    proj64, proj32 = oracle.rast64_project(*ins, **kw), oracle.rast32_project(*ins, **kw)
    zero = np.zeros((3, kw["H"], kw["W"]), np.float32)
    A = oracle.rast64_accumulators(*ins, zero, subpixel_offset=sub, **kw)
    vis = (proj64["flags"] & oracle.FLAG_VISIBLE) != 0
    ties = R.depth_ties(A["rects"], proj64["out"][:, 9], vis)
    geom = oracle.rast_preprocess(*ins, tight=sub is None, **{k: v for k, v in kw.items() if k != "bg"})
    binned_rects = np.where(geom[:, 15:16] != 0, geom[:, 11:15], 0).astype(np.int32)
    binned = (binned_rects[:, 2] > binned_rects[:, 0]) & (binned_rects[:, 3] > binned_rects[:, 1])
    return dict(proj64=proj64, proj32=proj32, rects=A["rects"], radii=A["radii"], ties=ties, vis=vis, binned_rects=binned_rects, binned=binned)
