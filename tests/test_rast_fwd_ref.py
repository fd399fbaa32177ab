"""Host tests of the forward conformance machinery (tests/rast_fwd_ref.py, oracle gvfo64_blend / gvfo32_blend / gvfo32_project): the measure
that tests/test_rast_fwd_conformance_gpu.py holds the device to must bite.  No GPU.

The stand-in candidate is the fp32 yardstick itself: rast32_project's records, the full 3-sigma lists sorted by those records' depth bits,
and rast32_blend(form=1) of them.  Unmutated it passes every bar with ratio 1; each of the perturbed candidates below fails:
  stage A   conic b x (1 + 1e-5); opacity_eff x (1 + 4e-6)
  stage B   one adjacent pair of one tile swapped; one contributing list member dropped (a member that reaches alpha >= 1/255 nowhere in its
            tile may be dropped: that is the forward's culled binning)
  stage C   (mutants 8 .. 11 of the yardstick library) skip threshold 1/256 for 1/255; clamp 0.995 for 0.99; the T-stop applied after
            compositing the splat instead of in front of it; every exp result x (1 + 3e-6)
Two scenes: `opaque`, the narrow diff_gauss scene with every third opacity raised to 1 (reaches the clamp), and `crowded`, the backward
conformance's scene of 700 faint Gaussians on four tiles (T runs out at the image centre).  The clamp mutant can only show in the first
(crowded keeps opacity <= 0.05: there it must change nothing); which scene must catch which mutant is asserted.  Measured here
(candidate : yardstick, max/p99 of e, worst channel):
  threshold 1/256     opaque  colour 3.3e5/6.4 : 19/5.8, and a pixel outside every footprint is no longer the exact background; crowded alike
  clamp 0.995         opaque  colour 5.1e4/6.3 : 19/5.8 (ratio 2688); crowded: bit-identical
  T-stop late         opaque  colour 6.9e4/6.1 : 19/5.8 (ratio 3633); crowded depth 106/93 : 20/13 (7.4), colour 124/73 : 28/15 (5.0)
  exp x (1 + 3e-6)    opaque  colour 3013/43 : 19/5.8 (ratio 158); crowded depth 62/56 : 20/13 (4.5: not relied on)
  conic b, opacity    ratio 26 .. 41 resp. infinite (diff_gauss opacity_eff is the input itself: the yardstick's error is 0)
Also here: DESIGN's accuracy claim for the Cholesky form of the exponent, the workspace-layout mirror against the library's byte count,
and rast64_blend over its own lists against rast64_forward.
"""
import numpy as np
import pytest

import oracle
import rast_bwd_ref as R
import rast_fwd_ref as F
from rast_util import cached
from test_rast_bwd_conformance_gpu import SINGLE

SCENES = ("opaque", "crowded")


def _scene(name):
    def make():
        c = F.opaque_case() if name == "opaque" else R.make_case(**SINGLE["crowded"])
        ref = F.reference(c.ins, c.kw, c.sub)
        rec32 = ref["proj32"]["out"]
        assert np.array_equal((ref["proj32"]["flags"] & oracle.FLAG_VISIBLE) != 0, ref["vis"])
        bits = np.ascontiguousarray(rec32[:, 9]).view(np.uint32)
        ranges, ids = F.full_lists(ref["rects"], bits, c.H, c.W)
        geo = dict(bg=c.kw["bg"], H=c.H, W=c.W)
        ref64 = oracle.rast64_blend(rec32.astype(np.float64), ranges=ranges, ids=ids, want_power=True, **geo)
        yard = oracle.rast32_blend(rec32, form=1, ranges=ranges, ids=ids, want_power=True, **geo)
        return dict(c=c, ref=ref, rec32=rec32, bits=bits, ranges=ranges, ids=ids, geo=geo, ref64=ref64, yard=yard)
    return cached(("rast_fwd_ref", name), make)


def _fails(check):
    """True when the check raises or reports a row beyond the bar."""
    try:
        return bool(F.beyond(check()))
    except AssertionError as e:
        print("  rejected:", str(e)[:160])
        return True


@pytest.mark.parametrize("name", SCENES)
def test_caps_hold_and_the_unmutated_candidate_passes_with_ratio_one(name):
    s = _scene(name)
    c, ref = s["c"], s["ref"]
    assert not ref["ties"], ref["ties"]
    assert (s["ref64"]["flags"] != 0).mean() <= F.MAX_FLAGGED_PIXELS
    rep = F.projection_report(name, s["rec32"], ref["proj64"], ref["proj32"], c.H, c.W)        # asserts the 1 % cap of flagged Gaussians
    F.check_lists(name, s["rec32"].astype(np.float64), s["bits"], s["ranges"], s["ids"], ref["rects"], len(s["ids"]), **s["geo"])
    rep += F.blend_report(name, s["yard"], s["ref64"], s["yard"], c.kw["bg"])
    F.assert_report(name, rep)
    assert all(row[3] in (0.0, 1.0) for row in rep), rep
    assert ref["vis"].sum() > 500 and len(s["ids"]) > 1000
    if name == "opaque":
        assert F.clamp_active(s["rec32"].astype(np.float64), s["ranges"], s["ids"], **s["geo"]) >= 10
    else:
        assert (s["ranges"][:, 1] - s["ranges"][:, 0]).max() > 512


@pytest.mark.parametrize("name", SCENES)
@pytest.mark.parametrize("col,eps", [(3, 1e-5), (5, 4e-6)], ids=["conic_b", "opacity"])
def test_perturbed_records_fail_stage_a(name, col, eps):
    s = _scene(name)
    c, ref = s["c"], s["ref"]
    got = s["rec32"].astype(np.float64)
    got[:, col] *= 1.0 + eps
    rep = F.projection_report(f"{name} x(1+{eps:g})", got.astype(np.float32), ref["proj64"], ref["proj32"], c.H, c.W)
    bad = [row[0] for row in F.beyond(rep)]
    assert bad == ["A " + F.COLS[col]], bad                   # that column, and no other


@pytest.mark.parametrize("name", SCENES)
def test_broken_lists_fail_stage_b(name):
    s = _scene(name)
    ref, ranges, ids, geo = s["ref"], s["ranges"], s["ids"], s["geo"]
    rec = s["rec32"].astype(np.float64)
    check = lambda r, i: F.check_lists(name, rec, s["bits"], r, i, ref["rects"], len(i), **geo)
    # the largest opacity * G each list entry reaches over its tile (fp64)
    reach = (rec[ids, 5][:, None, None] * 2.0 ** s["ref64"]["power"]).reshape(len(ids), -1).max(axis=1)
    tile_of = np.repeat(np.arange(len(ranges)), ranges[:, 1] - ranges[:, 0])
    # one adjacent pair of one tile swapped
    t = int(np.argmax(ranges[:, 1] - ranges[:, 0]))
    swapped = ids.copy()
    b = ranges[t, 0]
    swapped[[b, b + 1]] = swapped[[b + 1, b]]
    with pytest.raises(AssertionError, match="not sorted"):
        check(ranges, swapped)

    def without(k):
        r = ranges.copy()
        r[tile_of[k], 1] -= 1
        r[tile_of[k] + 1:] -= 1
        return r, np.delete(ids, k)
    # one contributing member dropped: the entry that reaches the largest alpha
    with pytest.raises(AssertionError, match="missing"):
        check(*without(int(np.argmax(reach))))
    # a member that stays under 1/255 everywhere in its tile contributes nothing: dropping it is what the culled binning does (the crowded
    # scene has no such pair: every Gaussian is wide enough to reach all four tiles)
    faint = np.flatnonzero(reach < 0.9 / 255.0)
    assert (faint.size > 0) == (name == "opaque")
    if faint.size:
        check(*without(int(faint[0])))
        # ... unless the binning rule says the pair belongs there: held to a rule's rects, the lists must hold exactly its members
        exact = lambda r, i: F.check_lists(name, rec, s["bits"], r, i, ref["rects"], len(i), binned_rects=ref["rects"], **geo)
        exact(ranges, ids)
        with pytest.raises(AssertionError, match="binning rule"):
            exact(*without(int(faint[0])))
    # a duplicate, a member from outside its rect, a wrong count
    dup = ids.copy()
    dup[b + 1] = dup[b]
    with pytest.raises(AssertionError, match="twice|not sorted"):
        check(ranges, dup)
    with pytest.raises(AssertionError, match="reported"):
        F.check_lists(name, rec, s["bits"], ranges, ids, ref["rects"], len(ids) + 1, **geo)
    outside = np.flatnonzero(~np.isin(np.arange(len(rec)), ids[ranges[t, 0]:ranges[t, 1]]) & ref["vis"])
    if outside.size:
        foreign = ids.copy()
        foreign[b] = outside[0]
        with pytest.raises(AssertionError):
            check(ranges, foreign)


# mutant -> the scenes that must catch it (see the module docstring)
_BLEND_MUTANTS = {8: ("threshold 1/256 instead of 1/255", ("opaque", "crowded")), 9: ("clamp 0.995 instead of 0.99", ("opaque",)),
                  10: ("T-stop after compositing the splat", ("opaque", "crowded")), 11: ("exp results x (1 + 3e-6)", ("opaque",))}


@pytest.mark.parametrize("mutant", list(_BLEND_MUTANTS))
def test_blend_mutants_fail_stage_c(mutant):
    what, must = _BLEND_MUTANTS[mutant]
    for name in SCENES:
        s = _scene(name)
        mut = oracle.rast32_blend(s["rec32"], form=1, ranges=s["ranges"], ids=s["ids"], mutant=mutant, **s["geo"])
        same = all(np.array_equal(mut[k], s["yard"][k]) for k in ("color", "alpha", "depth"))
        failed = _fails(lambda: F.blend_report(f"{name} mutant {mutant} ({what})", mut, s["ref64"], s["yard"], s["c"].kw["bg"]))
        if name in must:
            assert failed, f"{what}: passes the bar on {name}"
        elif mutant == 9:
            assert same, "the clamp changed an image whose opacities stay under 0.05"
    assert not hasattr(oracle.lib(), "gvfo64_set_mutant"), "the mutant switch leaked into the fp64 build"


@pytest.mark.parametrize("name", SCENES)
def test_cholesky_form_keeps_the_accuracy_design_claims(name):
    """csrc/rast_common.h and DESIGN: the tile-relative Cholesky evaluation costs ~1e-5 of the exponent.  Over every (list entry, pixel)
    pair of the scene, exponents in octaves as the kernel holds them: |form 1 - fp64| <= 1e-5 |exponent| + 2^-20."""
    s = _scene(name)
    p64, p32 = s["ref64"]["power"], s["yard"]["power"].astype(np.float64)
    d = np.abs(p32 - p64)
    bound = 1e-5 * np.abs(p64) + 2.0 ** -20
    print(f"{name}: {d.size} exponents, largest |exponent| {np.abs(p64).max():.0f} octaves, worst error / bound {(d / bound).max():.3f}")
    assert d.size > 100000 and (d <= bound).all()


def test_blend_over_its_own_lists_is_the_forward():
    """lists = NULL: rast64_blend builds the 3-sigma lists as pixel_list() does and reproduces rast64_forward."""
    c = R.make_case(**SINGLE["narrow-dilate-sh2"])
    assert c.sub is None
    ref = F.reference(c.ins, c.kw)
    want = oracle.rast64_forward(*c.ins, **c.kw)
    got = oracle.rast64_blend(ref["proj64"]["out"], rects=ref["rects"], bg=c.kw["bg"], H=c.H, W=c.W)
    for k in ("color", "alpha", "depth"):
        assert np.abs(got[k] - want[k]).max() <= 1e-13, k
    assert float(want["alpha"].max()) > 0.5
    # and the explicit full lists give the same image again
    bits = np.ascontiguousarray(ref["proj64"]["out"][:, 9].astype(np.float32)).view(np.uint32)
    ranges, ids = F.full_lists(ref["rects"], bits, c.H, c.W)
    again = oracle.rast64_blend(ref["proj64"]["out"], ranges=ranges, ids=ids, bg=c.kw["bg"], H=c.H, W=c.W)
    assert all(np.array_equal(again[k], got[k]) for k in ("color", "alpha", "depth", "flags"))


WORKSPACES = [(0, 1, 64, 64, 0), (0, 3, 40, 72, 65536), (1, 1, 16, 16, 1), (97, 1, 32, 32, 0), (257, 1, 32, 32, 65536), (300, 5, 64, 64, 65536),
              (600, 1, 64, 80, 2400), (700, 1, 32, 32, 65536), (4096, 4, 64, 64, 65536), (5000, 8, 64, 64, 160000),
              (5000, 8, 800, 800, 12345), (262144, 24, 800, 800, 25165824), (1000, 2, 4100, 17, 999)]


@pytest.mark.parametrize("P,Fr,H,W,cap", WORKSPACES)
def test_workspace_mirror_equals_the_library(P, Fr, H, W, cap):
    layout, total = F.carve(P, Fr, H, W, cap)
    assert total == F.library_workspace_bytes(P, Fr, H, W, cap) - 256
    assert all(start % 256 == 0 for start, _, _ in layout.values())
