"""The numpy restatement of the RGBA condition preprocessing (tests/rgba_ref.py) -- what the GPU tests hold csrc/rgba.hip to -- against
Pillow itself and the reference's literal numpy lines, exhaustively where the domain is 65 536 (value, alpha) pairs.  Every mutant of the
restatement (one wrong decision each) must fail at least one of these comparisons.  A fixture pins it to the reference's own functions
(tests/golden/make_rgba_golden.py).  All comparisons are exact.  No GPU."""
import hashlib
import os

import numpy as np
import pytest
from PIL import Image

import rgba_ref as R

LANCZOS = Image.Resampling.LANCZOS
A, C = (v.astype(np.uint8) for v in np.mgrid[0:256, 0:256])            # every (alpha, value) pair


def pil_crop_resize(img, box, size):
    im = Image.fromarray(img)
    if box is not None:
        im = im.crop(box)
    return np.asarray(im.resize(size, LANCZOS))


def literal_black(rgba):
    """What trellis_image_to_3d.py:116-118 computes, as plain numpy array expressions: fp32 throughout, then uint8."""
    f = rgba.astype(np.float32) / 255
    return (f[..., :3] * f[..., 3:4] * 255).astype(np.uint8)


def literal_white(rgba):
    """What encode_in_the_wild_img_cond_dinov2_feature.py:49-65 computes, without the paste offsets: the fp32 composite and the fp32 alpha are
    assigned into float64 canvases (np.ones / np.zeros), which are multiplied by 255 and cast."""
    f = rgba.astype(np.float32) / 255
    alpha64 = np.zeros(rgba.shape[:2] + (1,))
    alpha64[:] = f[..., 3:4]
    rgb64 = np.ones(rgba.shape[:2] + (3,))
    rgb64[:] = f[..., :3] * f[..., 3:4] + (1 - f[..., 3:4]) * 1.0
    return (rgb64 * 255).astype(np.uint8), (alpha64 * 255).astype(np.uint8).squeeze()


def literal_float(rgba):
    """What encode_img_cond_dinov2_feature.py:42-43 computes: fp32, not rounded."""
    f = rgba.astype(np.float32) / 255
    return f[..., :3] * f[..., 3:]


def test_premultiply_all_pairs():
    px = np.stack([C, C, C, A], axis=-1)
    pil = np.asarray(Image.fromarray(px).convert("RGBa"))
    assert np.array_equal(pil[..., 0], R.premultiply(C, A)) and np.array_equal(pil[..., 3], A)


def test_unpremultiply_all_pairs():
    px = np.stack([C, C, C, A], axis=-1)                                   # p > a included: what filter overshoot leaves
    pil = np.asarray(Image.frombytes("RGBa", (256, 256), px.tobytes()).convert("RGBA"))
    assert np.array_equal(pil[..., 0], R.unpremultiply(C, A)) and np.array_equal(pil[..., 3], A)
    assert int(((C > A) & (A > 0)).sum()) > 30000
    assert not np.array_equal(pil[..., 0], R.unpremultiply(C, A, mutant="round_unpremultiply"))


@pytest.mark.parametrize("name", sorted(R.cases()))
def test_crop_resize_matches_pillow(name):
    img, box, size = R.cases()[name]
    assert np.array_equal(R.crop_resize(img, box, size), pil_crop_resize(img, box, size))


def test_cases_cover_every_branch_of_the_conversions():
    """Counted on Pillow's output: transparent, opaque, partial alpha, and partial alpha whose un-premultiplied value is clamped (the resampled
    premultiplied colour above the resampled alpha)."""
    tot = np.zeros(4, dtype=np.int64)
    for img, box, size in R.cases().values():
        im = Image.fromarray(img)
        im = im.crop(box) if box is not None else im
        if im.size == size:
            continue
        a = np.asarray(im.resize(size, LANCZOS))[..., 3]
        pre = np.asarray(im.convert("RGBa").resize(size, LANCZOS))
        part = (a > 0) & (a < 255)
        tot += [(a == 0).sum(), (a == 255).sum(), part.sum(), (part & (pre[..., :3] > pre[..., 3:]).any(-1)).sum()]
    print("pixels with a == 0, a == 255, 0 < a < 255, clamped:", tot.tolist())
    assert (tot >= 100).all()


def test_composites_all_pairs():
    t = R.pair_table()
    c, a = t[..., :3], t[..., 3:]
    assert np.array_equal(R.composite_black(c, a), literal_black(t))
    white, mask = literal_white(t)
    assert np.array_equal(R.composite_white(c, a), white)
    assert np.array_equal(R.composite_mask(t[..., 3]), mask) and np.array_equal(mask, t[..., 3])
    assert np.array_equal(R.composite_float(c, a), literal_float(t))
    assert R.composite_float(c, a).dtype == np.float32
    for m in ("white_fma", "white_integer_floor"):
        d = R.composite_white(c, a, mutant=m).astype(int) - white
        print(f"{m}: {int((d[..., 0] != 0).sum())} of 65536 pairs differ")
        assert (d != 0).any() and np.abs(d).max() == 1


def test_crop_box_even_and_odd_extents():
    # even extents: integer centre; odd extents: half-integer centre, Image.crop rounds half to even
    assert R.crop_box((10, 20, 30, 50)) == ((2.0, 17.0, 38.0, 53.0), (2, 17, 38, 53))
    box, ints = R.crop_box((10, 20, 31, 45))                               # centre (20.5, 32.5), size int(25 * 1.2) = 30
    assert box == (5.5, 17.5, 35.5, 47.5) and ints == (6, 18, 36, 48)
    box, ints = R.crop_box((0, 0, 5, 2))                                   # centre (2.5, 1.0), size 6
    assert box == (-0.5, -2.0, 5.5, 4.0) and ints == (0, -2, 6, 4)
    from gvfdiffusion_amd.utils import rgba_ops
    for bb in ((10, 20, 30, 50), (10, 20, 31, 45), (0, 0, 5, 2), (3, 3, 3, 3), (7, 1, 100, 64)):
        assert rgba_ops.crop_box(bb) == R.crop_box(bb)
        xmin, ymin, xmax, ymax = (np.int64(v) for v in bb)                  # the reference's lines on numpy integers
        center = (xmin + xmax) / 2, (ymin + ymax) / 2
        size = int(max(xmax - xmin, ymax - ymin) * 1.2)
        lit = center[0] - size // 2, center[1] - size // 2, center[0] + size // 2, center[1] + size // 2
        assert tuple(float(v) for v in lit) == R.crop_box(bb)[0]
        assert tuple(map(int, map(round, lit))) == R.crop_box(bb)[1]
    with pytest.raises(ValueError):
        rgba_ops.crop_box((64, 48, -1, -1))


def test_alpha_bbox_is_argwhere():
    img = R.soft_disc(48, 64, 11)
    bbox = np.argwhere(img[..., 3] > 0.8 * 255)
    want = np.min(bbox[:, 1]), np.min(bbox[:, 0]), np.max(bbox[:, 1]), np.max(bbox[:, 0])
    assert R.alpha_bbox(img)[:4] == tuple(int(v) for v in want)
    assert R.alpha_bbox(np.zeros((5, 7, 4), dtype=np.uint8)) == (7, 5, -1, -1, 0)


@pytest.mark.parametrize("mutant", ["round_unpremultiply", "straight_alpha", "premultiply_same_size"])
def test_resize_comparison_rejects_mutants(mutant):
    bad = [n for n, (img, box, size) in R.cases().items() if not np.array_equal(R.crop_resize(img, box, size, mutant=mutant), pil_crop_resize(img, box, size))]
    print(f"{mutant}: differs from Pillow in {bad}")
    assert bad
    if mutant == "premultiply_same_size":
        assert bad == ["copy"]


def test_routes_match_pillow_and_the_literal_lines():
    """A, B and C end to end on one small image: Pillow for crop + resize, the scripts' numpy lines for the rest."""
    frames = np.stack([R.soft_disc(48, 64, s) for s in (21, 22)])
    a_img, a_box = R.preprocess_image(frames[0], size=37)
    assert np.array_equal(a_img, literal_black(pil_crop_resize(frames[0], a_box, (37, 37))))
    b_frames, b_mask, b_box = R.preprocess_video_frames(frames, size=30, canvas=40)
    assert b_box == a_box
    for t in range(2):
        white, mask = literal_white(pil_crop_resize(frames[t], b_box, (30, 30)))
        canvas = np.full((40, 40, 3), 255, dtype=np.uint8)
        canvas[5:35, 5:35] = white
        assert np.array_equal(b_frames[t], canvas)
        if t == 0:
            m = np.zeros((40, 40), dtype=np.uint8)
            m[5:35, 5:35] = mask
            assert np.array_equal(b_mask, m)
    c = R.dataset_pixels(frames, size=37)
    for t in range(2):
        assert np.array_equal(c[t], literal_float(pil_crop_resize(frames[t], None, (37, 37))).transpose(2, 0, 1))


def test_pinned_to_the_reference_functions():
    """tests/golden/rgba_golden.npz: one soft-edged RGBA image, the boxes and the SHA-256 of what the reference's own preprocess_image and
    remove_background returned for it (recorded by tests/golden/make_rgba_golden.py)."""
    g = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "rgba_golden.npz"))
    img = g["input"]
    sha = lambda a: hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()
    a_img, a_box = R.preprocess_image(img)
    assert a_img.shape == tuple(g["a_shape"]) and sha(a_img) == str(g["a_sha256"])
    b_frames, b_mask, b_box = R.preprocess_video_frames(img[None])
    assert tuple(float(v) for v in b_box) == tuple(g["b_box"].tolist()) == tuple(float(v) for v in a_box)
    assert sha(b_frames[0]) == str(g["b_image_sha256"]) and sha(b_mask) == str(g["b_mask_sha256"])
