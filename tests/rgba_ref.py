"""numpy restatement of the RGBA condition preprocessing (include/gvf_image.h, utils/rgba_ops.py): Pillow's crop + premultiplied-alpha
LANCZOS resize of an RGBA image, the reference's composites and box arithmetic, and its three routes end to end.  Held to Pillow and to the
literal numpy expressions in tests/test_rgba_ref.py; the GPU tests hold the kernels to it.  `mutant` switches in one wrong decision each."""
import numpy as np

from gvfdiffusion_amd.utils.image_ops import resample_table

PRECISION_BITS = 22
MUTANTS = ("round_unpremultiply", "straight_alpha", "premultiply_same_size", "white_fma", "white_integer_floor")


def premultiply(c, a):
    """RGBA -> RGBa of colour values c under alpha a (uint8 arrays)."""
    t = c.astype(np.int64) * a.astype(np.int64) + 128
    return (((t >> 8) + t) >> 8).astype(np.uint8)


def unpremultiply(p, a, mutant=None):
    """RGBa -> RGBA: copy at alpha 0 and 255, else min(255, 255 * p // a)."""
    p64, a64 = p.astype(np.int64), a.astype(np.int64)
    safe = np.maximum(a64, 1)
    q = (255 * p64 + safe // 2) // safe if mutant == "round_unpremultiply" else (255 * p64) // safe
    return np.where((a64 == 0) | (a64 == 255), p64, np.minimum(255, q)).astype(np.uint8)


def crop(img, ints):
    """Image.crop with an integer box on (H, W, C): zeros outside the image."""
    x0, y0, x1, y1 = ints
    H, W = img.shape[:2]
    out = np.zeros((y1 - y0, x1 - x0) + img.shape[2:], dtype=img.dtype)
    sx0, sy0, sx1, sy1 = max(x0, 0), max(y0, 0), min(x1, W), min(y1, H)
    if sx1 > sx0 and sy1 > sy0:
        out[sy0 - y0:sy1 - y0, sx0 - x0:sx1 - x0] = img[sy0:sy1, sx0:sx1]
    return out


def resample_axis(img, n_out, axis):
    """One 8-bit pass along `axis` (0 = vertical, 1 = horizontal) of (H, W, C) uint8."""
    first, count, coef, _ = resample_table(img.shape[axis], n_out)
    coef = np.asarray(coef, dtype=np.int64)
    src = np.moveaxis(img.astype(np.int64), axis, 0)
    out = np.empty((n_out,) + src.shape[1:], dtype=np.uint8)
    for i in range(n_out):
        k = coef[:count[i], i].reshape((-1,) + (1,) * (src.ndim - 1))
        acc = (1 << (PRECISION_BITS - 1)) + (src[first[i]:first[i] + count[i]] * k).sum(0)
        out[i] = np.clip(acc >> PRECISION_BITS, 0, 255)
    return np.moveaxis(out, 0, axis)


def resize_rgba(img, size, mutant=None):
    """Image.resize((w, h), LANCZOS) of an RGBA (H, W, 4) uint8 image."""
    w, h = (size, size) if np.isscalar(size) else size
    H, W = img.shape[:2]
    if (W, H) == (w, h) and mutant != "premultiply_same_size":
        return img.copy()
    if mutant == "straight_alpha":
        x = img
    else:
        x = np.concatenate([premultiply(img[..., :3], img[..., 3:]), img[..., 3:]], axis=-1)
    if W != w:
        x = resample_axis(x, w, 1)
    if H != h:
        x = resample_axis(x, h, 0)
    if mutant == "straight_alpha":
        return x
    return np.concatenate([unpremultiply(x[..., :3], x[..., 3:], mutant), x[..., 3:]], axis=-1)


def round_box(box):
    return tuple(int(round(float(v))) for v in box)


def crop_resize(img, box, size, mutant=None):
    """img.crop(box).resize(size, LANCZOS); box None = the whole image."""
    if box is not None:
        img = crop(img, round_box(box))
    return resize_rgba(img, size, mutant)


def composite_black(c, a):
    """(rgb / 255 * alpha / 255 * 255).astype(uint8) in fp32; equals c * a // 255."""
    return (c.astype(np.int64) * a.astype(np.int64) // 255).astype(np.uint8)


def composite_white(c, a, mutant=None):
    """uint8 of a float64 canvas holding the fp32 rgb * alpha + (1 - alpha) * 1.0, times 255."""
    if mutant == "white_integer_floor":
        return ((c.astype(np.int64) * a + 255 * (255 - a.astype(np.int64))) // 255).astype(np.uint8)
    fc, fa = c.astype(np.float32) / np.float32(255), a.astype(np.float32) / np.float32(255)
    rest = (np.float32(1) - fa) * np.float32(1)
    if mutant == "white_fma":
        w = (fc.astype(np.float64) * fa.astype(np.float64) + rest.astype(np.float64)).astype(np.float32)    # one rounding: exact product + add
    else:
        w = fc * fa + rest
    return (w.astype(np.float64) * 255.0).astype(np.uint8)


def composite_mask(a):
    return ((a.astype(np.float32) / np.float32(255)).astype(np.float64) * 255.0).astype(np.uint8)


def composite_float(c, a):
    return (c.astype(np.float32) / np.float32(255)) * (a.astype(np.float32) / np.float32(255))


def alpha_bbox(img, threshold=204):
    """(xmin, ymin, xmax, ymax, min alpha); (W, H, -1, -1) when no pixel is above the threshold."""
    a = img[..., 3]
    ys, xs = np.nonzero(a > threshold)
    if len(xs) == 0:
        return a.shape[1], a.shape[0], -1, -1, int(a.min())
    return int(xs.min()), int(ys.min()), int(xs.max()), int(ys.max()), int(a.min())


def crop_box(bbox, margin=1.2):
    xmin, ymin, xmax, ymax = (int(v) for v in bbox)
    cx, cy = (xmin + xmax) / 2, (ymin + ymax) / 2
    size = int(max(xmax - xmin, ymax - ymin) * margin)
    box = (cx - size // 2, cy - size // 2, cx + size // 2, cy + size // 2)
    return box, round_box(box)


def preprocess_image(img, size=518, mutant=None):
    """Route A: (H, W, 4) -> (size, size, 3) uint8 on black, and the float box."""
    box, _ = crop_box(alpha_bbox(img)[:4])
    r = crop_resize(img, box, size, mutant)
    return composite_black(r[..., :3], r[..., 3:]), box


def place(img, canvas, offset, pad):
    out = np.full((canvas, canvas) + img.shape[2:], pad, dtype=img.dtype)
    out[offset:offset + img.shape[0], offset:offset + img.shape[1]] = img
    return out


def preprocess_video_frames(frames, size=380, canvas=512, mutant=None):
    """Route B: (T, H, W, 4) -> frames (T, canvas, canvas, 3) on white, frame 0's mask (canvas, canvas), the float box."""
    box, _ = crop_box(alpha_bbox(frames[0])[:4])
    off = (canvas - size) // 2
    out, mask = [], None
    for t, f in enumerate(frames):
        r = crop_resize(f, box, size, mutant)
        out.append(place(composite_white(r[..., :3], r[..., 3:], mutant), canvas, off, 255))
        if t == 0:
            mask = place(composite_mask(r[..., 3]), canvas, off, 0)
    return np.stack(out), mask, box


def dataset_pixels(frames, size=518, mutant=None):
    """Route C: (T, H, W, 4) -> fp32 (T, 3, size, size), rgb * alpha of the resized render."""
    out = []
    for f in frames:
        r = resize_rgba(f, size, mutant)
        out.append(composite_float(r[..., :3], r[..., 3:]).transpose(2, 0, 1))
    return np.stack(out)


# ---- the images and cases the CPU and GPU tests share ----

def soft_disc(H, W, seed):
    """Random colours under a soft-edged alpha disc: every alpha from 0 to 255 along the rim."""
    g = np.random.default_rng(seed)
    img = g.integers(0, 256, size=(H, W, 4), dtype=np.uint8)
    y, x = np.mgrid[0:H, 0:W]
    d = np.hypot((x - W / 2 + 0.5) / (W / 2), (y - H / 2 + 0.5) / (H / 2))
    img[..., 3] = np.clip((0.85 - d) / 0.35 * 255, 0, 255).astype(np.uint8)
    return img


def hard_edges(H, W, seed, cell=5):
    """Alpha 0 / 255 in cells, saturated colour (0 / 255 per channel) in smaller cells: the filter overshoots on both, differently, so the
    resampled premultiplied colour exceeds the resampled alpha in the ringing next to the edges."""
    g = np.random.default_rng(seed)
    img = np.empty((H, W, 4), dtype=np.uint8)
    col = g.integers(0, 2, size=((H + 2) // 3, (W + 2) // 3, 3), dtype=np.uint8) * 255
    img[..., :3] = np.kron(col, np.ones((3, 3, 1), dtype=np.uint8))[:H, :W]
    a = g.integers(0, 2, size=((H + cell - 1) // cell, (W + cell - 1) // cell), dtype=np.uint8) * 255
    img[..., 3] = np.kron(a, np.ones((cell, cell), dtype=np.uint8))[:H, :W]
    return img


def pair_table():
    """256 x 256 x 4: pixel (a, c) = colour (c, 255 - c, (c * 7) % 256) under alpha a -- every (value, alpha) pair in the R channel."""
    a, c = np.mgrid[0:256, 0:256].astype(np.uint8)
    return np.stack([c, 255 - c, (c.astype(np.int64) * 7 % 256).astype(np.uint8), a], axis=-1).astype(np.uint8)


TABLE_BLOCK = 8


def conversion_table_image():
    """Constant TABLE_BLOCK x TABLE_BLOCK blocks, one per (alpha, three values): block row a, block column j holds colour
    (3j, 3j + 1, 3j + 2) (capped at 255) under alpha a."""
    a, j = np.mgrid[0:256, 0:86]
    px = np.stack([np.minimum(3 * j, 255), np.minimum(3 * j + 1, 255), np.minimum(3 * j + 2, 255), a], axis=-1).astype(np.uint8)
    return np.kron(px, np.ones((TABLE_BLOCK, TABLE_BLOCK, 1), dtype=np.uint8))


def unfiltered_outputs(n_in, n_out, block=TABLE_BLOCK):
    """Per output sample of one axis: the block index if all its taps (first / count of resample_table) lie inside one block, else -1."""
    first, count, _, _ = resample_table(n_in, n_out)
    first, count = np.asarray(first), np.asarray(count)
    lo, hi = first // block, (first + count - 1) // block
    return np.where(lo == hi, lo, -1)


# name -> (image, box or None, (width, height)): crop side -> output of the conformance list
def cases():
    return {
        "down_31_taps": (soft_disc(110, 120, 1), (10.0, 6.0, 107.0, 103.0), (20, 20)),                 # 97 -> 20, box inside
        "up_box_outside": (hard_edges(18, 20, 2), (-2.0, -3.0, 22.0, 21.0), (77, 77)),                 # 24 -> 77, box out on all four sides
        "up_soft": (soft_disc(24, 24, 3), None, (77, 77)),
        "rect_half_even": (soft_disc(60, 60, 4), (3.4, 5.5, 56.4, 53.0), (20, 20)),                    # 53 x 47 -> 20 x 20 (5.5 rounds to 6)
        "one_axis": (hard_edges(45, 50, 5), (5.0, 7.0, 45.0, 38.0), (40, 50)),                         # 40 x 31 -> 40 x 50
        "one_axis_h": (hard_edges(45, 50, 6), (5.0, 7.0, 45.0, 38.0), (57, 31)),                       # 40 x 31 -> 57 x 31
        "copy": (np.random.default_rng(7).integers(0, 256, size=(30, 30, 4), dtype=np.uint8), (4.0, 6.0, 24.0, 26.0), (20, 20)),
        "hard_down": (hard_edges(97, 97, 8, cell=11), None, (40, 40)),
    }
