"""RGBA condition preprocessing on the device, bit-identical to the Pillow + numpy host loops it replaces (csrc/rgba.hip):

  A  trellis/pipelines/trellis_image_to_3d.py:85-119   preprocess_image (the branch for an image that carries alpha)
  B  scripts/encode_in_the_wild_img_cond_dinov2_feature.py:27-66, 86-110   remove_background + the later frames of a sequence
  C  scripts/encode_img_cond_dinov2_feature.py:40-44   RGBA render -> 518 x 518 -> rgb * alpha in fp32

`Image.crop(box).resize(size, LANCZOS)` on an RGBA image premultiplies, resamples all four bands and un-premultiplies, each step with
its own integer rounding (include/gvf_image.h); the composites are the scripts' fp32 / fp64 expressions.  Not built: rembg (the
background removal of an image without alpha needs a downloaded network)."""
import ctypes

import torch

from .. import _lib
from .image_ops import _Table, _device_table

__all__ = ["alpha_bbox", "crop_box", "rgba_crop_resize", "preprocess_image", "preprocess_video_frames", "RGBA_MODES"]

_i, _vp, _i64 = ctypes.c_int, ctypes.c_void_p, ctypes.c_int64
_tab = ctypes.POINTER(_Table)

_lib.register({
    "gvf_alpha_bbox_u8": (_i, [_vp, _i64, _i, _i, _i, _vp, _vp]),
    "gvf_rgba_resample_u8": (_i, [_vp, _i64, _i, _i, _i, _i, _i, _i, _tab, _tab, _vp, _i, _vp, _vp, _i, _i, _i, _i, _i, _vp]),
})

# mode -> (GVF_RGBA_OUT_*, pad value of uncovered canvas pixels)
RGBA_MODES = {"rgba": (0, 0), "black": (1, 0), "white": (2, 255), "float": (3, 0)}
_MAX_BATCH = 65535
_MAX_EXTENT = 16384          # GVF_RESAMPLE_MAX_WIDTH


def _check_rgba(rgba, what="rgba"):
    if not isinstance(rgba, torch.Tensor) or rgba.dtype != torch.uint8 or rgba.dim() != 4 or rgba.shape[-1] != 4:
        raise ValueError(f"{what} must be a uint8 tensor (B, H, W, 4), got "
                         f"{getattr(rgba, 'dtype', type(rgba))} {tuple(getattr(rgba, 'shape', ()))}")
    _lib.require_cuda(rgba)
    if rgba.shape[1] < 1 or rgba.shape[2] < 1:
        raise ValueError(f"{what} has an empty image axis: {tuple(rgba.shape)}")
    return rgba.contiguous()


def _pair(v, what):
    if isinstance(v, (tuple, list)):
        if len(v) != 2:
            raise ValueError(f"{what} must be an int or a (width, height) pair")
        return int(v[0]), int(v[1])
    return int(v), int(v)


def alpha_bbox(rgba: torch.Tensor, threshold: int = 204) -> torch.Tensor:
    """rgba uint8 (B, H, W, 4) on the device -> int32 (B, 5) on the device: xmin, ymin, xmax, ymax of `alpha > threshold`
    (np.argwhere(alpha > 0.8 * 255) min / max; (W, H, -1, -1) when no pixel passes) and the smallest alpha of the image.  No read-back."""
    rgba = _check_rgba(rgba)
    threshold = int(threshold)
    if not 0 <= threshold <= 255:
        raise ValueError("threshold must be in 0..255")
    B, H, W, _ = rgba.shape
    out = torch.empty((B, 5), dtype=torch.int32, device=rgba.device)
    for b0 in range(0, B, _MAX_BATCH):
        n = min(_MAX_BATCH, B - b0)
        _lib.check(_lib.lib().gvf_alpha_bbox_u8(_lib.ptr(rgba[b0:]), n, H, W, threshold, _lib.ptr(out[b0:]), _lib.current_stream(rgba.device)),
                   "gvf_alpha_bbox_u8")
    return out


def crop_box(bbox, margin: float = 1.2):
    """bbox = (xmin, ymin, xmax, ymax) integers -> (the float box, its rounded ints): the reference's expression on the host,
        center = (xmin + xmax) / 2, (ymin + ymax) / 2;  size = int(max(xmax - xmin, ymax - ymin) * 1.2)
        box = center[0] - size // 2, center[1] - size // 2, center[0] + size // 2, center[1] + size // 2
    and Image.crop's int(round(v)) (round half to even) of each."""
    xmin, ymin, xmax, ymax = (int(v) for v in bbox)
    if xmax < xmin or ymax < ymin:
        raise ValueError("no pixel above the alpha threshold: the bounding box is empty")
    center = (xmin + xmax) / 2, (ymin + ymax) / 2
    size = int(max(xmax - xmin, ymax - ymin) * margin)
    box = center[0] - size // 2, center[1] - size // 2, center[0] + size // 2, center[1] + size // 2
    return box, tuple(int(round(v)) for v in box)


def rgba_crop_resize(rgba: torch.Tensor, box, size, mode: str = "rgba", canvas=None, offset=None, pad=None, out=None):
    """`img.crop(box).resize(size, LANCZOS)` of every image of rgba uint8 (B, H, W, 4), one box for the batch, then one composite.
    box: (x0, y0, x1, y1), floats rounded as Image.crop does, may stick out of the image (zeros there); None = the whole image.
    size: int or (width, height).  mode:
        "rgba"   uint8 (B, h, w, 4)  the resized image
        "black"  uint8 (B, h, w, 3)  (rgb * alpha * 255).astype(uint8)                      (preprocess_image)
        "white"  uint8 (B, h, w, 3)  ((rgb * alpha + (1 - alpha) * 1.0) * 255).astype(uint8) from a float64 canvas, and the
                 mask uint8 (B, h, w); returns (rgb, mask)                                  (remove_background)
        "float"  fp32 (B, 3, h, w)   rgb * alpha, not rounded                               (the dataset script)
    canvas: int or (width, height) of the output, default = size; offset = (x, y) of the resized image in it, default (0, 0);
    uncovered pixels take `pad` (default 255 for "white", else 0; the mask takes 0).  out: the tensor(s) to write into."""
    rgba = _check_rgba(rgba)
    if mode not in RGBA_MODES:
        raise ValueError(f"mode must be one of {sorted(RGBA_MODES)}, got {mode!r}")
    code, default_pad = RGBA_MODES[mode]
    pad = default_pad if pad is None else int(pad)
    B, H, W, _ = rgba.shape
    ow, oh = _pair(size, "size")
    x0, y0, x1, y1 = (0, 0, W, H) if box is None else (int(round(v)) for v in box)
    cw, ch = x1 - x0, y1 - y0
    if cw < 1 or ch < 1 or ow < 1 or oh < 1:
        raise ValueError(f"empty crop box or size: box {(x0, y0, x1, y1)}, size {(ow, oh)}")
    dw, dh = (ow, oh) if canvas is None else _pair(canvas, "canvas")
    offx, offy = (0, 0) if offset is None else _pair(offset, "offset")
    if max(cw, ch, ow, oh, dw, dh, H, W) > _MAX_EXTENT:
        raise ValueError(f"an extent beyond GVF_RESAMPLE_MAX_WIDTH = {_MAX_EXTENT}: image {(W, H)}, crop {(cw, ch)}, size {(ow, oh)}, canvas {(dw, dh)}")
    dev = rgba.device
    shape = (B, dh, dw, 4) if mode == "rgba" else (B, 3, dh, dw) if mode == "float" else (B, dh, dw, 3)
    dtype = torch.float32 if mode == "float" else torch.uint8
    mask = None
    if out is not None:
        dst, mask = out if mode == "white" else (out, None)
        for t, s, d in ((dst, shape, dtype),) + (((mask, (B, dh, dw), torch.uint8),) if mode == "white" else ()):
            if t.shape != s or t.dtype != d or not t.is_contiguous() or t.device != dev:
                raise ValueError("out has the wrong shape / dtype / device")
    else:
        dst = torch.empty(shape, dtype=dtype, device=dev)
        if mode == "white":
            mask = torch.empty((B, dh, dw), dtype=torch.uint8, device=dev)
    di = dev.index if dev.index is not None else torch.cuda.current_device()
    keep_h, tab_h = (None, None) if cw == ow else _device_table(cw, ow, "lanczos", di)          # Image.resize copies at equal size
    keep_v, tab_v = (None, None) if ch == oh else _device_table(ch, oh, "lanczos", di)
    step = min(B, _MAX_BATCH)
    tmp = torch.empty((step, ch, ow, 4), dtype=torch.uint8, device=dev) if (tab_h is not None or tab_v is not None) else None
    for b0 in range(0, B, _MAX_BATCH):
        n = min(_MAX_BATCH, B - b0)
        _lib.check(_lib.lib().gvf_rgba_resample_u8(_lib.ptr(rgba[b0:]), n, H, W, x0, y0, cw, ch, ctypes.byref(tab_h) if tab_h is not None else None,
                                                   ctypes.byref(tab_v) if tab_v is not None else None, _lib.ptr(tmp), code, _lib.ptr(dst[b0:]),
                                                   _lib.ptr(mask[b0:]) if mask is not None else None, dh, dw, offy, offx, pad,
                                                   _lib.current_stream(dev)), "gvf_rgba_resample_u8")
    return (dst, mask) if mode == "white" else dst


def _boxes(rgba, what):
    """The host's share: one read-back of (B, 5) integers, the refusals, the reference's box arithmetic."""
    rows = alpha_bbox(rgba).cpu().tolist()
    boxes = []
    for xmin, ymin, xmax, ymax, amin in rows:
        if amin == 255:
            raise NotImplementedError(f"{what}: the image is fully opaque; the reference removes its background with rembg (u2net), "
                                      "which is not built here -- pass an image that carries alpha")
        boxes.append(crop_box((xmin, ymin, xmax, ymax))[0])
    return boxes


def preprocess_image(rgba: torch.Tensor, size: int = 518) -> torch.Tensor:
    """TrellisImageTo3DPipeline.preprocess_image for images that carry alpha: uint8 (B, H, W, 4) (or one (H, W, 4)) on the device ->
    uint8 (B, size, size, 3): per image the alpha > 0.8 * 255 bounding box, the square crop x 1.2, the LANCZOS resize and rgb * alpha.
    One box per image, so one pair of launches per image; the boxes cost one read-back of B x 5 integers for the whole batch."""
    if isinstance(rgba, torch.Tensor) and rgba.dim() == 3:
        rgba = rgba[None]
    rgba = _check_rgba(rgba)
    out = torch.empty((rgba.shape[0], size, size, 3), dtype=torch.uint8, device=rgba.device)
    for i, box in enumerate(_boxes(rgba, "preprocess_image")):
        rgba_crop_resize(rgba[i:i + 1], box, size, mode="black", out=out[i:i + 1])
    return out


def preprocess_video_frames(rgba_frames: torch.Tensor, size: int = 380, canvas: int = 512):
    """The in-the-wild script's per-sequence loop: uint8 (T, H, W, 4) on the device -> (frames uint8 (T, canvas, canvas, 3), mask uint8
    (canvas, canvas), the float box).  Frame 0 fixes the box (remove_background); every frame is cropped with it, resized to size x size,
    composited on white and pasted at ((canvas - size) // 2,) * 2 of a white canvas; the mask is frame 0's alpha on a zero canvas.
    One read-back of frame 0's five integers per sequence; all frames go through one pair of launches."""
    rgba_frames = _check_rgba(rgba_frames, "rgba_frames")
    if rgba_frames.shape[0] < 1:
        raise ValueError("rgba_frames holds no frame")
    box = _boxes(rgba_frames[:1], "preprocess_video_frames")[0]
    off = (canvas - size) // 2
    frames, mask = rgba_crop_resize(rgba_frames, box, size, mode="white", canvas=canvas, offset=(off, off))
    return frames, mask[0], box
