"""Times the RGBA condition preprocessing on the device (csrc/rgba.hip, utils/rgba_ops.py) at the two sizes the reference's scripts run it:
  B  the in-the-wild route, 32 frames of 1024 x 1024 RGBA -> 380 x 380 on a white 512 x 512 canvas + mask (preprocess_video_frames)
  C  the dataset route, 24 renders of 512 x 512 RGBA -> fp32 (3, 518, 518), rgb * alpha
next to (a) the reference's route, Pillow + numpy per frame on one host core, and (b) what the package could compose on the device
without the fused launches: torch integer element-wise ops for the conversions and composites around resize_pad_crop_u8 on
de-interleaved planes -- checked for bit equality first.  Device times are HIP events around `iters` calls, the median, smallest and
largest of `windows` such windows after a warm-up; profiles/rgba_preprocess.txt is this script's output."""
import os
import sys
import time

import numpy as np
import torch
from PIL import Image

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from gvfdiffusion_amd.utils import alpha_bbox, crop_box, preprocess_video_frames, resize_pad_crop_u8, rgba_crop_resize  # noqa: E402

LANCZOS = Image.Resampling.LANCZOS


def frames_rgba(T, S, seed):
    """Random colours under a soft-edged alpha disc that drifts from frame to frame."""
    g = torch.Generator().manual_seed(seed)
    rgb = torch.randint(0, 256, (T, S, S, 3), generator=g, dtype=torch.uint8)
    y, x = torch.meshgrid(torch.arange(S, dtype=torch.float32), torch.arange(S, dtype=torch.float32), indexing="ij")
    a = []
    for t in range(T):
        d = torch.hypot((x - S / 2 - 2 * t) / (0.36 * S), (y - S / 2 + t) / (0.30 * S))
        a.append(((1.0 - d) / 0.25 * 255).clamp(0, 255).to(torch.uint8))
    return torch.cat([rgb, torch.stack(a)[..., None]], dim=-1).contiguous()


def device_ms(fn, iters=20, windows=7, warmup=3):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(windows):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(iters):
            fn()
        e1.record()
        torch.cuda.synchronize()
        out.append(e0.elapsed_time(e1) / iters)
    out.sort()
    return out[len(out) // 2], out[0], out[-1]


def host_ms(fn, repeats=3):
    out = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        fn()
        out.append((time.perf_counter() - t0) * 1e3)
    out.sort()
    return out[len(out) // 2], out[0], out[-1]


# ---- (a) the reference's route on the host ----

def host_wild(frames, box):
    out = []
    for f in frames:
        im = Image.fromarray(f).crop(box).resize((380, 380), LANCZOS)
        o = np.array(im).astype(np.float32) / 255
        o = o[:, :, :3] * o[:, :, 3:4] + (1 - o[:, :, 3:4]) * 1.0
        canvas = np.ones((512, 512, 3))
        canvas[66:446, 66:446, :3] = o
        out.append((canvas * 255).astype(np.uint8))
    return np.stack(out)


def host_dataset(frames):
    out = []
    for f in frames:
        o = np.array(Image.fromarray(f).resize((518, 518), LANCZOS)).astype(np.float32) / 255
        out.append((o[:, :, :3] * o[:, :, 3:]).transpose(2, 0, 1))
    return np.stack(out)


# ---- (b) composed on the device from torch element-wise ops and the plane resampler ----

def composed_resize(rgba, ints, size):
    """crop + premultiply + four plane resizes + un-premultiply -> int32 colour (T, 3, s, s), alpha (T, 1, s, s)."""
    T, H, W, _ = rgba.shape
    x0, y0, x1, y1 = ints
    win = torch.zeros((T, y1 - y0, x1 - x0, 4), dtype=torch.uint8, device=rgba.device)
    sx0, sy0, sx1, sy1 = max(x0, 0), max(y0, 0), min(x1, W), min(y1, H)
    win[:, sy0 - y0:sy1 - y0, sx0 - x0:sx1 - x0] = rgba[:, sy0:sy1, sx0:sx1]
    planes = win.permute(0, 3, 1, 2).to(torch.int32)
    a = planes[:, 3:]
    t = planes[:, :3] * a + 128
    pre = torch.cat([((t >> 8) + t) >> 8, a], dim=1).to(torch.uint8).contiguous()
    r = resize_pad_crop_u8(pre, size, out_size=size).to(torch.int32)
    p, a = r[:, :3], r[:, 3:]
    q = torch.clamp(torch.div(255 * p, torch.clamp(a, min=1), rounding_mode="floor"), max=255)
    return torch.where((a == 0) | (a == 255), p, q), a


def _f255(dev):
    # a divisor tensor on the device: torch turns the division by a Python scalar into a multiplication by its reciprocal there
    return torch.full((1,), 255.0, dtype=torch.float32, device=dev)


def composed_wild(rgba, ints):
    c, a = composed_resize(rgba, ints, 380)
    fa = a.float() / _f255(rgba.device)
    w = (c.float() / _f255(rgba.device)) * fa + (1 - fa) * 1.0
    out = torch.full((rgba.shape[0], 512, 512, 3), 255, dtype=torch.uint8, device=rgba.device)
    out[:, 66:446, 66:446] = (w.double() * 255.0).to(torch.uint8).permute(0, 2, 3, 1)
    mask = torch.zeros((512, 512), dtype=torch.uint8, device=rgba.device)
    mask[66:446, 66:446] = (fa[0, 0].double() * 255.0).to(torch.uint8)
    return out, mask


def composed_dataset(rgba):
    T, H, W, _ = rgba.shape
    c, a = composed_resize(rgba, (0, 0, W, H), 518)
    return (c.float() / _f255(rgba.device)) * (a.float() / _f255(rgba.device))


def report(name, fused, host, composed, equal_host, equal_composed, frames, algorithmic, moved):
    (f, f0, f1), (h, h0, h1), (c, c0, c1) = fused, host, composed
    print(f"{name}")
    print(f"  fused launches     {f:8.3f} ms per call (min {f0:.3f}, max {f1:.3f}), {f / frames * 1e3:.1f} us / frame; "
          f"bit-equal to the host route: {equal_host}")
    print(f"  (a) Pillow + numpy {h:8.1f} ms per call (min {h0:.1f}, max {h1:.1f}) on one host core: {h / f:.0f} x the fused launches")
    print(f"  (b) torch composed {c:8.3f} ms per call (min {c0:.3f}, max {c1:.3f}); bit-equal to the fused result: {equal_composed}: "
          f"{c / f:.2f} x the fused launches")
    print(f"  bytes: algorithmic {algorithmic / 1e6:.1f} MB (window read once, result written once), moved {moved / 1e6:.1f} MB "
          f"(+ the RGBa intermediate written and read, the mask planes) = {moved / algorithmic:.2f} x; "
          f"{algorithmic / f / 1e6:.0f} GB/s algorithmic, {moved / f / 1e6:.0f} GB/s moved")


def main():
    if not torch.cuda.is_available():
        raise SystemExit("bench_rgba_preprocess.py needs an MI355X")
    dev = torch.device("cuda")
    print(f"device: {torch.cuda.get_device_name(0)}")

    # B: 32 x 1024 x 1024
    T, S = 32, 1024
    host = frames_rgba(T, S, 1)
    x = host.to(dev)
    frames, mask, box = preprocess_video_frames(x)
    ints = crop_box(alpha_bbox(x[:1]).cpu().tolist()[0][:4])[1]
    hnp = host.numpy()
    want = host_wild(hnp, box)
    eq_h = bool(np.array_equal(frames.cpu().numpy(), want))
    cw, cm = composed_wild(x, ints)
    eq_c = bool(torch.equal(cw, frames) and torch.equal(cm, mask))
    c, a = composed_resize(x, ints, 380)
    eq_i = bool(torch.equal(torch.cat([c, a], 1).permute(0, 2, 3, 1).to(torch.uint8), rgba_crop_resize(x, box, 380)))
    print(f"(b) before the composite: the composed crop + conversions + plane resizes are bit-equal to the fused RGBA result: {eq_i}")
    side = ints[2] - ints[0]
    inside = (min(ints[2], S) - max(ints[0], 0)) * (min(ints[3], S) - max(ints[1], 0))
    alg = S * S * 4 + T * (inside * 4 + 512 * 512 * 3) + 512 * 512
    moved = alg + T * (2 * side * 380 * 4 + 512 * 512) - 512 * 512
    print(f"box {box} -> crop {side} x {side}")
    report(f"B  in-the-wild route: {T} x {S} x {S} RGBA -> 380 x 380 on white in 512 x 512 + mask (one bounding-box read-back included)",
           device_ms(lambda: preprocess_video_frames(x)), host_ms(lambda: host_wild(hnp, box)),
           device_ms(lambda: composed_wild(x, ints)), eq_h, eq_c, T, alg, moved)

    # C: 24 x 512 x 512 -> 518
    T, S = 24, 512
    host = frames_rgba(T, S, 2)
    x = host.to(dev)
    hnp = host.numpy()
    got = rgba_crop_resize(x, None, 518, mode="float")
    eq_h = bool(np.array_equal(got.cpu().numpy(), host_dataset(hnp)))
    eq_c = bool(torch.equal(composed_dataset(x), got))
    alg = T * (S * S * 4 + 518 * 518 * 12)
    moved = alg + T * 2 * S * 518 * 4
    report(f"C  dataset route: {T} x {S} x {S} RGBA -> fp32 (3, 518, 518), rgb * alpha",
           device_ms(lambda: rgba_crop_resize(x, None, 518, mode="float")), host_ms(lambda: host_dataset(hnp)),
           device_ms(lambda: composed_dataset(x)), eq_h, eq_c, T, alg, moved)


if __name__ == "__main__":
    main()
