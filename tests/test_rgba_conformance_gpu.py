"""RGBA condition preprocessing on the device (csrc/rgba.hip, utils/rgba_ops.py) against Pillow itself, the reference's literal numpy lines
and the numpy restatement (tests/rgba_ref.py, held to both in tests/test_rgba_ref.py).  Every comparison is exact."""
import functools

import numpy as np
import pytest
import torch
from PIL import Image

import rgba_ref as R
from test_rgba_ref import literal_black, literal_float, literal_white, pil_crop_resize

pytestmark = pytest.mark.gpu
LANCZOS = Image.Resampling.LANCZOS


def dev(a, cuda):
    return torch.from_numpy(np.ascontiguousarray(a)).to(cuda)


@pytest.mark.parametrize("name", sorted(R.cases()))
def test_crop_resize_matches_pillow(cuda, name):
    from gvfdiffusion_amd.utils import rgba_crop_resize
    img, box, size = R.cases()[name]
    want = pil_crop_resize(img, box, size)
    got = rgba_crop_resize(dev(img[None], cuda), box, size).cpu().numpy()
    assert got.shape == (1, size[1], size[0], 4)
    assert np.array_equal(got[0], want), int(np.abs(got[0].astype(int) - want).max())


def test_every_mode_on_an_odd_canvas_at_an_odd_offset(cuda):
    """97 -> 20 placed at (5, 5) of a 31 x 31 canvas (neither a multiple of 4), and once hanging out of the canvas at (-3, 17)."""
    from gvfdiffusion_amd.utils import rgba_crop_resize
    img, box, size = R.cases()["down_31_taps"]
    r = pil_crop_resize(img, box, size)
    white, mask = literal_white(r)
    x = dev(img[None], cuda)

    def canvas(a, pad, ox, oy):
        out = np.full((31, 31) + a.shape[2:], pad, dtype=a.dtype)
        ys, xs = slice(max(oy, 0), min(oy + 20, 31)), slice(max(ox, 0), min(ox + 20, 31))
        out[ys, xs] = a[ys.start - oy:ys.stop - oy, xs.start - ox:xs.stop - ox]
        return out
    for ox, oy in ((5, 5), (-3, 17)):
        kw = dict(canvas=31, offset=(ox, oy))
        assert np.array_equal(rgba_crop_resize(x, box, size, "rgba", pad=9, **kw)[0].cpu().numpy(), canvas(r, 9, ox, oy))
        assert np.array_equal(rgba_crop_resize(x, box, size, "black", **kw)[0].cpu().numpy(), canvas(literal_black(r), 0, ox, oy))
        w, m = rgba_crop_resize(x, box, size, "white", **kw)
        assert np.array_equal(w[0].cpu().numpy(), canvas(white, 255, ox, oy)) and np.array_equal(m[0].cpu().numpy(), canvas(mask, 0, ox, oy))
        f = rgba_crop_resize(x, box, size, "float", **kw)[0].cpu().numpy()
        assert f.dtype == np.float32 and np.array_equal(f, canvas(literal_float(r), 0, ox, oy).transpose(2, 0, 1))


def test_batch_of_three_shares_one_box(cuda):
    from gvfdiffusion_amd.utils import rgba_crop_resize
    imgs = np.stack([R.soft_disc(53, 61, 31), R.hard_edges(53, 61, 32), R.hard_edges(53, 61, 33, cell=7)])
    box = (-4.5, 3.5, 50.5, 58.5)
    got = rgba_crop_resize(dev(imgs, cuda), box, (33, 29)).cpu().numpy()
    for i in range(3):
        assert np.array_equal(got[i], pil_crop_resize(imgs[i], box, (33, 29)))


@pytest.mark.parametrize("H,W,size", [(5, 4100, (100, 7)), (3, 8200, (200, 3))])
def test_wide_rows_stage_fewer_rows_per_workgroup(cuda, H, W, size):
    """The horizontal pass stages 4 window rows per workgroup while they fit 16 384 pixels of LDS: 3 rows at 4100 wide (5 rows = two
    workgroups, the second one short), 1 row at 8200 wide.  247 taps per output, just inside GVF_RESAMPLE_MAX_TAPS."""
    from gvfdiffusion_amd._lib import GvfError
    from gvfdiffusion_amd.utils import rgba_crop_resize
    img = R.hard_edges(H, W, H + W, cell=37)
    img[..., 3] = np.maximum(img[..., 3], R.soft_disc(H, W, 1)[..., 3])
    got = rgba_crop_resize(dev(img[None], cuda), None, size)[0].cpu().numpy()
    assert np.array_equal(got, pil_crop_resize(img, None, size))
    with pytest.raises(GvfError):
        rgba_crop_resize(dev(img[None], cuda), None, (W // 100, size[1]))       # 601 taps: beyond GVF_RESAMPLE_MAX_TAPS, refused on the host


@functools.lru_cache(maxsize=None)
def _table_case():
    t = R.conversion_table_image()
    H, W = t.shape[:2]
    size = (W + 16, H + 48)
    return t, size, np.asarray(Image.fromarray(t).resize(size, LANCZOS))


def test_conversion_table_image(cuda):
    """Constant blocks, one per alpha and three values, slightly upscaled: the pixels whose taps stay inside one block in both axes go through
    premultiply and un-premultiply unfiltered, and together they cover all 65 536 (value, alpha) pairs -- asserted on the table geometry and on
    Pillow's output before the device is compared."""
    from gvfdiffusion_amd.utils import rgba_crop_resize
    t, size, want = _table_case()
    H, W = t.shape[:2]
    ux, uy = R.unfiltered_outputs(W, size[0]), R.unfiltered_outputs(H, size[1])
    seen = np.zeros((256, 256), dtype=bool)                                # [alpha][value]
    ys, xs = np.nonzero(uy >= 0)[0], np.nonzero(ux >= 0)[0]
    src = t[::R.TABLE_BLOCK, ::R.TABLE_BLOCK][uy[ys]][:, ux[xs]]            # the block behind each unfiltered output pixel
    for ch in range(3):
        seen[src[..., 3], src[..., ch]] = True
    assert seen.all()
    inner = want[ys][:, xs]
    expect = R.unpremultiply(R.premultiply(src[..., :3], src[..., 3:]), src[..., 3:])
    assert np.array_equal(inner[..., 3], src[..., 3]) and np.array_equal(inner[..., :3], expect)       # Pillow: conversions only, no filtering
    got = rgba_crop_resize(dev(t[None], cuda), None, size)[0].cpu().numpy()
    assert np.array_equal(got, want)


def test_composites_all_pairs_through_the_copy_path(cuda):
    from gvfdiffusion_amd.utils import rgba_crop_resize
    t = R.pair_table()
    x = dev(t[None], cuda)
    assert np.array_equal(rgba_crop_resize(x, None, 256, "rgba")[0].cpu().numpy(), t)                   # no premultiply round trip
    assert np.array_equal(rgba_crop_resize(x, None, 256, "black")[0].cpu().numpy(), literal_black(t))
    white, mask = literal_white(t)
    w, m = rgba_crop_resize(x, None, 256, "white")
    assert np.array_equal(w[0].cpu().numpy(), white) and np.array_equal(m[0].cpu().numpy(), mask)
    assert np.array_equal(rgba_crop_resize(x, None, 256, "float")[0].cpu().numpy(), literal_float(t).transpose(2, 0, 1))


def _bbox_images():
    e = np.zeros((9, 13, 4), dtype=np.uint8)
    single = e.copy(); single[4, 7, 3] = 205
    at_threshold = e.copy(); at_threshold[..., 3] = 204                   # not above the threshold: empty
    corners = e.copy(); corners[..., 3] = 17
    for y, x in ((0, 0), (0, 12), (8, 0), (8, 12)):
        corners[y, x, 3] = 255
    one_corner = e.copy(); one_corner[8, 12, 3] = 230
    return [e, single, at_threshold, corners, one_corner, R.soft_disc(9, 13, 3)]


def test_alpha_bbox_matches_argwhere(cuda):
    from gvfdiffusion_amd.utils import alpha_bbox
    imgs = np.stack(_bbox_images())
    got = alpha_bbox(dev(imgs, cuda))
    assert got.dtype == torch.int32 and got.shape == (len(imgs), 5) and got.is_cuda
    got = got.cpu().numpy()
    for i, img in enumerate(imgs):
        pts = np.argwhere(img[..., 3] > 0.8 * 255)
        want = (13, 9, -1, -1) if len(pts) == 0 else (pts[:, 1].min(), pts[:, 0].min(), pts[:, 1].max(), pts[:, 0].max())
        assert tuple(got[i, :4]) == tuple(int(v) for v in want) and got[i, 4] == img[..., 3].min(), i
    big = np.stack([R.soft_disc(300, 517, 5), R.hard_edges(300, 517, 6)])                                # several workgroups per image
    assert [tuple(r) for r in alpha_bbox(dev(big, cuda), threshold=100).cpu().tolist()] == [R.alpha_bbox(b, 100) for b in big]


@functools.lru_cache(maxsize=None)
def _routes():
    frames = np.stack([R.soft_disc(64, 64, s) for s in (41, 42, 43)])
    frames[1:, :, :, 3] = np.roll(frames[1:, :, :, 3], 3, axis=2)          # the later frames move; frame 0's box still crops them
    return frames, R.preprocess_video_frames(frames)


def test_preprocess_image_matches_the_reference_route(cuda):
    from gvfdiffusion_amd.trellis.pipelines import preprocess_image
    imgs = np.stack([R.soft_disc(48, 64, 51), R.hard_edges(48, 64, 52, cell=9)])                         # one box per image
    got = preprocess_image(dev(imgs, cuda), size=140)
    assert got.shape == (2, 140, 140, 3) and got.dtype == torch.uint8
    for i in range(2):
        want, box = R.preprocess_image(imgs[i], size=140)
        assert np.array_equal(got[i].cpu().numpy(), want)
        assert np.array_equal(want, literal_black(pil_crop_resize(imgs[i], box, (140, 140))))
    one = preprocess_image(dev(imgs[0], cuda), size=140)                   # a single (H, W, 4) image
    assert torch.equal(one[0], got[0])


def test_preprocess_video_frames_at_the_real_offsets(cuda):
    """64 x 64 source -> 380 x 380 at (66, 66) of 512 x 512, T = 3, frames 1-2 reusing frame 0's box."""
    from gvfdiffusion_amd.utils import preprocess_video_frames
    frames, (want, want_mask, want_box) = _routes()
    got, mask, box = preprocess_video_frames(dev(frames, cuda))
    assert box == want_box and got.shape == (3, 512, 512, 3) and mask.shape == (512, 512)
    assert np.array_equal(got.cpu().numpy(), want) and np.array_equal(mask.cpu().numpy(), want_mask)
    white, m = literal_white(pil_crop_resize(frames[2], box, (380, 380)))                                # and against Pillow + the literal lines
    assert np.array_equal(got[2, 66:446, 66:446].cpu().numpy(), white) and bool((got[2, :66] == 255).all())


D, DEPTH, GRID, REG = 128, 2, 4, 4          # the img_size = 56 encoder of tests/test_vit_ref.py


def _tiny_encoder(cuda):
    import vit_ref as V
    from gvfdiffusion_amd.model.dinov2 import DinoVisionTransformer
    m = DinoVisionTransformer(img_size=GRID * 14, patch_size=14, embed_dim=D, depth=DEPTH, num_heads=D // 64, num_register_tokens=REG, dtype=torch.bfloat16)
    m.load_state_dict(V.random_state_dict(D, DEPTH, GRID, REG, seed=3), strict=True)
    return m.to(cuda)


def test_inference_script_cond_rgba_routes(cuda, tmp_path, monkeypatch):
    """--cond_rgba FILE.pt: `wild` = preprocess_video_frames -> encode_cond_frames, `dataset` = RGBA frames straight into encode_cond_frames;
    both equal the encoder fed the reference route's pixels."""
    import inference_dpm_latent as S
    from gvfdiffusion_amd.utils import encode_cond_frames
    m = _tiny_encoder(cuda)
    monkeypatch.setattr(S, "image_encoder", lambda args, dev: m)
    frames, (want, _, _) = _routes()
    path = str(tmp_path / "rgba.pt")
    torch.save(torch.from_numpy(frames)[None], path)
    base = ["--synthetic", "--gaussians", "64", "--num_timesteps", "3", "--cond_rgba", path]
    _, cond = S.sample_inputs(S.create_argparser().parse_args(base), 0, cuda, {"image_cond_channels": D})
    assert cond.shape == (1, 3, GRID * GRID + 1, D) and cond.dtype == torch.float32
    assert torch.equal(cond[0], encode_cond_frames(m, dev(want, cuda)).float())
    _, cond = S.sample_inputs(S.create_argparser().parse_args(base + ["--cond_rgba_route", "dataset"]), 0, cuda, {"image_cond_channels": D})
    assert torch.equal(cond[0], encode_cond_frames(m, dev(R.dataset_pixels(frames, size=56), cuda)).float())


def test_encode_cond_frames_takes_rgba(cuda):
    """Route C through the encoder: RGBA frames in == the same encoder fed the reference route's pixels."""
    from gvfdiffusion_amd.trellis.pipelines.image_encoder import image01
    from gvfdiffusion_amd.utils import encode_cond_frames
    m = _tiny_encoder(cuda)
    frames = np.stack([R.soft_disc(40, 52, s) for s in (61, 62)])
    pixels = np.stack([literal_float(pil_crop_resize(f, None, (56, 56))).transpose(2, 0, 1) for f in frames])
    assert np.array_equal(R.dataset_pixels(frames, size=56), pixels)
    x = dev(frames, cuda)
    assert np.array_equal(image01(m, x).cpu().numpy(), pixels)
    got, want = encode_cond_frames(m, x), encode_cond_frames(m, dev(pixels, cuda))
    assert got.shape == (2, GRID * GRID + 1, D) and torch.equal(got, want)
    rgb = encode_cond_frames(m, x[..., :3].contiguous())                   # three channels: the route that was there before
    assert rgb.shape == got.shape and not torch.equal(rgb, got)


def test_refusals(cuda):
    from gvfdiffusion_amd._lib import GvfError
    from gvfdiffusion_amd.utils import alpha_bbox, preprocess_image, preprocess_video_frames, rgba_crop_resize
    img = R.soft_disc(20, 24, 71)
    opaque = img.copy(); opaque[..., 3] = 255
    faint = img.copy(); faint[..., 3] = np.minimum(faint[..., 3], 204)
    for fn in (preprocess_image, preprocess_video_frames):
        with pytest.raises(NotImplementedError, match="rembg"):
            fn(dev(opaque[None], cuda))
        with pytest.raises(ValueError):
            fn(dev(faint[None], cuda))                                     # no pixel above the threshold
        with pytest.raises(GvfError):
            fn(torch.from_numpy(img[None]))                                # host tensor
        with pytest.raises(ValueError):
            fn(dev(img[None], cuda).float())
        with pytest.raises(ValueError):
            fn(dev(img[None, ..., :3], cuda))
    later_opaque = np.stack([img, opaque])                                 # only frame 0 decides, as in the script
    assert preprocess_video_frames(dev(later_opaque, cuda), size=10, canvas=12)[0].shape == (2, 12, 12, 3)
    x = dev(img[None], cuda)
    with pytest.raises(GvfError):
        alpha_bbox(torch.from_numpy(img[None]))
    with pytest.raises(ValueError):
        alpha_bbox(x[0])
    with pytest.raises(ValueError):
        rgba_crop_resize(x, None, 10, mode="grey")
    with pytest.raises(ValueError):
        rgba_crop_resize(x, (5, 5, 5, 9), 10)
    with pytest.raises(ValueError):
        rgba_crop_resize(x, None, 16385)                                   # beyond GVF_RESAMPLE_MAX_WIDTH: refused before anything is allocated


def test_two_runs_give_equal_bytes(cuda):
    from gvfdiffusion_amd.utils import alpha_bbox, preprocess_video_frames
    frames, _ = _routes()
    x = dev(frames, cuda)
    a, b = preprocess_video_frames(x), preprocess_video_frames(x)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and a[2] == b[2]
    assert torch.equal(alpha_bbox(x), alpha_bbox(x))
