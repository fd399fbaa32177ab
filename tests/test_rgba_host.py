"""RGBA condition preprocessing, what needs no GPU: the inference script's --cond_rgba flags, the argument errors of utils/rgba_ops.py and
the host-side refusals of the two C entry points (include/gvf_image.h)."""
import ctypes

import pytest
import torch


def test_inference_script_takes_cond_rgba():
    import inference_dpm_latent as S
    a = S.create_argparser().parse_args(["--synthetic", "--cond_rgba", "rgba.pt"])
    assert a.cond_rgba == "rgba.pt" and a.cond_rgba_route == "wild" and a.cond_frames is None and a.cond_images is None
    S.check_cond_sources(a)
    a = S.create_argparser().parse_args(["--synthetic", "--cond_rgba", "rgba.pt", "--cond_rgba_route", "dataset"])
    assert a.cond_rgba_route == "dataset"
    with pytest.raises(SystemExit):
        S.create_argparser().parse_args(["--cond_rgba", "rgba.pt", "--cond_rgba_route", "studio"])
    for other in ("--cond_frames", "--cond_images"):                       # one source of the condition
        with pytest.raises(SystemExit, match="cond_rgba"):
            S.main(["--synthetic", "--cond_rgba", "rgba.pt", other, "x.pt"])
    b = S.create_argparser().parse_args(["--synthetic", "--cond_frames", "frames.pt"])                 # the existing flags as before
    assert b.cond_rgba is None and b.cond_frames == "frames.pt"
    S.check_cond_sources(b)
    with pytest.raises(SystemExit):                                      # neither a checkpoint nor --synthetic: no silent random encoder
        S.image_encoder(S.create_argparser().parse_args(["--cond_rgba", "rgba.pt"]), torch.device("cpu"))


def test_exports():
    import gvfdiffusion_amd.utils as U
    from gvfdiffusion_amd.trellis import pipelines as P
    for n in ("alpha_bbox", "crop_box", "rgba_crop_resize", "preprocess_image", "preprocess_video_frames"):
        assert callable(getattr(U, n))
    assert P.preprocess_image is U.preprocess_image


def test_argument_errors_need_no_gpu():
    from gvfdiffusion_amd._lib import GvfError
    from gvfdiffusion_amd.utils import alpha_bbox, crop_box, preprocess_image, preprocess_video_frames, rgba_crop_resize
    img = torch.zeros((2, 8, 9, 4), dtype=torch.uint8)
    for fn in (alpha_bbox, preprocess_image, preprocess_video_frames, lambda x: rgba_crop_resize(x, None, 4)):
        with pytest.raises(GvfError):
            fn(img)                                                        # a host tensor: no CPU fallback
        with pytest.raises(ValueError):
            fn(img.float())
        with pytest.raises(ValueError):
            fn(img[..., :3])
        with pytest.raises(ValueError):
            fn(img[None])                                                  # rank 5
    with pytest.raises(ValueError):
        crop_box((9, 8, -1, -1))                                           # the empty sentinel, as numpy's min of nothing
    assert crop_box((2, 2, 2, 2)) == ((2.0, 2.0, 2.0, 2.0), (2, 2, 2, 2))


def test_c_entry_points_refuse_bad_arguments_on_the_host():
    from gvfdiffusion_amd import _lib
    import gvfdiffusion_amd.utils  # noqa: F401  (registers the entry points)
    from gvfdiffusion_amd.utils.image_ops import _Table
    l = _lib.lib()
    p = ctypes.c_void_p(4096)                                              # never dereferenced: every call below is refused before a launch
    E = _lib.GVF_EINVAL
    assert l.gvf_alpha_bbox_u8(None, 1, 8, 8, 204, p, None) == E
    assert l.gvf_alpha_bbox_u8(p, 1, 8, 8, 256, p, None) == E
    assert l.gvf_alpha_bbox_u8(p, 1, 8, 16385, 204, p, None) == E
    assert l.gvf_alpha_bbox_u8(ctypes.c_void_p(4097), 1, 8, 8, 204, p, None) == E      # pixels are read as 32-bit words
    assert l.gvf_alpha_bbox_u8(p, 65536, 8, 8, 204, p, None) == E
    assert l.gvf_alpha_bbox_u8(p, 0, 8, 8, 204, p, None) == _lib.GVF_OK

    def resample(src=p, n=1, in_h=8, in_w=8, cx=0, cy=0, cw=8, ch=8, th=None, tv=None, tmp=p, mode=0, dst=p, dh=8, dw=8, pad=0):
        return l.gvf_rgba_resample_u8(src, n, in_h, in_w, cx, cy, cw, ch, th, tv, tmp, mode, dst, None, dh, dw, 0, 0, pad, None)
    assert resample(n=0) == _lib.GVF_OK
    assert resample(src=None) == E and resample(dst=None) == E
    assert resample(cw=0) == E and resample(cw=16385) == E and resample(ch=16385) == E and resample(dw=16385) == E and resample(in_w=16385) == E
    assert resample(mode=4) == E and resample(mode=-1) == E and resample(pad=256) == E and resample(n=65536) == E
    good = _Table(4096, 4096, 4096, 7, 8)
    assert resample(th=ctypes.byref(_Table(4096, 4096, 4096, 257, 8))) == E            # more taps than GVF_RESAMPLE_MAX_TAPS
    assert resample(tv=ctypes.byref(_Table(4096, 4096, 4096, 7, 16385))) == E          # more outputs than GVF_RESAMPLE_MAX_WIDTH
    assert resample(th=ctypes.byref(_Table(None, 4096, 4096, 7, 8))) == E
    assert resample(th=ctypes.byref(good), tmp=None) == E                              # a pass needs the intermediate buffer
