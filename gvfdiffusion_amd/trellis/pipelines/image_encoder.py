"""The front of the TRELLIS image -> 3D pipeline: `encode_image` / `get_cond` (trellis/pipelines/trellis_image_to_3d.py:121-163) on the HIP DINOv2
encoder (model/dinov2.py), and `image_to_gaussians`, which chains it with `tokens_to_gaussians`.

`preprocess_image` (:85-119) for an image that carries alpha -- bounding box, crop, Pillow's premultiplied-alpha RGBA resize, rgb * alpha -- is
utils/rgba_ops.py (csrc/rgba.hip), re-exported here; its output feeds `encode_image` / `image_to_gaussians` as any RGB frames do.
Not built: rembg, the background removal of an image without alpha (a downloaded network); such an image is refused."""
from typing import Optional

import torch

from ... import _lib
from ...ops import vit as vit_ops
from ...utils.image_ops import resize_pad_crop_u8
from ...utils.rgba_ops import preprocess_image, rgba_crop_resize
from .samplers import tokens_to_gaussians

__all__ = ["image01", "encode_image", "get_cond", "image_to_gaussians", "preprocess_image"]


def image01(model, image: torch.Tensor) -> torch.Tensor:
    """What the encoder's patch kernel reads: fp32 (B, 3, S, S) in [0, 1], S = model.img_size.
    image: such a tensor already, or uint8 RGB frames (B, H, W, 3) of any size -- those are resized to S x S exactly as
    `Image.resize((S, S), Image.LANCZOS)` does (gvf_resample_place_u8, bit-identical to Pillow) and divided by 255 in fp32
    (`np.array(i).astype(np.float32) / 255`, :136-138) -- or uint8 RGBA frames (B, H, W, 4), which follow the dataset script
    (scripts/encode_img_cond_dinov2_feature.py:40-44): resized as RGBA (premultiplied, as Pillow does), divided by 255 and multiplied by
    their alpha in fp32, without a rounding to 8 bit in between (gvf_rgba_resample_u8)."""
    _lib.require_cuda(image)
    S = model.img_size
    if image.dtype == torch.uint8:
        if image.dim() == 4 and image.shape[-1] == 4:
            return rgba_crop_resize(image, None, S, mode="float")
        if image.dim() != 4 or image.shape[-1] != 3:
            raise ValueError(f"uint8 frames must be (B, H, W, 3) RGB or (B, H, W, 4) RGBA, got {tuple(image.shape)}")
        planes = image.permute(0, 3, 1, 2).contiguous()
        return resize_pad_crop_u8(planes, S, S).float() / 255
    if image.dim() != 4 or tuple(image.shape[1:]) != (3, S, S) or not image.is_floating_point():
        raise ValueError(f"the image must be a float (B, 3, {S}, {S}) tensor in [0, 1] or uint8 (B, H, W, 3) frames, got {image.dtype} {tuple(image.shape)}")
    return image.float().contiguous()


@torch.no_grad()
def encode_image(model, image: torch.Tensor) -> torch.Tensor:
    """-> fp32 (B, 1 + R + n, D): F.layer_norm(model(normalize(image), is_training=True)['x_prenorm']) -- all tokens, registers included, as the
    reference's encode_image returns them.  The ImageNet z-score runs inside the patch kernel."""
    x = model.forward_stream(image01(model, image))
    return vit_ops.tokens_out(x, model.num_register_tokens, vit_ops.OUT_LN, vit_ops.ORDER_STORED, torch.float32, eps=1e-5)


def get_cond(model, image: torch.Tensor) -> dict:
    cond = encode_image(model, image)
    return {"cond": cond, "neg_cond": torch.zeros_like(cond)}


@torch.no_grad()
def image_to_gaussians(models: dict, image: torch.Tensor, num_samples: int = 1, sparse_structure_sampler_params: Optional[dict] = None,
                       slat_sampler_params: Optional[dict] = None, slat_normalization: Optional[dict] = None, noise: Optional[torch.Tensor] = None,
                       **model_kwargs):
    """Pixels -> Gaussians: encode_image on models["image_cond_model"], zeros as the negative condition (get_cond), then tokens_to_gaussians
    with the same arguments.  -> (the decoder's Gaussians, the structured latent, the coords)."""
    c = get_cond(models["image_cond_model"], image)
    return tokens_to_gaussians(models, c["cond"], c["neg_cond"], num_samples, sparse_structure_sampler_params, slat_sampler_params,
                               slat_normalization, noise=noise, **model_kwargs)
