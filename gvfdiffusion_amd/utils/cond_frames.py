"""The DiT's image condition from frames: what scripts/encode_img_cond_dinov2_feature.py:36-64 stores per object, on the HIP DINOv2 encoder."""
import torch

from ..ops import vit as vit_ops

__all__ = ["encode_cond_frames"]


@torch.no_grad()
def encode_cond_frames(model, frames: torch.Tensor, normalize: bool = False) -> torch.Tensor:
    """frames: uint8 RGB (T, H, W, 3) or RGBA (T, H, W, 4) of any size, or fp32 (T, 3, S, S) in [0, 1] -> fp16 (T, n + 1, D): per frame the
    n patch tokens, then the cls token (registers dropped) -- of x_prenorm, or of x_norm with normalize=True (the script's --normalize) --
    rounded to fp16 as the script's `.astype(np.float16)` does.  RGBA frames are the script's renders: resized as RGBA and multiplied by
    their alpha in fp32 on the device (image01).  The in-the-wild route (crop, white composite) is utils.preprocess_video_frames, whose
    RGB frames come here."""
    from ..trellis.pipelines.image_encoder import image01
    x = model.forward_stream(image01(model, frames))
    if normalize:
        w, b = model.weight_images()["norm"]
        return vit_ops.tokens_out(x, model.num_register_tokens, vit_ops.OUT_LN_AFFINE, vit_ops.ORDER_PATCHES_CLS, torch.float16, w, b, eps=1e-6)
    return vit_ops.tokens_out(x, model.num_register_tokens, vit_ops.OUT_COPY, vit_ops.ORDER_PATCHES_CLS, torch.float16)
