"""Fused L1 + SSIM image loss (include/gvf_loss.h, csrc/loss.hip): the render loss of the motion-VAE training step without its
LPIPS term (train_vae.py:328-334), SSIM as utils/loss_util.py:ssim (11 x 11 Gaussian window, sigma 1.5, zero padding 5,
C1 = 0.01^2, C2 = 0.03^2, mean over every pixel, channel and image).  Forward and gradient are HIP kernels; there is no CPU
fallback.  Differentiable in `pred` only."""
import ctypes

import torch

from .. import _lib
from ._util import f32c as _f32c, scratch as _scratch

_vp, _i, _i64, _sz, _f = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64, ctypes.c_size_t, ctypes.c_float

SSIM_GRAD = 1   # GVF_IMAGE_LOSS_SSIM_GRAD

_lib.register({
    "gvf_ssim_window": (_i, [ctypes.POINTER(_f)]),
    "gvf_image_loss_scratch_bytes": (_i, [_i64, _i, _i, _i, ctypes.POINTER(_sz)]),
    "gvf_image_loss_forward": (_i, [_vp, _vp, _i64, _i, _i, _f, _f, _vp, _vp, _sz, _i, _vp]),
    "gvf_image_loss_backward": (_i, [_vp, _vp, _i64, _i, _i, _f, _f, _vp, _vp, _vp, _sz, _i, _vp]),
})


def window_taps() -> torch.Tensor:
    """The 11 fp32 taps of the 1-D window the kernels apply (the reference's gaussian(11, 1.5))."""
    buf = (_f * 11)()
    _lib.check(_lib.lib().gvf_ssim_window(buf), "gvf_ssim_window")
    return torch.tensor(list(buf), dtype=torch.float32)


def _planes(pred: torch.Tensor, target: torch.Tensor):
    if not isinstance(pred, torch.Tensor) or not isinstance(target, torch.Tensor):
        raise TypeError("image_loss: pred and target must be tensors")
    _lib.require_cuda(pred, target)
    if pred.dim() not in (3, 4):
        raise ValueError(f"image_loss: expected (C,H,W) or (N,C,H,W) images, got shape {tuple(pred.shape)}")
    if pred.shape != target.shape:
        raise ValueError(f"image_loss: pred {tuple(pred.shape)} and target {tuple(target.shape)} differ in shape")
    if pred.device != target.device:
        raise ValueError("image_loss: pred and target are on different devices")
    H, W = int(pred.shape[-2]), int(pred.shape[-1])
    planes = pred.numel() // max(H * W, 1)
    if planes == 0 or H == 0 or W == 0:
        raise ValueError(f"image_loss: empty images {tuple(pred.shape)}")
    return planes, H, W


class _ImageLossFn(torch.autograd.Function):
    """(pred, target) -> (loss, mean L1, mean SSIM); the gradient flows to pred only.  keep_ssim: the forward keeps the SSIM
    partial maps for the backward (needed whenever the SSIM term can reach the gradient)."""

    @staticmethod
    def forward(ctx, pred, target, w_l1: float, w_ssim: float, keep_ssim: bool):
        planes, H, W = _planes(pred, target)
        flags = SSIM_GRAD if (keep_ssim and ctx.needs_input_grad[0]) else 0
        scratch = _scratch("gvf_image_loss_scratch_bytes", pred.device, planes, H, W, flags)
        terms = torch.empty(3, dtype=torch.float32, device=pred.device)
        l = _lib.lib()
        _lib.check(l.gvf_image_loss_forward(_lib.ptr(pred), _lib.ptr(target), planes, H, W, float(w_l1), float(w_ssim), _lib.ptr(terms),
                                            _lib.ptr(scratch), scratch.numel(), flags, _lib.current_stream(pred.device)),
                   "gvf_image_loss_forward")
        if ctx.needs_input_grad[0]:
            ctx.save_for_backward(pred, target)
            ctx.scratch, ctx.flags, ctx.geom, ctx.w = scratch, flags, (planes, H, W), (float(w_l1), float(w_ssim))
        ctx.set_materialize_grads(False)
        return terms[0], terms[1], terms[2]

    @staticmethod
    def backward(ctx, g_loss, g_l1, g_ssim):
        if not ctx.needs_input_grad[0] or (g_loss is None and g_l1 is None and g_ssim is None):
            return None, None, None, None, None
        pred, target = ctx.saved_tensors
        planes, H, W = ctx.geom
        w_l1, w_ssim = ctx.w
        ssim_used = (g_loss is not None and w_ssim != 0.0) or g_ssim is not None
        if ssim_used and not ctx.flags & SSIM_GRAD:
            raise RuntimeError("image_loss: the SSIM term reaches the gradient but its maps were not kept (keep_ssim=False)")
        z = torch.zeros((), dtype=torch.float32, device=pred.device)
        gt3 = torch.stack([z if g is None else g.reshape(()).float() for g in (g_loss, g_l1, g_ssim)]).contiguous()
        grad = torch.empty_like(pred)
        flags = ctx.flags if ssim_used else 0
        _lib.check(_lib.lib().gvf_image_loss_backward(_lib.ptr(pred), _lib.ptr(target), planes, H, W, w_l1, w_ssim, _lib.ptr(gt3),
                                                      _lib.ptr(grad), _lib.ptr(ctx.scratch), ctx.scratch.numel(), flags,
                                                      _lib.current_stream(pred.device)),
                   "gvf_image_loss_backward")
        return grad, None, None, None, None


def _prepare(pred, target):
    if isinstance(target, torch.Tensor) and target.requires_grad:
        raise ValueError("image_loss: target requires grad; the loss is differentiable in pred only (detach the target)")
    _planes(pred, target)
    return _f32c(pred), _f32c(target)


def image_loss(pred: torch.Tensor, target: torch.Tensor, l1_weight: float = 1.0, ssim_weight: float = 0.2, return_terms: bool = False):
    """l1_weight * mean|pred - target| + ssim_weight * (1 - ssim(pred, target)) over (C,H,W) or (N,C,H,W) images, as one fused HIP
    forward and one fused HIP gradient.  return_terms: also return the mean L1 and the mean SSIM (0-d tensors, themselves
    differentiable in pred)."""
    pred, target = _prepare(pred, target)
    keep = ssim_weight != 0.0 or return_terms
    loss, l1, s = _ImageLossFn.apply(pred, target, float(l1_weight), float(ssim_weight), keep)
    return (loss, l1, s) if return_terms else loss


def ssim(img1: torch.Tensor, img2: torch.Tensor) -> torch.Tensor:
    """Mean SSIM (0-d tensor) over (C,H,W) or (N,C,H,W) images: utils/loss_util.py:ssim(img1, img2, size_average=True) on the
    HIP kernels; differentiable in img1."""
    img1, img2 = _prepare(img1, img2)
    return _ImageLossFn.apply(img1, img2, 0.0, 0.0, True)[2]
