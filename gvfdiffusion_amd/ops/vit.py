"""ctypes bindings of include/gvf_vit.h (csrc/vit.hip) on torch device tensors: the DINOv2 patch embedding with its token assembly, and
the read-out of the fp32 token stream.  The blocks between them run on dit_ops (gemm_ln_bf16, attention, gemm_resid_stats)."""
import ctypes

import torch

from .. import _lib
from . import dit_ops
from ._util import ptr as _p, stream as _stream

_vp, _i, _f = ctypes.c_void_p, ctypes.c_int, ctypes.c_float
_f3 = ctypes.c_float * 3
_pf = ctypes.POINTER(ctypes.c_float)

_lib.register({
    "gvf_vit_pack_patch_weight": (_i, [_i, _vp, _i, _vp, _vp]),
    "gvf_vit_patch_embed": (_i, [_i, _vp, _i, _i, _i, _pf, _pf, _vp, _vp, _vp, _vp, _i, _vp, _i, _i, _vp, _vp, _vp]),
    "gvf_vit_tokens_out": (_i, [_vp, _i, _i, _i, _i, _i, _f, _vp, _vp, _i, _i, _vp, _vp]),
})

PATCH, PATCH_K, PATCH_KPAD = 14, 588, 608
IMAGENET_MEAN, IMAGENET_STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
OUT_COPY, OUT_LN_AFFINE, OUT_LN = 0, 1, 2
ORDER_STORED, ORDER_PATCHES_CLS = 0, 1


def pack_patch_weight(w: torch.Tensor, dtype=torch.float16) -> torch.Tensor:
    """patch_embed.proj.weight fp32 (D, 3, 14, 14) -> the 16-bit (D, 608) operand image of patch_embed (k = c * 196 + dy * 14 + dx, zero-padded)."""
    _lib.require_cuda(w)
    if w.dtype != torch.float32 or w.dim() != 4 or tuple(w.shape[1:]) != (3, PATCH, PATCH):
        raise _lib.GvfError(f"patch weight must be fp32 (D, 3, 14, 14), got {w.dtype} {tuple(w.shape)}")
    w = w.contiguous()
    out = torch.empty((w.shape[0], PATCH_KPAD), dtype=dtype, device=w.device)
    _lib.check(_lib.lib().gvf_vit_pack_patch_weight(dit_ops.dt_code(dtype), _p(w), w.shape[0], _p(out), _stream(w)), "gvf_vit_pack_patch_weight")
    return out


def patch_embed(img: torch.Tensor, w_packed: torch.Tensor, bias, cls_token: torch.Tensor, register_tokens, pos_embed: torch.Tensor,
                mean=IMAGENET_MEAN, std=IMAGENET_STD, stats: bool = True):
    """img fp32 (B, 3, H, W) in [0, 1] -> (x, stats): the fp32 token stream (B, 1 + R + n, D) = [cls + pos[0] | registers | conv + bias + pos[1:]]
    of the z-scored image, and the partial LayerNorm statistics (B * (1 + R + n), parts(D), 2) gemm_ln_bf16 reads (None with stats=False).
    cls_token (D,), register_tokens (R, D) or None, pos_embed (1 + n, D): fp32.  H / 14 x W / 14 must be the n patches pos_embed holds."""
    _lib.require_cuda(img, w_packed, cls_token, pos_embed, bias, register_tokens)
    if img.dtype != torch.float32 or img.dim() != 4 or img.shape[1] != 3:
        raise _lib.GvfError(f"image must be fp32 (B, 3, H, W), got {img.dtype} {tuple(img.shape)}")
    img = img.contiguous()
    D = w_packed.shape[0]
    R = 0 if register_tokens is None else register_tokens.shape[0]
    for t in (bias, cls_token, register_tokens, pos_embed):
        assert t is None or (t.dtype == torch.float32 and t.is_contiguous() and t.shape[-1] == D)
    assert w_packed.is_contiguous() and w_packed.shape[1] == PATCH_KPAD and pos_embed.dim() == 2
    B, _, H, W = img.shape
    n = pos_embed.shape[0] - 1
    x = torch.empty((B, 1 + R + n, D), dtype=torch.float32, device=img.device)
    st = torch.empty((B * (1 + R + n), dit_ops.gemm_stats_parts(D), 2), dtype=torch.float32, device=img.device) if stats else None
    _lib.check(_lib.lib().gvf_vit_patch_embed(dit_ops.dt_code(w_packed.dtype), _p(img), B, H, W, _f3(*mean), _f3(*std), _p(w_packed), _p(bias),
                                              _p(cls_token), _p(register_tokens), R, _p(pos_embed), n, D, _p(x), _p(st), _stream(img)),
               "gvf_vit_patch_embed")
    return x, st


def tokens_out(x: torch.Tensor, num_register_tokens: int, mode: int = OUT_COPY, order: int = ORDER_STORED, out_dtype=torch.float32,
               ln_w=None, ln_b=None, eps: float = None) -> torch.Tensor:
    """x fp32 (B, 1 + R + n, D) (x_prenorm) -> (B, 1 + R + n, D) [ORDER_STORED] or (B, n + 1, D) = patches then cls [ORDER_PATCHES_CLS], fp32 or
    fp16: a copy, the affine LayerNorm (ln_w, ln_b; eps 1e-6: x_norm) or the plain one (eps 1e-5: F.layer_norm(x, x.shape[-1:]))."""
    _lib.require_cuda(x, ln_w, ln_b)
    if x.dtype != torch.float32 or x.dim() != 3 or not x.is_contiguous():
        raise _lib.GvfError("the token stream must be a contiguous fp32 (B, tokens, D) tensor")
    if out_dtype not in (torch.float32, torch.float16):
        raise _lib.GvfError(f"tokens_out writes fp32 or fp16, not {out_dtype}")
    B, T, D = x.shape
    R = int(num_register_tokens)
    n = T - 1 - R
    if eps is None:
        eps = 1e-6 if mode == OUT_LN_AFFINE else 1e-5
    out = torch.empty((B, T if order == ORDER_STORED else n + 1, D), dtype=out_dtype, device=x.device)
    _lib.check(_lib.lib().gvf_vit_tokens_out(_p(x), B, R, n, D, int(mode), float(eps), _p(ln_w), _p(ln_b), int(order),
                                             int(out_dtype == torch.float16), _p(out), _stream(x)), "gvf_vit_tokens_out")
    return out
