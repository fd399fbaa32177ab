"""ctypes bindings of include/gvf_clip.h (csrc/clip.hip) on torch device tensors: the 32 x 32 patch embedding of CLIP's ViT-B/32 image tower
with its token assembly, ln_pre, and the read-out ln_post(cls) @ proj -> unit vector -> cosine.  The blocks between them run on dit_ops
(gemm_ln_bf16 with EPI_QUICK_GELU_16, attention, gemm_resid_stats)."""
import ctypes

import torch

from .. import _lib
from . import dit_ops
from ._util import ptr as _p, stream as _stream

_vp, _i, _i64, _f = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64, ctypes.c_float

_lib.register({
    "gvf_clip_pack_patch_weight": (_i, [_i, _vp, _i, _vp, _vp]),
    "gvf_clip_patch_embed": (_i, [_i, _i, _vp, _vp, _i, _i, _vp, _vp, _vp, _i, _i, _vp, _vp]),
    "gvf_clip_ln_rows": (_i, [_vp, _i64, _i, _f, _vp, _vp, _vp, _vp]),
    "gvf_clip_head": (_i, [_i, _vp, _i, _i, _i, _f, _vp, _vp, _vp, _i, _vp, _vp, _vp, _vp, _vp]),
})

PATCH, PATCH_K = 32, 3072
IN_U8, IN_F32 = 0, 1
# OpenAI's preprocessing constants (clip.py's _transform: Normalize(mean, std)); transformers.image_utils.OPENAI_CLIP_MEAN / _STD are the same
CLIP_MEAN, CLIP_STD = (0.48145466, 0.4578275, 0.40821073), (0.26862954, 0.26130258, 0.27577711)


def operand_table(dtype=torch.float16, mean=CLIP_MEAN, std=CLIP_STD) -> torch.Tensor:
    """The (3, 256) operand of every (channel, uint8 pixel value), on the host: (u8 / 255 - mean[c]) / std[c] in fp32 -- ToTensor's .div(255),
    Normalize's sub_(mean).div_(std), each an IEEE fp32 operation -- then ONE rounding to `dtype`.  For fp16 this is bit for bit what
    ToTensor -> Normalize -> image.type(fp16) feeds the reference's conv1."""
    u = torch.arange(256, dtype=torch.float32).div(255)[None].repeat(3, 1)
    m = torch.tensor(mean, dtype=torch.float32).view(3, 1)
    s = torch.tensor(std, dtype=torch.float32).view(3, 1)
    return u.sub_(m).div_(s).to(dtype).contiguous()


def pack_patch_weight(w: torch.Tensor, dtype=torch.float16) -> torch.Tensor:
    """conv1.weight fp32 (D, 3, 32, 32) -> the 16-bit (D, 3072) operand image of patch_embed (k = c * 1024 + dy * 32 + dx)."""
    _lib.require_cuda(w)
    if w.dtype != torch.float32 or w.dim() != 4 or tuple(w.shape[1:]) != (3, PATCH, PATCH):
        raise _lib.GvfError(f"patch weight must be fp32 (D, 3, 32, 32), got {w.dtype} {tuple(w.shape)}")
    w = w.contiguous()
    out = torch.empty((w.shape[0], PATCH_K), dtype=dtype, device=w.device)
    _lib.check(_lib.lib().gvf_clip_pack_patch_weight(dit_ops.dt_code(dtype), _p(w), w.shape[0], _p(out), _stream(w)), "gvf_clip_pack_patch_weight")
    return out


def patch_embed(img: torch.Tensor, w_packed: torch.Tensor, cls_token: torch.Tensor, pos_embed: torch.Tensor, lut: torch.Tensor = None,
                out: torch.Tensor = None) -> torch.Tensor:
    """img (B, 3, S, S) -> the fp32 token stream (B, 1 + n, D) = [cls + pos[0] | conv32(operand) + pos[1:]] (before ln_pre).  img uint8: the
    operand is lut[c][pixel] (lut: operand_table(...) on the device, of w_packed's type); img fp32, normalised already: the operand is the
    pixel rounded once.  cls_token (D,), pos_embed (1 + n, D): fp32.  (S / 32)^2 must be the n patches pos_embed holds."""
    _lib.require_cuda(img, w_packed, cls_token, pos_embed, lut, out)
    if img.dtype not in (torch.uint8, torch.float32) or img.dim() != 4 or img.shape[1] != 3:
        raise _lib.GvfError(f"image must be uint8 or fp32 (B, 3, S, S), got {img.dtype} {tuple(img.shape)}")
    B, _, H, W = img.shape
    if H != W:
        raise _lib.GvfError(f"non-square images are not built: got {H} x {W}")
    kind = IN_U8 if img.dtype == torch.uint8 else IN_F32
    if kind == IN_U8 and (lut is None or lut.dtype != w_packed.dtype or tuple(lut.shape) != (3, 256) or not lut.is_contiguous()):
        raise _lib.GvfError("uint8 pixels need the (3, 256) operand table of the weight's 16-bit type")
    img = img.contiguous()
    D = w_packed.shape[0]
    for t in (cls_token, pos_embed):
        assert t.dtype == torch.float32 and t.is_contiguous() and t.shape[-1] == D
    assert w_packed.is_contiguous() and w_packed.shape[1] == PATCH_K and pos_embed.dim() == 2
    n = pos_embed.shape[0] - 1
    x = torch.empty((B, 1 + n, D), dtype=torch.float32, device=img.device) if out is None else out
    assert x.dtype == torch.float32 and x.is_contiguous() and tuple(x.shape) == (B, 1 + n, D)
    _lib.check(_lib.lib().gvf_clip_patch_embed(dit_ops.dt_code(w_packed.dtype), kind, _p(img), _p(lut), B, H, _p(w_packed), _p(cls_token),
                                               _p(pos_embed), n, D, _p(x), _stream(img)), "gvf_clip_patch_embed")
    return x


def ln_rows(x: torch.Tensor, ln_w: torch.Tensor, ln_b: torch.Tensor, eps: float = 1e-5, stats: torch.Tensor = None):
    """x fp32 (..., D) contiguous <- LayerNorm(x) * ln_w + ln_b IN PLACE; stats (rows, parts(D), 2) fp32, when given, <- the partial (sum, sum
    of squares) of the rows as written (the statistics gemm_ln_bf16 reads).  Returns x."""
    _lib.require_cuda(x, ln_w, ln_b, stats)
    if x.dtype != torch.float32 or not x.is_contiguous() or x.dim() < 2:
        raise _lib.GvfError("ln_rows takes a contiguous fp32 (..., D) tensor")
    D = x.shape[-1]
    rows = x.numel() // D if D else 0
    for t in (ln_w, ln_b):
        assert t.dtype == torch.float32 and t.is_contiguous() and tuple(t.shape) == (D,)
    if stats is not None:
        assert stats.dtype == torch.float32 and stats.is_contiguous() and stats.numel() >= rows * (D // 64) * 2
    _lib.check(_lib.lib().gvf_clip_ln_rows(_p(x), rows, D, float(eps), _p(ln_w), _p(ln_b), _p(stats), _stream(x)), "gvf_clip_ln_rows")
    return x


def head(x: torch.Tensor, ln_w: torch.Tensor, ln_b: torch.Tensor, proj16: torch.Tensor, ref_unit: torch.Tensor = None, eps: float = 1e-5,
         out=None):
    """x fp32 (B, L, D) -> (feat, unit, sim): feat (B, E) fp32 = r16(r16(ln_post(x[:, 0])) @ proj), unit = feat / |feat|, and, with ref_unit fp32
    (E,), sim (B,) = <unit, ref_unit> (else None).  proj16: the 16-bit (D, E) projection.  out: (feat, unit, sim) buffers to write into."""
    _lib.require_cuda(x, ln_w, ln_b, proj16, ref_unit)
    if x.dtype != torch.float32 or x.dim() != 3 or not x.is_contiguous():
        raise _lib.GvfError("the token stream must be a contiguous fp32 (B, tokens, D) tensor")
    B, L, D = x.shape
    assert proj16.dim() == 2 and proj16.shape[0] == D and proj16.is_contiguous()
    E = proj16.shape[1]
    for t in (ln_w, ln_b):
        assert t.dtype == torch.float32 and t.is_contiguous() and tuple(t.shape) == (D,)
    if ref_unit is not None:
        assert ref_unit.dtype == torch.float32 and ref_unit.is_contiguous() and tuple(ref_unit.shape) == (E,)
    if out is None:
        feat = torch.empty((B, E), dtype=torch.float32, device=x.device)
        unit = torch.empty((B, E), dtype=torch.float32, device=x.device)
        sim = torch.empty((B,), dtype=torch.float32, device=x.device) if ref_unit is not None else None
    else:
        feat, unit, sim = out
    _lib.check(_lib.lib().gvf_clip_head(dit_ops.dt_code(proj16.dtype), _p(x), B, L, D, float(eps), _p(ln_w), _p(ln_b), _p(proj16), E, _p(ref_unit),
                                        _p(feat), _p(unit), _p(sim), _stream(x)), "gvf_clip_head")
    return feat, unit, sim
