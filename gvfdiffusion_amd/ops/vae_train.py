"""The operators of the motion VAE's training path that are not matrix products or attention, as torch.autograd.Functions on the HIP kernels of
include/gvf_vae_train.h (csrc/vae_train.hip):

  geglu             a = x * gelu_erf(g) on the 16-bit rows u = [x | g] (the output of net.0), fp32 inside; the backward recomputes from the saved u.
  embed             e = LN(r W^T + b) + LN(PointEmbed(r[:, :3])) as an fp32 tensor; gradients of W, b and (when r requires one) of the rows r.
  posterior_groups  (z, kl[G]) from mean / logvar with the reference's clamp(logvar, -30, 20): one KL term per group of L rows.

The reductions (dW, db, kl) are deterministic: one partial per workgroup, added in a fixed order.  There is no CPU fallback."""
import ctypes

import torch

from .. import _lib
from . import dit_ops
from ._util import psz as _psz, ptr as _p, rows16 as _rows16, scratch as _scratch

_vp, _i, _i64, _sz, _f = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64, ctypes.c_size_t, ctypes.c_float

_lib.register({
    "gvf_geglu_fwd": (_i, [_i, _vp, _i64, _vp, _i64, _i64, _i, _vp]),
    "gvf_geglu_bwd": (_i, [_i, _vp, _i64, _vp, _i64, _vp, _i64, _i64, _i, _vp]),
    "gvf_vae_embed_train_fwd": (_i, [_vp, _i, _vp, _vp, _vp, _vp, _i64, _i, _f, _vp]),
    "gvf_vae_embed_bwd_workspace_bytes": (_i, [_i64, _i, _i, _psz]),
    "gvf_vae_embed_bwd": (_i, [_vp, _i, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i64, _i, _f, _vp, _sz, _vp]),
    "gvf_posterior_groups_workspace_bytes": (_i, [_i64, _i64, _i, _psz]),
    "gvf_posterior_groups_fwd": (_i, [_vp, _i64, _vp, _i64, _vp, _vp, _vp, _i64, _i64, _i, _vp, _sz, _vp]),
    "gvf_posterior_groups_bwd": (_i, [_vp, _i64, _vp, _i64, _vp, _vp, _vp, _vp, _i64, _vp, _i64, _i64, _i64, _i, _vp]),
})

EMBED_EPS = 1e-5          # nn.LayerNorm's default: the two embedding norms of the reference (the PreNorm norms use 1e-6)
MAX_QDIM, MAX_C = 16, 768


def _row_ld(x):
    """leading dimension, in elements, of what _rows16 returned"""
    return x.stride(0) if x.shape[0] > 1 else x.shape[1]


# ---- GEGLU ------------------------------------------------------------------------------------------------------------------------------
class _GegluFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, u):
        rows, F = u.shape[0], u.shape[1] // 2
        uv = _rows16(u)
        ldu = _row_ld(uv)
        a = torch.empty((rows, F), dtype=u.dtype, device=u.device)
        if rows > 0:
            _lib.check(_lib.lib().gvf_geglu_fwd(dit_ops.dt_code(u.dtype), _p(uv), ldu, _p(a), F, rows, F, _lib.current_stream(u.device)), "gvf_geglu_fwd")
        ctx.save_for_backward(uv)
        ctx.ldu = ldu
        return a

    @staticmethod
    def backward(ctx, da):
        uv, = ctx.saved_tensors
        rows, F = uv.shape[0], uv.shape[1] // 2
        if da.dtype != uv.dtype:
            da = da.to(uv.dtype)
        dav = _rows16(da)
        du = torch.empty((rows, 2 * F), dtype=uv.dtype, device=uv.device)
        if rows > 0:
            _lib.check(_lib.lib().gvf_geglu_bwd(dit_ops.dt_code(uv.dtype), _p(uv), ctx.ldu, _p(dav), _row_ld(dav), _p(du), 2 * F, rows, F,
                                                _lib.current_stream(uv.device)), "gvf_geglu_bwd")
        return du


def geglu(u):
    """u fp16 / bf16 [..., 2F] = [x | g] (F a multiple of 8; a row-strided 2-D view is read in place) -> a [..., F] = x * gelu(g) with the exact
    erf GELU, fp32 inside, rounded once; differentiable in u.  No NaN for any finite u and incoming gradient."""
    _lib.require_cuda(u)
    dit_ops.dt_code(u.dtype)
    if u.dim() < 1 or u.shape[-1] == 0 or u.shape[-1] % 16 != 0:
        raise ValueError(f"geglu: the last dimension must be 2F with F a positive multiple of 8, got {tuple(u.shape)} (there is no fallback)")
    u2 = u if u.dim() == 2 else u.reshape(-1, u.shape[-1])
    return _GegluFn.apply(u2).reshape(*u.shape[:-1], u.shape[-1] // 2)


# ---- embedding --------------------------------------------------------------------------------------------------------------------------
class _EmbedFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, r, weight, bias, omega):
        P, qdim = r.shape
        C = weight.shape[0]
        e = torch.empty((P, C), dtype=torch.float32, device=r.device)
        if P > 0:
            _lib.check(_lib.lib().gvf_vae_embed_train_fwd(_p(r), qdim, _p(weight), _p(bias), _p(omega), _p(e), P, C, EMBED_EPS,
                                                          _lib.current_stream(r.device)), "gvf_vae_embed_train_fwd")
        ctx.save_for_backward(r, weight, bias, omega)
        return e

    @staticmethod
    def backward(ctx, de):
        r, weight, bias, omega = ctx.saved_tensors
        P, qdim = r.shape
        C = weight.shape[0]
        need = ctx.needs_input_grad
        dev = r.device
        if P == 0:
            return (torch.zeros_like(r) if need[0] else None, torch.zeros_like(weight) if need[1] else None,
                    torch.zeros_like(bias) if need[2] else None, None)
        if de.dtype != torch.float32 or not de.is_contiguous():
            de = de.float().contiguous()
        dW, db = torch.empty_like(weight), torch.empty_like(bias)
        dr = torch.empty_like(r) if need[0] else None
        ws = _scratch("gvf_vae_embed_bwd_workspace_bytes", dev, P, qdim, C)
        _lib.check(_lib.lib().gvf_vae_embed_bwd(_p(r), qdim, _p(weight), _p(bias), _p(omega), _p(de), _p(dW), _p(db), _p(dr), P, C, EMBED_EPS,
                                                _p(ws), ws.numel(), _lib.current_stream(dev)), "gvf_vae_embed_bwd")
        return dr, (dW if need[1] else None), (db if need[2] else None), None


def embed(r, weight, bias, omega):
    """r fp32 [P, qdim] (columns 0..2 = xyz), weight fp32 [C, qdim], bias fp32 [C], omega fp32 [C / 6] (PointEmbed's frequencies) ->
    e fp32 [P, C] = LN_1e-5(r weight^T + bias) + LN_1e-5(PointEmbed(r[:, :3])).  Differentiable in weight, bias and r (the gradient of r is
    computed only when r requires one); the backward recomputes both rows and their statistics."""
    _lib.require_cuda(r, weight, bias, omega)
    if r.dim() != 2 or weight.dim() != 2 or bias.dim() != 1 or omega.dim() != 1 or any(t.dtype != torch.float32 for t in (r, weight, bias, omega)):
        raise ValueError("embed: r [P, qdim], weight [C, qdim], bias [C], omega [C / 6] must be fp32 tensors")
    qdim, C = r.shape[1], weight.shape[0]
    if not 3 <= qdim <= MAX_QDIM or C == 0 or C > MAX_C or C % 6 != 0:
        raise ValueError(f"embed: qdim in 3..{MAX_QDIM} and C a multiple of 6 up to {MAX_C} are built, got qdim {qdim}, C {C} (there is no fallback)")
    if weight.shape[1] != qdim or bias.shape[0] != C or omega.shape[0] != C // 6:
        raise ValueError(f"embed: weight {tuple(weight.shape)}, bias {tuple(bias.shape)}, omega {tuple(omega.shape)} do not fit r {tuple(r.shape)}")
    return _EmbedFn.apply(r.contiguous(), weight.contiguous(), bias.contiguous(), omega.contiguous())


# ---- grouped posterior ------------------------------------------------------------------------------------------------------------------
def _ld(t):
    """fp32 [rows, Dl] with unit column stride read through its row stride; else a copy -> (tensor, leading dimension)"""
    if t.stride(1) != 1 or (t.shape[0] > 1 and t.stride(0) < t.shape[1]):
        t = t.contiguous()
    return t, (t.stride(0) if t.shape[0] > 1 else t.shape[1])


class _PosteriorGroupsFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, mean, logvar, eps, G):
        rows, Dl = eps.shape
        L = rows // G
        dev = mean.device
        mv, ldm = _ld(mean)
        lv, ldl = _ld(logvar)
        z = torch.empty((rows, Dl), dtype=torch.float32, device=dev)
        kl = torch.empty((G,), dtype=torch.float32, device=dev)
        ws = _scratch("gvf_posterior_groups_workspace_bytes", dev, G, L, Dl)
        _lib.check(_lib.lib().gvf_posterior_groups_fwd(_p(mv), ldm, _p(lv), ldl, _p(eps), _p(z), _p(kl), G, L, Dl, _p(ws), ws.numel(),
                                                       _lib.current_stream(dev)), "gvf_posterior_groups_fwd")
        ctx.save_for_backward(mv, lv, eps)
        ctx.dims = (G, L, Dl, ldm, ldl)
        ctx.set_materialize_grads(False)
        return z, kl

    @staticmethod
    def backward(ctx, dz, dkl):
        mv, lv, eps = ctx.saved_tensors
        G, L, Dl, ldm, ldl = ctx.dims
        if dz is None and dkl is None:
            return None, None, None, None
        if dz is not None and (dz.dtype != torch.float32 or not dz.is_contiguous()):
            dz = dz.float().contiguous()
        if dkl is not None:
            dkl = dkl.float().reshape(G).contiguous()
        d = torch.empty((2, G * L, Dl), dtype=torch.float32, device=mv.device)
        _lib.check(_lib.lib().gvf_posterior_groups_bwd(_p(mv), ldm, _p(lv), ldl, _p(eps), _p(dz), _p(dkl), _p(d[0]), Dl, _p(d[1]), Dl, G, L, Dl,
                                                       _lib.current_stream(mv.device)), "gvf_posterior_groups_bwd")
        return d[0], d[1], None, None


def posterior_groups(mean, logvar, eps, groups):
    """mean, logvar fp32 [G * L, Dl] (unit column stride, any row stride: two column slices of one matrix are read in place), eps fp32
    [G * L, Dl] (the noise), groups = G ->
        z fp32 [G * L, Dl] = mean + exp(0.5 lv) eps,   kl fp32 [G] = 0.5 mean over each group's L * Dl elements of (mean^2 + exp(lv) - 1 - lv),
    lv = clamp(logvar, -30, 20) (DiagonalGaussianDistribution of the reference).  Differentiable in mean and logvar through both outputs, in
    one backward launch; the clamp passes the gradient on its bounds and blocks it strictly outside."""
    _lib.require_cuda(mean, logvar, eps)
    if mean.dim() != 2 or mean.shape != logvar.shape or mean.shape != eps.shape or any(t.dtype != torch.float32 for t in (mean, logvar, eps)):
        raise ValueError(f"posterior_groups: mean, logvar and eps must be fp32 [G * L, Dl] tensors of one shape, got {tuple(mean.shape)} / "
                         f"{tuple(logvar.shape)} / {tuple(eps.shape)}")
    G = int(groups)
    if G <= 0 or mean.shape[0] == 0 or mean.shape[1] == 0 or mean.shape[0] % G != 0:
        raise ValueError(f"posterior_groups: {mean.shape[0]} rows of {mean.shape[1]} do not split into {G} non-empty groups (kl is a mean)")
    return _PosteriorGroupsFn.apply(mean, logvar, eps.contiguous(), G)
