"""The operators of the static VAE's training path that are not matrix products, as torch.autograd.Functions on the HIP kernels of
include/gvf_sparse_train.h (csrc/sparse_train.hip):

  gelu_tanh      tanh-GELU on a 16-bit tensor (the output of mlp.0), fp32 inside; the backward recomputes g'(u) from the saved u.
  gather_rows    out[i] = x[index[i]] over the rows of a 2-D tensor: the window-order gather of the packed qkv rows, the scatter back, and --
                 given the inverse permutation -- both gradients, all on one kernel and without atomics.
  posterior      (z, kl) = (mean + exp(0.5 logvar) eps, 0.5 mean(mean^2 + exp(logvar) - logvar - 1)) from h = [mean | logvar].
  gaussian_reg   (vol, opa): the volume and opacity regularisers on the raw scaling / opacity tensors of a GaussianModel.
  bias_grad_tap  the bias gradient of a projection that closes a sub-layer as fp32 column sums (colsum) of the stream's gradient.

The scalars are deterministic: double-precision partials per workgroup, added in a fixed order.  There is no CPU fallback."""
import ctypes

import torch

from .. import _lib
from . import dit_ops
from ._util import psz as _psz, ptr as _p, rows16 as _rows16, scratch as _scratch

_vp, _i, _i64, _sz, _f = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64, ctypes.c_size_t, ctypes.c_float

_lib.register({
    "gvf_gelu_tanh_fwd": (_i, [_i, _vp, _vp, _i64, _vp]),
    "gvf_gelu_tanh_bwd": (_i, [_i, _vp, _vp, _vp, _i64, _vp]),
    "gvf_gather_rows": (_i, [_vp, _i64, _vp, _vp, _i64, _i64, _vp]),
    "gvf_posterior_workspace_bytes": (_i, [_i64, _i, _psz]),
    "gvf_posterior_fwd": (_i, [_vp, _i64, _vp, _vp, _vp, _i64, _i, _vp, _sz, _vp]),
    "gvf_posterior_bwd": (_i, [_vp, _i64, _vp, _vp, _vp, _vp, _i64, _i64, _i, _vp]),
    "gvf_gaussian_reg_workspace_bytes": (_i, [_i64, _psz]),
    "gvf_gaussian_reg_fwd": (_i, [_vp, _vp, _i64, _f, _f, _f, _i, _vp, _vp, _vp, _sz, _vp]),
    "gvf_gaussian_reg_bwd": (_i, [_vp, _vp, _i64, _f, _f, _f, _i, _vp, _vp, _vp, _vp, _vp]),
    "gvf_colsum_f32_workspace_bytes": (_i, [_i64, _i, _psz]),
    "gvf_colsum_f32": (_i, [_vp, _i64, _i, _vp, _vp, _sz, _vp]),
})

ACTIVATIONS = {"exp": 0, "softplus": 1}


# ---- tanh-GELU ----------------------------------------------------------------------------------------------------------------------------
class _GeluTanhFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, u):
        a = torch.empty_like(u)
        if u.numel() > 0:
            _lib.check(_lib.lib().gvf_gelu_tanh_fwd(dit_ops.dt_code(u.dtype), _p(u), _p(a), u.numel(), _lib.current_stream(u.device)), "gvf_gelu_tanh_fwd")
        ctx.save_for_backward(u)
        return a

    @staticmethod
    def backward(ctx, da):
        u, = ctx.saved_tensors
        if da.dtype != u.dtype:
            da = da.to(u.dtype)
        if not da.is_contiguous():
            da = da.contiguous()
        du = torch.empty_like(u)
        if u.numel() > 0:
            _lib.check(_lib.lib().gvf_gelu_tanh_bwd(dit_ops.dt_code(u.dtype), _p(u), _p(da), _p(du), u.numel(), _lib.current_stream(u.device)),
                       "gvf_gelu_tanh_bwd")
        return du


def gelu_tanh(u):
    """a = 0.5 u (1 + tanh(sqrt(2 / pi) (u + 0.044715 u^3))) on an fp16 / bf16 tensor of any shape, fp32 inside, rounded once; differentiable
    in u.  Finite for every finite u, in both directions."""
    _lib.require_cuda(u)
    dit_ops.dt_code(u.dtype)
    return _GeluTanhFn.apply(u.contiguous())


# ---- a closing projection's bias gradient ------------------------------------------------------------------------------------------------
def colsum(x):
    """fp32 [rows, C] -> fp32 [C] column sums, accumulated in double in a fixed order (no gradient of its own)."""
    _lib.require_cuda(x)
    if x.dim() != 2 or x.dtype != torch.float32 or x.shape[0] == 0 or x.shape[1] == 0:
        raise ValueError(f"colsum: x must be a non-empty fp32 [rows, C] tensor, got {x.dtype} {tuple(x.shape)}")
    x = x.contiguous()
    out = torch.empty(x.shape[1], dtype=torch.float32, device=x.device)
    ws = _scratch("gvf_colsum_f32_workspace_bytes", x.device, x.shape[0], x.shape[1])
    _lib.check(_lib.lib().gvf_colsum_f32(_p(x), x.shape[0], x.shape[1], _p(out), _p(ws), ws.numel(), _lib.current_stream(x.device)), "gvf_colsum_f32")
    return out


class _BiasGradTapFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, out, bias):
        return out.view_as(out)

    @staticmethod
    def backward(ctx, dout):
        need = ctx.needs_input_grad
        return dout, (colsum(dout.reshape(-1, dout.shape[-1]).float()) if need[1] else None)


def bias_grad_tap(out, bias):
    """out = x + (h W^T + bias) on the fp32 stream, computed with `bias` DETACHED inside the projection: returns out unchanged and gives `bias`
    its gradient as the fp32 column sums of out's incoming gradient -- before gate_residual rounds that gradient to the 16-bit operand of the
    weight-gradient product, whose own column sums would carry that rounding into a gradient no 16-bit value needs to touch."""
    _lib.require_cuda(out, bias)
    if out.dtype != torch.float32 or bias.dim() != 1 or bias.shape[0] != out.shape[-1]:
        raise ValueError(f"bias_grad_tap: out must be fp32 [..., C] and bias [C], got {out.dtype} {tuple(out.shape)} / {tuple(bias.shape)}")
    return _BiasGradTapFn.apply(out, bias)


# ---- row gather ---------------------------------------------------------------------------------------------------------------------------
def _gather_launch(x, index, out):
    """x [R, W] (unit column stride, 16-byte rows), index int64 [rows], out contiguous [rows, W]"""
    rows, es = index.numel(), x.element_size()
    if rows > 0:
        _lib.check(_lib.lib().gvf_gather_rows(_p(x), (x.stride(0) if x.shape[0] > 1 else x.shape[1]) * es, _p(index), _p(out), rows, x.shape[1] * es,
                                              _lib.current_stream(x.device)), "gvf_gather_rows")
    return out


class _GatherRowsFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, index, inverse):
        out = torch.empty((index.numel(), x.shape[1]), dtype=x.dtype, device=x.device)
        _gather_launch(_rows16(x), index, out)
        ctx.save_for_backward(index if inverse is None else inverse)
        ctx.permutation, ctx.src_rows = inverse is not None, x.shape[0]
        return out

    @staticmethod
    def backward(ctx, dy):
        idx, = ctx.saved_tensors
        if ctx.permutation:                                   # dx[j] = dy[inverse[j]]: the same kernel
            dx = torch.empty((ctx.src_rows, dy.shape[1]), dtype=dy.dtype, device=dy.device)
            return _gather_launch(_rows16(dy), idx, dx), None, None
        dx = torch.zeros((ctx.src_rows, dy.shape[1]), dtype=dy.dtype, device=dy.device)
        return dx.index_add_(0, idx, dy), None, None       # torch's indexing: an index with repeats (several serialized windows)


def gather_rows(x, index, inverse=None):
    """out[i, :] = x[index[i], :] for a 2-D x (fp16 / bf16 / fp32; rows of a multiple of 16 bytes; a column slice of a wider matrix is read in
    place) and an int64 device index [rows].  Differentiable in x: with `inverse` given, `index` is a permutation of x's rows and `inverse` its
    inverse (index[inverse[j]] == j), and the gradient is gather_rows(dy, inverse) on the same kernel; without it the gradient is torch's
    index_add_ (an index that repeats or omits rows).
    The index values are a PRECONDITION (0 <= index[i] < x.shape[0]) and are not checked: checking would read the device from the host."""
    _lib.require_cuda(x, index, inverse)
    if x.dim() != 2 or x.dtype not in (torch.float16, torch.bfloat16, torch.float32):
        raise ValueError(f"gather_rows: x must be a 2-D fp16 / bf16 / fp32 tensor, got {x.dtype} {tuple(x.shape)}")
    if (x.shape[1] * x.element_size()) % 16 != 0 or x.shape[1] == 0:
        raise ValueError(f"gather_rows: rows of {x.shape[1] * x.element_size()} bytes (a positive multiple of 16 is built; there is no fallback)")
    for name, t in (("index", index), ("inverse", inverse)):
        if t is not None and (t.dtype != torch.int64 or t.dim() != 1):
            raise ValueError(f"gather_rows: {name} must be a 1-D int64 tensor, got {t.dtype} {tuple(t.shape)}")
    if inverse is not None and (index.numel() != x.shape[0] or inverse.numel() != x.shape[0]):
        raise ValueError(f"gather_rows: a permutation of {x.shape[0]} rows has {x.shape[0]} entries, got {index.numel()} / {inverse.numel()}")
    if index.numel() > 0 and x.shape[0] == 0:
        raise ValueError("gather_rows: rows requested from an empty tensor")
    return _GatherRowsFn.apply(x, index.contiguous(), None if inverse is None else inverse.contiguous())


# ---- posterior ----------------------------------------------------------------------------------------------------------------------------
def _h_view(h):
    if h.stride(1) != 1 or (h.shape[0] > 1 and h.stride(0) < h.shape[1]):
        h = h.contiguous()
    return h, (h.stride(0) if h.shape[0] > 1 else h.shape[1])


class _PosteriorFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, h, eps):
        T, L = eps.shape
        hv, ldh = _h_view(h)
        dev = h.device
        z = torch.empty((T, L), dtype=torch.float32, device=dev)
        kl = torch.empty((), dtype=torch.float32, device=dev)
        ws = _scratch("gvf_posterior_workspace_bytes", dev, T, L)
        _lib.check(_lib.lib().gvf_posterior_fwd(_p(hv), ldh, _p(eps), _p(z), _p(kl), T, L, _p(ws), ws.numel(), _lib.current_stream(dev)), "gvf_posterior_fwd")
        ctx.save_for_backward(hv, eps)
        ctx.ldh = ldh
        ctx.set_materialize_grads(False)
        return z, kl

    @staticmethod
    def backward(ctx, dz, dkl):
        hv, eps = ctx.saved_tensors
        T, L = eps.shape
        if dz is None and dkl is None:
            return None, None
        if dz is not None and (dz.dtype != torch.float32 or not dz.is_contiguous()):
            dz = dz.float().contiguous()
        if dkl is not None:
            dkl = dkl.float().reshape(()).contiguous()
        dh = torch.empty((T, 2 * L), dtype=torch.float32, device=hv.device)
        _lib.check(_lib.lib().gvf_posterior_bwd(_p(hv), ctx.ldh, _p(eps), _p(dz), _p(dkl), _p(dh), 2 * L, T, L, _lib.current_stream(hv.device)),
                   "gvf_posterior_bwd")
        return dh, None


def posterior(h, eps):
    """h fp32 [T, 2L] = [mean | logvar] (unit column stride, any row stride), eps fp32 [T, L] (the noise) ->
    (z fp32 [T, L] = mean + exp(0.5 logvar) eps,  kl = 0.5 mean(mean^2 + exp(logvar) - logvar - 1) as a 0-d fp32 tensor).
    Differentiable in h through both outputs, in one backward launch."""
    _lib.require_cuda(h, eps)
    if h.dim() != 2 or eps.dim() != 2 or h.dtype != torch.float32 or eps.dtype != torch.float32 or h.shape[0] != eps.shape[0] or \
            h.shape[1] != 2 * eps.shape[1] or eps.shape[1] == 0:
        raise ValueError(f"posterior: h must be fp32 [T, 2L] and eps fp32 [T, L], got {h.dtype} {tuple(h.shape)} / {eps.dtype} {tuple(eps.shape)}")
    if h.shape[0] == 0:
        raise ValueError("posterior: no rows (the KL term is a mean over nothing)")
    return _PosteriorFn.apply(h, eps.contiguous())


# ---- regularisers -------------------------------------------------------------------------------------------------------------------------
class _GaussianRegFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, scaling, opacity, bs, bo, kappa, act):
        N, dev = scaling.shape[0], scaling.device
        out = torch.empty(2, dtype=torch.float32, device=dev)
        ws = _scratch("gvf_gaussian_reg_workspace_bytes", dev, N)
        _lib.check(_lib.lib().gvf_gaussian_reg_fwd(_p(scaling), _p(opacity), N, bs, bo, kappa, act, _p(out[0:]), _p(out[1:]), _p(ws), ws.numel(),
                                                   _lib.current_stream(dev)), "gvf_gaussian_reg_fwd")
        ctx.save_for_backward(scaling, opacity)
        ctx.consts = (bs, bo, kappa, act)
        ctx.set_materialize_grads(False)
        return out[0], out[1]

    @staticmethod
    def backward(ctx, dvol, dopa):
        scaling, opacity = ctx.saved_tensors
        need = ctx.needs_input_grad
        if dvol is not None and not need[0]:
            dvol = None
        if dopa is not None and not need[1]:
            dopa = None
        if dvol is None and dopa is None:
            return (None,) * 6
        dvol = None if dvol is None else dvol.float().reshape(()).contiguous()
        dopa = None if dopa is None else dopa.float().reshape(()).contiguous()
        ds = torch.empty_like(scaling) if dvol is not None else None
        do = torch.empty_like(opacity) if dopa is not None else None
        _lib.check(_lib.lib().gvf_gaussian_reg_bwd(_p(scaling), _p(opacity), scaling.shape[0], *ctx.consts, _p(dvol), _p(dopa), _p(ds), _p(do),
                                                   _lib.current_stream(scaling.device)), "gvf_gaussian_reg_bwd")
        return ds, do, None, None, None, None


def gaussian_reg(scaling, opacity, scale_bias, opacity_bias, min_kernel_size=0.0, activation="exp"):
    """The regularisers of sparse_vae.py:229-249 on the RAW tensors of a GaussianModel (`_scaling` fp32 [N, 3], `_opacity` fp32 [N, 1] or [N],
    both already lr-scaled) and its constants (scale_bias / opacity_bias: the model's inverse-activated biases; min_kernel_size; activation
    "exp" or "softplus", torch's softplus with its threshold of 20):
        vol = mean_i prod_k sqrt(act(s_ik + scale_bias)^2 + min_kernel_size^2),   opa = mean_i (sigmoid(o_i + opacity_bias) - 1)^2
    -> (vol, opa), 0-d fp32 tensors, differentiable in scaling and opacity."""
    _lib.require_cuda(scaling, opacity)
    if activation not in ACTIVATIONS:
        raise ValueError(f"gaussian_reg: activation must be one of {tuple(ACTIVATIONS)}, got {activation!r}")
    if scaling.dim() != 2 or scaling.shape[1] != 3 or scaling.dtype != torch.float32 or opacity.dtype != torch.float32 or \
            opacity.numel() != scaling.shape[0] or opacity.dim() not in (1, 2):
        raise ValueError(f"gaussian_reg: scaling must be fp32 [N, 3] and opacity fp32 [N, 1], got {scaling.dtype} {tuple(scaling.shape)} / "
                         f"{opacity.dtype} {tuple(opacity.shape)}")
    if scaling.shape[0] == 0:
        raise ValueError("gaussian_reg: no Gaussians (the regularisers are means over nothing)")
    if not float(min_kernel_size) >= 0.0:
        raise ValueError(f"gaussian_reg: min_kernel_size must not be negative, got {min_kernel_size}")
    return _GaussianRegFn.apply(scaling.contiguous(), opacity.contiguous(), float(scale_bias), float(opacity_bias), float(min_kernel_size),
                                ACTIVATIONS[activation])
