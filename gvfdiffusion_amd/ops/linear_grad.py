"""A projection y = x W^T + b that trains on this library's own matrix kernels (include/gvf_linear_grad.h, csrc/linear_grad.hip):

  cast_transpose   one pass over the fp32 master weight [N, K] -> the 16-bit image [N, K] the forward reads and its transpose [K, N] the input
                   gradient reads.
  wgrad            dW = dy^T x and db = column sums of dy: 16-bit operands, fp32 accumulation, fp32 results (no 16-bit weight gradient).
  linear           the torch.autograd.Function over the fp32 master weight and bias: forward gvf_gemm on the image, backward gvf_gemm on the
                   transposed image (only if x needs a gradient) and wgrad (only if the weight or the bias does).

Deterministic: the weight gradient's split over the rows is reduced in a fixed order, no atomics.  There is no CPU fallback and no other GEMM to
fall back to: K % 32 != 0 or N % 32 != 0 (the contraction constraints of the forward and of the input gradient) raise ValueError."""
import ctypes

import torch

from .. import _lib
from . import _util, dit_ops
from ._util import ptr as _p

_vp, _i, _sz = ctypes.c_void_p, ctypes.c_int, ctypes.c_size_t

_lib.register({
    "gvf_cast_transpose": (_i, [_i, _vp, _i, _vp, _i, _vp, _i, _i, _i, _vp]),
    "gvf_gemm_wgrad_splits": (_i, [_i, _i, _i]),
    "gvf_gemm_wgrad_workspace_bytes": (_i, [_i, _i, _i, _i, ctypes.POINTER(_sz)]),
    "gvf_gemm_wgrad": (_i, [_i, _vp, _i, _vp, _i, _i, _i, _i, _vp, _i, _vp, _vp, _sz, _i, _vp]),
})


def _pad8(n: int) -> int:
    return (n + 7) // 8 * 8


def cast_transpose(w, dtype=torch.bfloat16, out=None):
    """w fp32 [N, K] (unit column stride, any row stride) -> (w16 [N, K], w16t [K, N]) in `dtype`, rounded to nearest even as Tensor.to rounds.
    The images' rows are padded to a multiple of 8 elements (zeros) and returned as views of their first K / N columns; out = (buf16, buf16t):
    2-D 16-bit tensors [N, ld_k >= K] / [K, ld_n >= N] of unit column stride to write into (their row strides are the leading dimensions)."""
    _lib.require_cuda(w)
    dt = dit_ops.dt_code(dtype)
    if w.dim() != 2 or w.dtype != torch.float32 or w.numel() == 0:
        raise ValueError(f"cast_transpose: w must be a non-empty fp32 [N, K] matrix, got {w.dtype} {tuple(w.shape)}")
    if w.stride(1) != 1:
        w = w.contiguous()
    N, K = w.shape
    if out is None:
        w16 = torch.empty((N, _pad8(K)), dtype=dtype, device=w.device)
        w16t = torch.empty((K, _pad8(N)), dtype=dtype, device=w.device)
    else:
        w16, w16t = out
        _lib.require_cuda(w16, w16t)
        for t, (r, c) in ((w16, (N, K)), (w16t, (K, N))):
            if t.dtype != dtype or t.dim() != 2 or t.shape[0] != r or t.shape[1] < c or t.stride(1) != 1:
                raise ValueError(f"cast_transpose: an output image must be {dtype} [{r}, >= {c}] with unit column stride, got {t.dtype} {tuple(t.shape)}")
    ld_k = w16.stride(0) if N > 1 else w16.shape[1]
    ld_n = w16t.stride(0) if K > 1 else w16t.shape[1]
    _lib.check(_lib.lib().gvf_cast_transpose(dt, _p(w), w.stride(0) if N > 1 else K, _p(w16), ld_k, _p(w16t), ld_n, N, K,
                                             _lib.current_stream(w.device)), "gvf_cast_transpose")
    return w16[:, :K], w16t[:, :N]


def wgrad_splits(M: int, N: int, K: int) -> int:
    """The split count wgrad(splits=0) uses: a function of the three extents only."""
    s = _lib.lib().gvf_gemm_wgrad_splits(M, N, K)
    if s < 1:
        _lib.check(s, "gvf_gemm_wgrad_splits")
    return s


def wgrad_workspace_bytes(M: int, N: int, K: int, splits: int = 0) -> int:
    return _util.workspace_bytes("gvf_gemm_wgrad_workspace_bytes", M, N, K, splits)


def _rows2d(t, name):
    if t.dim() != 2:
        raise ValueError(f"wgrad: {name} must be a 2-D tensor, got {tuple(t.shape)}")
    t = _util.rows16(t)
    return t, (t.stride(0) if t.shape[0] > 1 else t.shape[1])


def wgrad(dy, x, bias=True, splits=0, out=None, out_bias=None, workspace=None):
    """dy [M, N], x [M, K] of one 16-bit type (row-strided views are read in place) -> (dW fp32 [N, K], db fp32 [N] or None): dW = dy^T x,
    db = dy.sum(0), accumulated in fp32.  N and K multiples of 8.  splits: over how many groups of rows the sum is split (0 = wgrad_splits);
    out / out_bias / workspace: caller-owned results (dW may be a row-strided view) and scratch (uint8, at least wgrad_workspace_bytes)."""
    _lib.require_cuda(dy, x, out, out_bias, workspace)
    dt = dit_ops._same_lp(dy, x)
    dy, ldy = _rows2d(dy, "dy")
    x, ldx = _rows2d(x, "x")
    M, N = dy.shape
    K = x.shape[1]
    if x.shape[0] != M or N % 8 != 0 or K % 8 != 0 or N == 0 or K == 0:
        raise ValueError(f"wgrad: dy [M, N] and x [M, K] with N and K positive multiples of 8, got {tuple(dy.shape)} / {tuple(x.shape)}")
    dev = dy.device
    dw = torch.empty((N, K), dtype=torch.float32, device=dev) if out is None else out
    if dw.dtype != torch.float32 or tuple(dw.shape) != (N, K) or dw.stride(1) != 1:
        raise ValueError(f"wgrad: out must be fp32 [{N}, {K}] with unit column stride")
    db = None
    if bias:
        db = torch.empty(N, dtype=torch.float32, device=dev) if out_bias is None else out_bias
        if db.dtype != torch.float32 or tuple(db.shape) != (N,) or not db.is_contiguous():
            raise ValueError(f"wgrad: out_bias must be a contiguous fp32 [{N}]")
    if M == 0:                                               # (an empty operand has no address to hand over)
        dw.zero_()
        if db is not None:
            db.zero_()
        return dw, db
    if workspace is None:
        workspace = _util.scratch("gvf_gemm_wgrad_workspace_bytes", dev, M, N, K, splits)
    _lib.check(_lib.lib().gvf_gemm_wgrad(dt, _p(dy), ldy, _p(x), ldx, M, N, K, _p(dw), dw.stride(0) if N > 1 else K, _p(db), _p(workspace),
                                         workspace.numel() * workspace.element_size(), int(splits), _lib.current_stream(dev)), "gvf_gemm_wgrad")
    return dw, db


class _LinearFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x2, weight, bias, w16, w16t):
        M, N = x2.shape[0], weight.shape[0]
        y = torch.empty((M, N), dtype=x2.dtype, device=x2.device)
        if M > 0:
            dit_ops.gemm(x2, w16, bias, y, dit_ops.EPI_STORE_16)
        ctx.save_for_backward(x2, w16t)
        ctx.has_bias = bias is not None
        return y

    @staticmethod
    def backward(ctx, dy):
        x2, w16t = ctx.saved_tensors
        M, K = x2.shape
        need = ctx.needs_input_grad
        if dy.dtype != x2.dtype:
            dy = dy.to(x2.dtype)
        if not dy.is_contiguous():
            dy = dy.contiguous()
        dx = dw = db = None
        if need[0]:
            dx = torch.empty((M, K), dtype=x2.dtype, device=x2.device)
            if M > 0:
                dit_ops.gemm(dy, w16t, None, dx, dit_ops.EPI_STORE_16)
        want_db = ctx.has_bias and need[2]
        if need[1] or want_db:
            dw, db = wgrad(dy, x2, bias=want_db)
        return dx, (dw if need[1] else None), db, None, None


def linear(x, weight, bias=None, dtype=torch.bfloat16, cache=None):
    """y = x weight^T + bias in `dtype` (fp16 / bf16): x [..., K] in `dtype`, weight fp32 [N, K] and bias fp32 [N] the master parameters, whose
    gradients arrive in fp32 straight from the weight-gradient kernel.  The weight is cast once per call -- or once per `cache` (a dict keyed by
    the weight tensor, holding both 16-bit images): hand the same dict to every use of a step, and a recomputed forward reads the same images."""
    _lib.require_cuda(x, weight, bias)
    dit_ops.dt_code(dtype)
    if weight.dim() != 2 or weight.dtype != torch.float32 or (bias is not None and (bias.dtype != torch.float32 or bias.shape != (weight.shape[0],))):
        raise ValueError(f"linear: weight must be the fp32 [N, K] master and bias fp32 [N], got {weight.dtype} {tuple(weight.shape)}")
    N, K = weight.shape
    if K % 32 != 0 or N % 32 != 0:
        raise ValueError(f"linear: N = {N} and K = {K} must be multiples of 32 (the contraction of the forward and of the input gradient); "
                         "there is no fallback")
    if x.dtype != dtype or x.dim() < 1 or x.shape[-1] != K:
        raise ValueError(f"linear: x must be {dtype} [..., {K}], got {x.dtype} {tuple(x.shape)}")
    images = None if cache is None else cache.get(weight)
    if images is None:
        with torch.no_grad():
            images = cast_transpose(weight, dtype)
        if cache is not None:
            cache[weight] = images
    x2 = x.reshape(-1, K)
    if not x2.is_contiguous():
        x2 = x2.contiguous()
    if bias is not None and not bias.is_contiguous():
        bias = bias.contiguous()
    return _LinearFn.apply(x2, weight, bias, images[0], images[1]).view(x.shape[:-1] + (N,))
