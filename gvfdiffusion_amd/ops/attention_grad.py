"""Differentiable attention (include/gvf_attn_bwd.h, csrc/attn_bwd.hip): softmax(q k^T * scale) v on [N, L, H, C] fp16 / bf16 tensors as
a torch.autograd.Function.  The forward is the inference kernel (dit_ops.attention), so the output under grad is bit-identical to the
no-grad output; the backward recomputes the probabilities from q, k and a row log-sum-exp of its own and is deterministic.  head_dim 32
and 64; no mask, no dropout; there is no CPU fallback."""
import ctypes

import torch

from .. import _lib
from . import dit_ops

_vp, _i, _i64, _sz, _f = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64, ctypes.c_size_t, ctypes.c_float

_lib.register({
    "gvf_attn_bwd_workspace_bytes": (_i, [_i, _i, _i, _i, _i, _i, ctypes.POINTER(_sz)]),
    "gvf_attn_bwd": (_i, [_i] + [_vp] * 8 + [_i] * 6 + [ctypes.POINTER(_i64)] * 8 + [_f, _vp, _sz, _vp]),
})


def _st(t):
    """(outer, inner, seq, head) strides in elements of an [N, L, H, C] tensor."""
    return (t.stride(0), 0, t.stride(1), t.stride(2))


def _s4(t):
    return (_i64 * 4)(*(int(s) for s in _st(t)))


def _layout(t):
    """Heads packed and channels contiguous, 16-byte rows: what the kernels address through their four strides; else a copy."""
    C = t.shape[3]
    ok = t.stride(3) == 1 and t.stride(2) == C and t.stride(0) % 8 == 0 and t.stride(1) % 8 == 0 and t.data_ptr() % 16 == 0
    return t if ok else t.contiguous()


def workspace_bytes(N: int, Lq: int, Lk: int, H: int, C: int) -> int:
    nb = ctypes.c_size_t(0)
    _lib.check(_lib.lib().gvf_attn_bwd_workspace_bytes(N, 1, Lq, Lk, H, C, ctypes.byref(nb)), "gvf_attn_bwd_workspace_bytes")
    return int(nb.value)


def attention_backward(q, k, v, out, dout, scale: float):
    """dq, dk, dv (contiguous, in the operand type) of out = softmax(q k^T * scale) v; every tensor [N, L, H, C]."""
    _lib.require_cuda(q, k, v, out, dout)
    dt = dit_ops._same_lp(q, k, v, out, dout)
    N, Lq, H, C = q.shape
    Lk = k.shape[1]
    dq, dk, dv = torch.empty_like(q, memory_format=torch.contiguous_format), torch.empty_like(k, memory_format=torch.contiguous_format), \
        torch.empty_like(v, memory_format=torch.contiguous_format)
    if N == 0 or Lq == 0 or Lk == 0 or H == 0:          # nothing attends to anything: zero gradients, no launch
        return dq.zero_(), dk.zero_(), dv.zero_()
    q, k, v, out, dout = (_layout(t) for t in (q, k, v, out, dout))
    ws = torch.empty(workspace_bytes(N, Lq, Lk, H, C), dtype=torch.uint8, device=q.device)
    _lib.check(_lib.lib().gvf_attn_bwd(dt, _lib.ptr(q), _lib.ptr(k), _lib.ptr(v), _lib.ptr(out), _lib.ptr(dout), _lib.ptr(dq), _lib.ptr(dk),
                                       _lib.ptr(dv), N, 1, Lq, Lk, H, C, _s4(q), _s4(k), _s4(v), _s4(out), _s4(dout), _s4(dq), _s4(dk), _s4(dv),
                                       float(scale), _lib.ptr(ws), ws.numel(), _lib.current_stream(q.device)), "gvf_attn_bwd")
    return dq, dk, dv


class _AttentionFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, q, k, v, scale):
        N, Lq, H, C = q.shape
        Lk = k.shape[1]
        q, k, v = (_layout(t) for t in (q, k, v))
        out = torch.empty((N, Lq, H, C), dtype=q.dtype, device=q.device)
        if Lk == 0:
            out.zero_()                                  # zero rows for an empty key range, as the varlen forward writes
        elif N > 0 and Lq > 0:
            dit_ops.attention(q, k, v, out, N, 1, Lq, Lk, H, _st(q), _st(k), _st(v), _st(out), scale=scale, head_dim=C)
        ctx.save_for_backward(q, k, v, out)
        ctx.scale = scale
        return out

    @staticmethod
    def backward(ctx, dout):
        q, k, v, out = ctx.saved_tensors
        dq, dk, dv = attention_backward(q, k, v, out, dout, ctx.scale)
        need = ctx.needs_input_grad
        return (dq if need[0] else None, dk if need[1] else None, dv if need[2] else None, None)


def attention(q, k, v, scale=None):
    """softmax(q k^T * scale) v for q [N, Lq, H, C], k, v [N, Lk, H, C] in fp16 or bf16 (C 32 or 64; scale defaults to C ** -0.5),
    differentiable in q, k and v.  Strided views (the unbind slices of a packed projection) are read in place."""
    for name, t in (("q", q), ("k", k), ("v", v)):
        if not isinstance(t, torch.Tensor) or t.dim() != 4:
            raise ValueError(f"attention: {name} must be an [N, L, H, C] tensor")
    _lib.require_cuda(q, k, v)
    dit_ops._same_lp(q, k, v)
    if not (q.dtype == k.dtype == v.dtype):
        raise _lib.GvfError(f"attention: q, k, v must share one 16-bit type, got {q.dtype}, {k.dtype}, {v.dtype}")
    N, Lq, H, C = q.shape
    if C not in (32, 64):
        raise NotImplementedError(f"attention: head_dim {C} (32 and 64 are built)")
    if k.shape != v.shape or k.shape[0] != N or k.shape[2] != H or k.shape[3] != C:
        raise ValueError(f"attention: q {tuple(q.shape)}, k {tuple(k.shape)}, v {tuple(v.shape)} do not fit")
    scale = C ** -0.5 if scale is None else float(scale)
    if not scale > 0.0:
        raise ValueError(f"attention: scale must be positive, got {scale}")
    return _AttentionFn.apply(q, k, v, scale)
