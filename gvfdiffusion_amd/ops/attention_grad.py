"""Differentiable attention (include/gvf_attn_bwd.h, csrc/attn_bwd.hip): softmax(q k^T * scale) v on [N, L, H, C] fp16 / bf16 tensors as
a torch.autograd.Function.  The forward is the inference kernel (dit_ops.attention), so the output under grad is bit-identical to the
no-grad output; the backward recomputes the probabilities from q, k and a row log-sum-exp of its own and is deterministic.  head_dim 32
and 64; no mask, no dropout; there is no CPU fallback.

attention_varlen is the ragged form over packed [T, H, C] token lists with device cu_seqlens (the seam sparse/attention/full_attn.py): forward
dit_ops.attention_varlen without gains, backward gvf_attn_varlen_bwd.  No sequence length is read back from the device."""
import ctypes

import torch

from .. import _lib
from . import _util, dit_ops

_vp, _i, _i64, _sz, _f, _ll = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64, ctypes.c_size_t, ctypes.c_float, ctypes.c_longlong

_lib.register({
    "gvf_attn_bwd_workspace_bytes": (_i, [_i, _i, _i, _i, _i, _i, ctypes.POINTER(_sz)]),
    "gvf_attn_bwd": (_i, [_i] + [_vp] * 8 + [_i] * 6 + [ctypes.POINTER(_i64)] * 8 + [_f, _vp, _sz, _vp]),
    "gvf_attn_varlen_bwd_workspace_bytes": (_i, [_i, _ll, _ll, _i, _i, _i, _i, ctypes.POINTER(_sz)]),
    "gvf_attn_varlen_bwd": (_i, [_i] + [_vp] * 8 + [_i, _vp, _vp, _ll, _ll] + [_i] * 4 + [ctypes.POINTER(_i64)] * 8 + [_f, _vp, _sz, _vp]),
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
    return _util.workspace_bytes("gvf_attn_bwd_workspace_bytes", N, 1, Lq, Lk, H, C)


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
    ws = _util.scratch("gvf_attn_bwd_workspace_bytes", q.device, N, 1, Lq, Lk, H, C)
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


# ---- the ragged form: packed [T, H, C] token lists, device cu_seqlens -------------------------------------------------------------------
def _st3(t):
    """(outer, inner, seq, head) strides in elements of a packed [T, H, C] tensor."""
    return (0, 0, t.stride(0), t.stride(1))


def _s43(t):
    return (_i64 * 4)(*(int(s) for s in _st3(t)))


def _layout3(t):
    """Channels contiguous, rows and heads on 16-byte boundaries: what the kernels address through their strides (the unbind slices of a
    packed projection in either channel layout); else a copy."""
    ok = t.stride(2) == 1 and t.stride(0) % 8 == 0 and t.stride(1) % 8 == 0 and t.data_ptr() % 16 == 0
    return t if ok else t.contiguous()


def _check_cu(cu_q, cu_k):
    _lib.require_cuda(cu_q, cu_k)
    if cu_q.dtype != torch.int32 or cu_k.dtype != torch.int32 or cu_q.dim() != 1 or cu_q.shape != cu_k.shape or cu_q.numel() < 2:
        raise ValueError(f"attention_varlen: cu_q and cu_k must be int32 [n_seqs + 1] device tensors, got {cu_q.dtype} {tuple(cu_q.shape)} / "
                         f"{cu_k.dtype} {tuple(cu_k.shape)}")
    return cu_q.contiguous(), cu_k.contiguous()


def varlen_workspace_bytes(n_seqs: int, total_q: int, total_k: int, max_Lq: int, max_Lk: int, H: int, C: int) -> int:
    return _util.workspace_bytes("gvf_attn_varlen_bwd_workspace_bytes", n_seqs, total_q, total_k, max_Lq, max_Lk, H, C)


def attention_varlen_backward(q, k, v, out, dout, cu_q, cu_k, max_Lq: int, max_Lk: int, scale: float, workspace=None, grads=None):
    """dq, dk, dv (contiguous, in the operand type) of the packed out = softmax(q k^T * scale) v per sequence: q, out, dout [Tq, H, C] follow
    cu_q, k, v [Tk, H, C] follow cu_k (int32 [n_seqs + 1] on the device, ending at Tq / Tk); max_Lq / max_Lk bound the sequence lengths.
    workspace: caller-owned scratch (uint8, at least varlen_workspace_bytes); grads = (dq, dk, dv): caller-owned results of the operands'
    shapes and type (channels contiguous, rows and heads on 8-byte boundaries)."""
    _lib.require_cuda(q, k, v, out, dout, workspace, *(grads or ()))
    dt = dit_ops._same_lp(q, k, v, out, dout)
    cu_q, cu_k = _check_cu(cu_q, cu_k)
    Tq, H, C = q.shape
    Tk = k.shape[0]
    if out.shape != q.shape or dout.shape != q.shape or k.shape != v.shape or k.shape[1:] != q.shape[1:]:
        raise ValueError(f"attention_varlen_backward: q {tuple(q.shape)}, k {tuple(k.shape)}, v {tuple(v.shape)}, out {tuple(out.shape)}, "
                         f"dout {tuple(dout.shape)} do not fit")
    if grads is None:
        dq, dk, dv = (torch.empty(t.shape, dtype=t.dtype, device=t.device) for t in (q, k, v))
    else:
        dq, dk, dv = grads
        for g, t in ((dq, q), (dk, k), (dv, v)):
            if g.shape != t.shape or g.dtype != t.dtype or g.stride(2) != 1 or g.stride(0) % 4 or g.stride(1) % 4 or g.data_ptr() % 8:
                raise ValueError(f"attention_varlen_backward: a result must be {t.dtype} {tuple(t.shape)} with contiguous channels and 8-byte rows")
    if Tq == 0 or Tk == 0 or H == 0:                     # nothing attends to anything: zero gradients, no launch
        return dq.zero_(), dk.zero_(), dv.zero_()
    q, k, v, out, dout = (_layout3(t) for t in (q, k, v, out, dout))
    n_seqs = cu_q.numel() - 1
    if workspace is None:
        workspace = _util.scratch("gvf_attn_varlen_bwd_workspace_bytes", q.device, n_seqs, Tq, Tk, int(max_Lq), int(max_Lk), H, C)
    _lib.check(_lib.lib().gvf_attn_varlen_bwd(dt, _lib.ptr(q), _lib.ptr(k), _lib.ptr(v), _lib.ptr(out), _lib.ptr(dout), _lib.ptr(dq), _lib.ptr(dk),
                                              _lib.ptr(dv), n_seqs, _lib.ptr(cu_q), _lib.ptr(cu_k), Tq, Tk, int(max_Lq), int(max_Lk), H, C,
                                              _s43(q), _s43(k), _s43(v), _s43(out), _s43(dout), _s43(dq), _s43(dk), _s43(dv), float(scale),
                                              _lib.ptr(workspace), workspace.numel(), _lib.current_stream(q.device)), "gvf_attn_varlen_bwd")
    return dq, dk, dv


class _AttentionVarlenFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, q, k, v, cu_q, cu_k, max_Lq, max_Lk, scale):
        Tq, H, C = q.shape
        q, k, v = (_layout3(t) for t in (q, k, v))
        out = torch.empty((Tq, H, C), dtype=q.dtype, device=q.device)
        if k.shape[0] == 0:
            out.zero_()                                  # no keys at all: zero rows, as the kernel writes for one sequence without keys
        elif Tq > 0:
            dit_ops.attention_varlen(q, k, v, out, cu_q, cu_k, max_Lq, max_Lk, H, _st3(q), _st3(k), _st3(v), _st3(out), scale=scale, head_dim=C)
        ctx.save_for_backward(q, k, v, out, cu_q, cu_k)
        ctx.max_Lq, ctx.max_Lk, ctx.scale = max_Lq, max_Lk, scale
        return out

    @staticmethod
    def backward(ctx, dout):
        q, k, v, out, cu_q, cu_k = ctx.saved_tensors
        dq, dk, dv = attention_varlen_backward(q, k, v, out, dout, cu_q, cu_k, ctx.max_Lq, ctx.max_Lk, ctx.scale)
        need = ctx.needs_input_grad
        return (dq if need[0] else None, dk if need[1] else None, dv if need[2] else None, None, None, None, None, None)


def attention_varlen(q, k, v, cu_q, cu_k, max_Lq: int, max_Lk: int, scale=None):
    """Per-sequence softmax(q k^T * scale) v over packed token lists: q [Tq, H, C], k, v [Tk, H, C] in fp16 or bf16 (C 32 or 64; scale defaults
    to C ** -0.5), sequence s owning rows cu_q[s]:cu_q[s + 1] of q and cu_k[s]:cu_k[s + 1] of k, v (int32 device tensors [n_seqs + 1] that end
    at Tq / Tk); max_Lq / max_Lk are host-side bounds of the lengths.  Differentiable in q, k and v; strided views (the unbind slices of a
    packed projection) are read in place.  A sequence without keys gets zero output rows and zero dq; one without queries zero dk, dv."""
    for name, t in (("q", q), ("k", k), ("v", v)):
        if not isinstance(t, torch.Tensor) or t.dim() != 3:
            raise ValueError(f"attention_varlen: {name} must be a packed [T, H, C] tensor")
    _lib.require_cuda(q, k, v)
    dit_ops._same_lp(q, k, v)
    if not (q.dtype == k.dtype == v.dtype):
        raise _lib.GvfError(f"attention_varlen: q, k, v must share one 16-bit type, got {q.dtype}, {k.dtype}, {v.dtype}")
    Tq, H, C = q.shape
    if C not in (32, 64):
        raise NotImplementedError(f"attention_varlen: head_dim {C} (32 and 64 are built)")
    if k.shape != v.shape or k.shape[1] != H or k.shape[2] != C:
        raise ValueError(f"attention_varlen: q {tuple(q.shape)}, k {tuple(k.shape)}, v {tuple(v.shape)} do not fit")
    cu_q, cu_k = _check_cu(cu_q, cu_k)
    max_Lq, max_Lk = int(max_Lq), int(max_Lk)
    if max_Lq < 0 or max_Lk < 0 or (Tq > 0 and max_Lq < 1) or (k.shape[0] > 0 and max_Lk < 1):
        raise ValueError(f"attention_varlen: max_Lq = {max_Lq} / max_Lk = {max_Lk} cannot bound the sequences of {Tq} / {k.shape[0]} tokens")
    scale = C ** -0.5 if scale is None else float(scale)
    if not scale > 0.0:
        raise ValueError(f"attention_varlen: scale must be positive, got {scale}")
    return _AttentionVarlenFn.apply(q, k, v, cu_q, cu_k, max_Lq, max_Lk, scale)
