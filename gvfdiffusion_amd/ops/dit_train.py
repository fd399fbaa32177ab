"""The element-wise operators of a DiT block as torch.autograd.Functions on the HIP kernels of include/gvf_dit_train.h (csrc/dit_train.hip):

  layernorm_modulate   fp32 rows -> LayerNorm -> (affine | adaLN modulate) -> the 16-bit operand of the next projection.  The forward is the
                       inference kernel (dit_ops.layernorm_modulate), so the output under grad is bit-identical to the no-grad output.
  gate_residual        x + gate_g * h on the fp32 residual stream.
  rmsnorm_heads        MultiHeadRMSNorm of the q / k slices of a packed projection, read in place.

Gradients of per-sample vectors (shift, scale, gate: `chunk` views of the [B, 6C] / [B, 3C] modulation output, read in place through their row
stride) and of the gains are deterministic: per-workgroup partial sums added in a fixed order, no atomics.  There is no CPU fallback."""
import ctypes

import torch

from .. import _lib
from . import dit_ops
from ._util import psz as _psz, ptr as _p, scratch as _scratch

_vp, _i, _i64, _sz, _f = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64, ctypes.c_size_t, ctypes.c_float

_lib.register({
    "gvf_ln_mod_bwd_workspace_bytes": (_i, [_i, _i, _i, _psz]),
    "gvf_ln_mod_bwd": (_i, [_i, _vp, _vp, _vp, _vp, _i, _i, _f, _vp, _vp, _vp, _i, _i, _vp, _vp, _vp, _vp, _vp, _sz, _vp]),
    "gvf_gate_residual_fwd": (_i, [_i, _vp, _vp, _vp, _i, _i, _vp, _i, _i, _vp]),
    "gvf_gate_residual_bwd_workspace_bytes": (_i, [_i, _i, _i, _psz]),
    "gvf_gate_residual_bwd": (_i, [_i, _vp, _vp, _vp, _i, _i, _vp, _vp, _i, _i, _vp, _sz, _vp]),
    "gvf_rmsnorm_heads_fwd": (_i, [_i, _vp, _i64, _vp, _vp, _i64, _i, _i, _i, _vp]),
    "gvf_rmsnorm_heads_bwd_workspace_bytes": (_i, [_i, _i, _i, _psz]),
    "gvf_rmsnorm_heads_bwd": (_i, [_i, _vp, _i64, _vp, _i64, _vp, _vp, _i64, _vp, _i, _i, _i, _vp, _sz, _vp]),
})


def _table_view(t, name, G, C):
    """A per-group vector as the kernels read it: [G, C] fp32, unit column stride, any row stride (a `chunk` view of the modulation output)."""
    if t.dim() != 2 or t.shape != (G, C) or t.dtype != torch.float32:
        raise ValueError(f"{name} must be a [{G}, {C}] fp32 tensor (or a column-slice view of one), got {tuple(t.shape)} {t.dtype}")
    if t.stride(1) != 1 or (G > 1 and (t.stride(0) < C or t.stride(0) % 4 != 0)) or t.data_ptr() % 16 != 0:
        t = t.contiguous()                                   # (what the 16-byte loads of the row-in-registers kernels cannot address)
    return t, (t.stride(0) if G > 1 else max(t.stride(0), C))


def _groups(rows, rows_per_group):
    if rows_per_group is None or int(rows_per_group) <= 0:
        raise ValueError("rows_per_group must be a positive row count when per-group vectors are given")
    rpg = int(rows_per_group)
    return rpg, max(1, (rows + rpg - 1) // rpg)


class _LayerNormModulateFn(torch.autograd.Function):
    """Returns (y, x): the second output is the input itself, handed on to the residual add, so that the residual stream's gradient comes
    back as an argument of this backward and is added inside the kernel (dx = dres + ...) instead of by autograd's accumulation."""

    @staticmethod
    def forward(ctx, x, ln_w, ln_b, shift, scale, rpg, mod_ld, eps, dtype):
        x2 = x.reshape(-1, x.shape[-1])
        y = torch.empty(x2.shape, dtype=dtype, device=x.device)
        if x2.shape[0] > 0:
            dit_ops.layernorm_modulate(x2, y, eps, ln_w, ln_b, shift, scale, mod_ld, rpg)
        ctx.save_for_backward(x2, ln_w, ln_b, scale)
        ctx.rpg, ctx.mod_ld, ctx.eps, ctx.has_shift = rpg, mod_ld, eps, shift is not None
        ctx.x_shape = x.shape
        ctx.set_materialize_grads(False)                     # an unused output's gradient arrives as None, not as a tensor of zeros
        return y.view(x.shape), x

    @staticmethod
    def backward(ctx, dy, dres):
        x2, ln_w, ln_b, scale = ctx.saved_tensors
        rows, C = x2.shape
        if dy is None:                                       # only the pass-through output was used
            return (dres,) + (None,) * 8
        dy2 = dy.reshape(rows, C)
        if not dy2.is_contiguous():
            dy2 = dy2.contiguous()
        if dres is not None:
            dres = dres.reshape(rows, C)
            if dres.dtype != torch.float32 or not dres.is_contiguous():
                dres = dres.float().contiguous()
        dev = x2.device
        dx = torch.empty_like(x2)
        G = max(1, (rows + ctx.rpg - 1) // ctx.rpg) if scale is not None else 0
        dshift = torch.zeros((G, C), dtype=torch.float32, device=dev) if scale is not None else None
        dscale = torch.zeros((G, C), dtype=torch.float32, device=dev) if scale is not None else None
        dw = torch.zeros(C, dtype=torch.float32, device=dev) if ln_w is not None else None
        db = torch.zeros(C, dtype=torch.float32, device=dev) if ln_w is not None else None
        if rows > 0:
            ws = _scratch("gvf_ln_mod_bwd_workspace_bytes", dev, rows, C, ctx.rpg if scale is not None else 0)
            _lib.check(_lib.lib().gvf_ln_mod_bwd(dit_ops.dt_code(dy2.dtype), _p(x2), _p(dy2), _p(dres), _p(dx), rows, C, float(ctx.eps), _p(ln_w), _p(ln_b),
                                                 _p(scale), ctx.mod_ld, ctx.rpg, _p(dshift), _p(dscale), _p(dw), _p(db), _p(ws), ws.numel(),
                                                 _lib.current_stream(dev)), "gvf_ln_mod_bwd")
        need = ctx.needs_input_grad
        return (dx.view(ctx.x_shape) if need[0] else None, dw if need[1] else None, db if need[2] else None,
                dshift if (ctx.has_shift and need[3]) else None, dscale if need[4] else None, None, None, None, None)


def layernorm_modulate(x, ln_w=None, ln_b=None, shift=None, scale=None, rows_per_group=None, eps=1e-6, dtype=torch.bfloat16,
                       return_residual=False):
    """LayerNorm over the last dimension of x (fp32, contiguous), then y = (xh * ln_w + ln_b) * (1 + scale_g) + shift_g with the optional
    affine pair and the optional per-group pair (g = row / rows_per_group over the flattened rows), stored in `dtype` (fp16 / bf16).
    Differentiable in x, ln_w, ln_b, shift and scale.  return_residual=True returns (y, x_res) with x_res the input itself: use x_res in
    the residual add and the stream's gradient is added to dx inside the backward kernel (the fused dres + dx); with the default, autograd
    adds the two with a launch of its own."""
    _lib.require_cuda(x, ln_w, ln_b, shift, scale)
    dit_ops.dt_code(dtype)
    if x.dtype != torch.float32 or x.dim() < 2:
        raise ValueError(f"layernorm_modulate: x must be an fp32 [..., C] tensor, got {x.dtype} {tuple(x.shape)}")
    if (ln_w is None) != (ln_b is None) or (shift is None) != (scale is None):
        raise ValueError("layernorm_modulate: ln_w / ln_b and shift / scale are given in pairs")
    if not x.is_contiguous():
        x = x.contiguous()
    C = x.shape[-1]
    rows = x.numel() // C
    if ln_w is not None:
        if ln_w.shape != (C,) or ln_b.shape != (C,) or ln_w.dtype != torch.float32 or ln_b.dtype != torch.float32:
            raise ValueError(f"layernorm_modulate: ln_w, ln_b must be fp32 [{C}]")
        ln_w, ln_b = ln_w.contiguous(), ln_b.contiguous()
    rpg, mod_ld = 0, 0
    if scale is not None:
        rpg, G = _groups(rows, rows_per_group)
        scale, mod_ld = _table_view(scale, "scale", G, C)
        shift, ld2 = _table_view(shift, "shift", G, C)
        if ld2 != mod_ld:                                   # the forward kernel reads both tables through one row stride
            shift, scale = shift.contiguous(), scale.contiguous()
            mod_ld = C
    y, x_res = _LayerNormModulateFn.apply(x, ln_w, ln_b, shift, scale, rpg, mod_ld, float(eps), dtype)
    return (y, x_res) if return_residual else y


class _GateResidualFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, h, gate, rpg, gate_ld):
        rows, C = x.numel() // x.shape[-1], x.shape[-1]
        out = torch.empty_like(x)
        if rows > 0:
            _lib.check(_lib.lib().gvf_gate_residual_fwd(dit_ops.dt_code(h.dtype), _p(x), _p(h), _p(gate), gate_ld, rpg, _p(out), rows, C,
                                                        _lib.current_stream(x.device)), "gvf_gate_residual_fwd")
        if gate is not None:
            ctx.save_for_backward(h, gate)                   # (without a gate the backward needs no tensor: dh = dout rounded)
        ctx.rpg, ctx.gate_ld, ctx.h_shape, ctx.h_dtype = rpg, gate_ld, h.shape, h.dtype
        return out

    @staticmethod
    def backward(ctx, dout):
        saved = ctx.saved_tensors                            # (read once: a checkpointed region unpacks on each read)
        h, gate = saved if saved else (None, None)
        C = ctx.h_shape[-1]
        rows = dout.numel() // C
        dev = dout.device
        need = ctx.needs_input_grad
        if dout.dtype != torch.float32 or not dout.is_contiguous():
            dout = dout.float().contiguous()
        dh, dgate = None, None
        if need[1] or (gate is not None and need[2]):
            dh = torch.empty(ctx.h_shape, dtype=ctx.h_dtype, device=dev)
            G = max(1, (rows + ctx.rpg - 1) // ctx.rpg) if gate is not None else 0
            dgate = torch.zeros((G, C), dtype=torch.float32, device=dev) if gate is not None else None
            if rows > 0:
                ws = _scratch("gvf_gate_residual_bwd_workspace_bytes", dev, rows, C, ctx.rpg if gate is not None else 0)
                _lib.check(_lib.lib().gvf_gate_residual_bwd(dit_ops.dt_code(ctx.h_dtype), _p(dout), _p(h), _p(gate), ctx.gate_ld, ctx.rpg, _p(dh), _p(dgate),
                                                            rows, C, _p(ws), ws.numel(), _lib.current_stream(dev)), "gvf_gate_residual_bwd")
        # the gradient of x is dout itself: the same tensor, no copy
        return (dout if need[0] else None, dh if need[1] else None, dgate if (gate is not None and need[2]) else None, None, None)


def gate_residual(x, h, gate=None, rows_per_group=None):
    """out = x + gate_g * h: x fp32 [..., C] (the residual stream), h fp16 / bf16 of the same shape (a projection's output), gate an optional
    [G, C] fp32 per-group vector (g = row / rows_per_group; a `chunk` view is read in place); without a gate, plain x + h.  Differentiable in
    x, h and gate; the gradient of x is the incoming gradient tensor itself."""
    _lib.require_cuda(x, h, gate)
    dit_ops.dt_code(h.dtype)
    if x.dtype != torch.float32 or x.shape != h.shape or x.dim() < 2:
        raise ValueError(f"gate_residual: x must be fp32 and h 16-bit of one [..., C] shape, got {x.dtype} {tuple(x.shape)} / {h.dtype} {tuple(h.shape)}")
    x, h = x.contiguous(), h.contiguous()
    C = x.shape[-1]
    rpg, gate_ld = 0, 0
    if gate is not None:
        rpg, G = _groups(x.numel() // C, rows_per_group)
        gate, gate_ld = _table_view(gate, "gate", G, C)
    return _GateResidualFn.apply(x, h, gate, rpg, gate_ld)


def _rows_view(t):
    """[..., H, d] 16-bit -> (tensor, rows, row stride) with heads packed, channels contiguous and the leading dimensions one strided run of
    16-byte-aligned rows (the unbind slice of a packed projection); anything else is copied."""
    H, d = t.shape[-2], t.shape[-1]
    rows = t.numel() // (H * d)
    ok = t.stride(-1) == 1 and t.stride(-2) == d and t.data_ptr() % 16 == 0
    ld = H * d
    if ok and t.dim() > 2:
        ld = t.stride(-3)
        ok = ld >= H * d and ld % 8 == 0
        for i in range(t.dim() - 4, -1, -1):
            ok = ok and (t.shape[i] == 1 or t.stride(i) == t.stride(i + 1) * t.shape[i + 1])
    if not ok:
        t, ld = t.contiguous(), H * d
    return t, rows, ld


class _RmsNormHeadsFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, gamma):
        H, d = x.shape[-2], x.shape[-1]
        xv, rows, ldx = _rows_view(x)
        y = torch.empty(x.shape, dtype=x.dtype, device=x.device)
        if rows > 0:
            _lib.check(_lib.lib().gvf_rmsnorm_heads_fwd(dit_ops.dt_code(x.dtype), _p(xv), ldx, _p(gamma), _p(y), H * d, rows, H, d,
                                                        _lib.current_stream(x.device)), "gvf_rmsnorm_heads_fwd")
        ctx.save_for_backward(xv, gamma)
        ctx.ldx, ctx.rows = ldx, rows
        return y

    @staticmethod
    def backward(ctx, dy):
        xv, gamma = ctx.saved_tensors
        H, d = gamma.shape
        rows, dev = ctx.rows, xv.device
        dyv, _, lddy = _rows_view(dy)
        dx = torch.empty(xv.shape, dtype=xv.dtype, device=dev)
        dgamma = torch.zeros((H, d), dtype=torch.float32, device=dev)
        if rows > 0:
            ws = _scratch("gvf_rmsnorm_heads_bwd_workspace_bytes", dev, rows, H, d)
            _lib.check(_lib.lib().gvf_rmsnorm_heads_bwd(dit_ops.dt_code(xv.dtype), _p(xv), ctx.ldx, _p(dyv), lddy, _p(gamma), _p(dx), H * d, _p(dgamma),
                                                        rows, H, d, _p(ws), ws.numel(), _lib.current_stream(dev)), "gvf_rmsnorm_heads_bwd")
        need = ctx.needs_input_grad
        return (dx if need[0] else None, dgamma if need[1] else None)


def rmsnorm_heads(x, gamma):
    """MultiHeadRMSNorm: y = x / max(|x|, 1e-12) * gamma[h, :] * sqrt(d) over the last dimension of x [..., H, d] (fp16 / bf16, d 32 or 64), fp32
    inside, rounded once to x's type; gamma fp32 [H, d].  The q / k slice of a packed qkv / kv projection is read in place.  Differentiable
    in x and gamma."""
    _lib.require_cuda(x, gamma)
    dit_ops.dt_code(x.dtype)
    if x.dim() < 3 or gamma.dim() != 2 or tuple(x.shape[-2:]) != tuple(gamma.shape) or gamma.dtype != torch.float32:
        raise ValueError(f"rmsnorm_heads: x [..., H, d] and fp32 gamma [H, d] do not fit: {tuple(x.shape)} / {tuple(gamma.shape)} {gamma.dtype}")
    if x.shape[-1] not in (32, 64) or x.shape[-2] * x.shape[-1] > 2048:
        raise NotImplementedError(f"rmsnorm_heads: head_dim {x.shape[-1]} x {x.shape[-2]} heads (32 and 64, up to 2048 channels, are built)")
    return _RmsNormHeadsFn.apply(x, gamma.contiguous())
