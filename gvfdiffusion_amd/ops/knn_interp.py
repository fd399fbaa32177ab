"""KNN interpolation of point motion and the interpolation ("deformation xyz") loss of the motion-VAE training step
(include/gvf_interp.h, csrc/interp.hip; the reference's compute_interpolation_loss_delta_interp, train_vae.py:486-586, and the
encoder's compute_delta_interp).  Search, weights, gather, loss and gradient are HIP kernels; there is no CPU fallback and no
(P, N)-sized intermediate.  The loss is differentiable in `pred` only (the reference forms the estimate under no_grad)."""
import ctypes

import torch

from .. import _lib
from ._util import f32c as _f32c, scratch as _scratch

_vp, _i, _i64, _sz, _f = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64, ctypes.c_size_t, ctypes.c_float

MAX_K = 16   # GVF_INTERP_MAX_K

_lib.register({
    "gvf_knn_interp_weights": (_i, [_vp, _vp, _vp, _i, _i, _i, _i, _f, _i, _vp, _vp, _vp, _vp]),
    "gvf_knn_interp_apply": (_i, [_vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _vp, _vp]),
    "gvf_interp_loss_scratch_bytes": (_i, [_i, _i, _i, ctypes.POINTER(_sz)]),
    "gvf_interp_loss_forward": (_i, [_vp, _i64, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _vp, _vp, _vp, _vp, _sz, _vp]),
    "gvf_interp_loss_backward": (_i, [_vp, _vp, _vp, _i, _i, _i, _vp, _i64, _i, _vp]),
})


def _check(name, q, a, m, lengths, k, pred=None):
    """Shapes and values (ValueError), then the device (GvfError).  Returns (B, P, N, T or None, lengths as an int32 device
    tensor or None)."""
    for what, t in (("q", q), ("a", a), ("m", m)):
        if t is None:
            continue
        if not isinstance(t, torch.Tensor):
            raise TypeError(f"{name}: {what} must be a tensor")
        if t.requires_grad:
            raise ValueError(f"{name}: {what} requires grad; the interpolation is differentiable in pred only (detach {what})")
    if q.dim() != 3 or q.shape[-1] != 3 or a.dim() != 3 or a.shape[-1] != 3:
        raise ValueError(f"{name}: expected q (B, P, 3) and a (B, N, 3), got {tuple(q.shape)} and {tuple(a.shape)}")
    B, P, N = int(q.shape[0]), int(q.shape[1]), int(a.shape[1])
    if a.shape[0] != B:
        raise ValueError(f"{name}: q has {B} samples, a has {a.shape[0]}")
    if B == 0 or P == 0 or N == 0:
        raise ValueError(f"{name}: empty input, q {tuple(q.shape)}, a {tuple(a.shape)}")
    T = None
    if m is not None:
        if m.dim() != 4 or m.shape[0] != B or m.shape[2] != N or m.shape[3] != 3 or m.shape[1] == 0:
            raise ValueError(f"{name}: expected m (B, T, N, 3) = ({B}, T, {N}, 3), got {tuple(m.shape)}")
        T = int(m.shape[1])
    k = int(k)
    if k < 1 or k > MAX_K:
        raise ValueError(f"{name}: k = {k} outside 1..{MAX_K}")
    if k > N:
        raise ValueError(f"{name}: k = {k} exceeds the {N} anchors")
    host_len = None
    if lengths is not None:
        if isinstance(lengths, torch.Tensor):
            if lengths.dim() != 1 or lengths.shape[0] != B or lengths.dtype.is_floating_point:
                raise ValueError(f"{name}: lengths must be {B} integers, got {tuple(lengths.shape)} {lengths.dtype}")
            if not lengths.is_cuda:
                host_len = [int(v) for v in lengths.tolist()]
        else:
            host_len = [int(v) for v in lengths]
            if len(host_len) != B:
                raise ValueError(f"{name}: {len(host_len)} lengths for {B} samples")
        if host_len is not None and (min(host_len) < 0 or max(host_len) > P):
            raise ValueError(f"{name}: lengths {host_len} outside 0..P = {P}")
    if pred is not None:
        if not isinstance(pred, torch.Tensor):
            raise TypeError(f"{name}: pred must be a tensor")
        if pred.dim() != 4 or pred.shape[0] != B or pred.shape[1] != T or pred.shape[2] != P or pred.shape[3] < 3:
            raise ValueError(f"{name}: expected pred ({B}, {T}, {P}, >= 3), got {tuple(pred.shape)}")
    _lib.require_cuda(q, a, m, pred)
    if any(t is not None and t.device != q.device for t in (a, m, pred)):
        raise ValueError(f"{name}: inputs are on different devices")
    if lengths is None:
        len_dev = None
    elif host_len is not None:
        len_dev = torch.tensor(host_len, dtype=torch.int32, device=q.device)
    else:   # a device tensor is used as it is (a value above P counts as P on the device): no host read-back
        len_dev = lengths.to(device=q.device, dtype=torch.int32).contiguous()
    return B, P, N, T, k, len_dev


def _weights(q, a, len_dev, B, P, N, k, beta, adaptive, want_dist):
    idx = torch.empty((B, P, k), dtype=torch.int32, device=q.device)
    w = torch.empty((B, P, k), dtype=torch.float32, device=q.device)
    dist = torch.empty((B, P, k), dtype=torch.float32, device=q.device) if want_dist else None
    _lib.check(_lib.lib().gvf_knn_interp_weights(_lib.ptr(q), _lib.ptr(len_dev), _lib.ptr(a), B, P, N, k, float(beta), int(bool(adaptive)),
                                                 _lib.ptr(idx), _lib.ptr(w), _lib.ptr(dist), _lib.current_stream(q.device)),
               "gvf_knn_interp_weights")
    return idx, w, dist


@torch.no_grad()
def knn_interp_weights(q, a, lengths=None, k: int = 8, beta: float = 7.0, adaptive_radius: bool = True, return_dists: bool = False):
    """q (B, P, 3), a (B, N, 3) -> idx (B, P, k) int32, w (B, P, k) [, squared distances (B, P, k)]: the k nearest anchors of every
    query (ascending distance, the lower index first among equals) and their normalised interpolation weights.  lengths: valid
    queries per sample (a sequence or tensor of B integers); the queries beyond get weight 0."""
    B, P, N, _, k, len_dev = _check("knn_interp_weights", q, a, None, lengths, k)
    idx, w, dist = _weights(_f32c(q), _f32c(a), len_dev, B, P, N, k, beta, adaptive_radius, return_dists)
    return (idx, w, dist) if return_dists else (idx, w)


@torch.no_grad()
def delta_interp(q, a, m, lengths=None, k: int = 8, beta: float = 7.0, adaptive_radius: bool = True) -> torch.Tensor:
    """KNN-interpolated motion est (B, T, P, 3) of the queries q (B, P, 3) from the anchors a (B, N, 3) and their positions per frame
    m (B, T, N, 3): sum_k w_k (m[:, t, idx_k] - a[:, idx_k])."""
    B, P, N, T, k, len_dev = _check("delta_interp", q, a, m, lengths, k)
    q, a, m = _f32c(q), _f32c(a), _f32c(m)
    idx, w, _ = _weights(q, a, len_dev, B, P, N, k, beta, adaptive_radius, False)
    est = torch.empty((B, T, P, 3), dtype=torch.float32, device=q.device)
    _lib.check(_lib.lib().gvf_knn_interp_apply(_lib.ptr(idx), _lib.ptr(w), _lib.ptr(a), _lib.ptr(m), B, T, P, N, k, _lib.ptr(est),
                                               _lib.current_stream(q.device)), "gvf_knn_interp_apply")
    return est


def _row_stride(pred: torch.Tensor):
    """The row stride if the (b, t, p) rows of pred (B, T, P, C) are evenly spaced in that order with unit channel stride, else None."""
    B, T, P, _ = pred.shape
    s = pred.stride(2) if P > 1 else (pred.stride(1) // P if T > 1 else (pred.stride(0) // (T * P) if B > 1 else pred.shape[3]))
    if s < 3 or pred.stride(3) != 1:
        return None
    want = (T * P * s, P * s, s)
    ok = all(pred.shape[d] == 1 or pred.stride(d) == want[d] for d in range(3))
    return int(s) if ok else None


class _InterpL1Fn(torch.autograd.Function):
    """pred (B, T, P, C >= 3) -> (loss, est or None); the gradient flows to pred only, written by the backward kernel from the sign
    bytes the forward left (channels >= 3 zero)."""

    @staticmethod
    def forward(ctx, pred, idx, w, a, m, len_dev, want_est: bool):
        B, T, N = int(m.shape[0]), int(m.shape[1]), int(m.shape[2])
        P, k, C = int(idx.shape[1]), int(idx.shape[2]), int(pred.shape[3])
        stride = _row_stride(pred)
        if stride is None:
            pred = pred[..., :3].contiguous()
            stride = 3
        dev = pred.device
        l = _lib.lib()
        scratch = _scratch("gvf_interp_loss_scratch_bytes", dev, B, T, P)
        loss = torch.empty(1, dtype=torch.float32, device=dev)
        est = torch.empty((B, T, P, 3), dtype=torch.float32, device=dev) if want_est else None
        need_grad = ctx.needs_input_grad[0]
        sign = torch.empty((B, T, P), dtype=torch.uint8, device=dev) if need_grad else None
        _lib.check(l.gvf_interp_loss_forward(_lib.ptr(pred), stride, _lib.ptr(idx), _lib.ptr(w), _lib.ptr(a), _lib.ptr(m), _lib.ptr(len_dev),
                                             B, T, P, N, k, _lib.ptr(loss), _lib.ptr(est), _lib.ptr(sign), _lib.ptr(scratch),
                                             scratch.numel(), _lib.current_stream(dev)), "gvf_interp_loss_forward")
        if need_grad:
            ctx.save_for_backward(sign, len_dev)
            ctx.geom = (B, T, P, C)
        ctx.set_materialize_grads(False)
        if est is not None:
            ctx.mark_non_differentiable(est)
        return loss[0], est

    @staticmethod
    def backward(ctx, g_loss, _g_est):
        if not ctx.needs_input_grad[0] or g_loss is None:
            return (None,) * 7
        B, T, P, C = ctx.geom
        sign, len_dev = ctx.saved_tensors
        g = g_loss.reshape(1).float().contiguous()
        grad = torch.empty((B, T, P, C), dtype=torch.float32, device=g.device)
        _lib.check(_lib.lib().gvf_interp_loss_backward(_lib.ptr(sign), _lib.ptr(g), _lib.ptr(len_dev), B, T, P, _lib.ptr(grad), C, C,
                                                       _lib.current_stream(g.device)), "gvf_interp_loss_backward")
        return (grad,) + (None,) * 6


def interpolation_l1(pred, q, a, m, lengths=None, k: int = 8, beta: float = 7.0, adaptive_radius: bool = True, return_est: bool = False):
    """Masked L1 between the predicted deltas pred (B, T, P, C >= 3; channels 0..2 are scored, e.g. the decoder's (.., 14) output or
    its [..., :3] view, both read in place) and the KNN-interpolated motion of the queries (delta_interp):
        sum_{b, t, p < lengths[b], c < 3} |pred - est| / (3 T sum_b lengths[b])
    as a 0-d tensor differentiable in pred; return_est: also the estimate (B, T, P, 3), which carries no gradient.  A pred whose
    (b, t, p) rows are not evenly spaced in memory (e.g. a slice along P) is scored from a contiguous copy of its channels 0..2."""
    if m is None:
        raise TypeError("interpolation_l1: m must be a tensor")
    B, P, N, T, k, len_dev = _check("interpolation_l1", q, a, m, lengths, k, pred=pred)
    if pred.dtype != torch.float32:
        pred = pred.float()
    q, a, m = _f32c(q), _f32c(a), _f32c(m)
    with torch.no_grad():
        idx, w, _ = _weights(q, a, len_dev, B, P, N, k, beta, adaptive_radius, False)
    loss, est = _InterpL1Fn.apply(pred, idx, w, a, m, len_dev, bool(return_est))
    return (loss, est) if return_est else loss
