"""LPIPS (VGG16) term of the render loss (include/gvf_lpips.h, csrc/conv3x3.hip, csrc/lpips.hip): the reference's
`LPIPS_vgg(pred * 2 - 1, gt * 2 - 1)` (train_vae.py:328-334; utils/lpips/lpips.py, networks.py) as HIP kernels, forward and
gradient with respect to the first argument.  There is no CPU fallback and nothing is ever downloaded: the module starts from a
deterministic initialisation and takes real weights through load_state_dict (its key names are the reference's).

Per-layer wrappers (pack_conv, conv3x3, first_forward, first_backward, maxpool2x2, maxpool2x2_backward, tap_forward,
tap_backward) bind the C ABI one to one; `LPIPS` composes them in one autograd Function.  Activations are NHWC 16-bit tensors of
the forward dtype; every gradient tensor and the input-gradient weight images are bf16 whatever the forward dtype (gvf_lpips.h)."""
import ctypes
import math

import torch
from torch import nn

from .. import _lib
from . import _util, precision
from ._util import stream as _stream

_vp, _i, _sz = ctypes.c_void_p, ctypes.c_int, ctypes.c_size_t

PACK_FWD, PACK_DGRAD = 0, 1     # GVF_CONV_PACK_*
CONV_RELU = 1                   # GVF_CONV_RELU
TAP_RELU_MASK = 1               # GVF_TAP_RELU_MASK

_lib.register({
    "gvf_conv3x3_packed_bytes": (_i, [_i, _i, _i, ctypes.POINTER(_sz)]),
    "gvf_conv3x3_pack": (_i, [_vp, _i, _i, _i, _i, _vp, _sz, _vp]),
    "gvf_conv3x3": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _i, _vp]),
    "gvf_lpips_first_forward": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _vp]),
    "gvf_lpips_first_backward": (_i, [_vp, _vp, _vp, _vp, _i, _i, _i, _vp]),
    "gvf_maxpool2x2_forward": (_i, [_vp, _vp, _i, _i, _i, _i, _i, _vp]),
    "gvf_maxpool2x2_backward": (_i, [_vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _vp]),
    "gvf_lpips_tap_scratch_bytes": (_i, [_i, _i, _i, ctypes.POINTER(_sz)]),
    "gvf_lpips_tap_forward": (_i, [_vp, _vp, _vp, _i, _i, _i, _i, _i, _vp, _vp, _sz, _vp]),
    "gvf_lpips_tap_backward": (_i, [_vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _vp, _vp]),
})

# vgg16.features[0:30]: (index in features, Cin, Cout) of the 13 convolutions; a 2x2 pool follows convs 2, 4, 7, 10 (0-based 1, 3, 6, 9);
# the taps are the ReLU outputs of convs 2, 4, 7, 10, 13
VGG_CONVS = ((0, 3, 64), (2, 64, 64), (5, 64, 128), (7, 128, 128), (10, 128, 256), (12, 256, 256), (14, 256, 256), (17, 256, 512),
             (19, 512, 512), (21, 512, 512), (24, 512, 512), (26, 512, 512), (28, 512, 512))
POOL_AFTER = (1, 3, 6, 9)
TAPS = (1, 3, 6, 9, 12)
TAP_CHANNELS = (64, 128, 256, 512, 512)
MIN_SIDE = 16                   # four floor pools


def _dt(dtype) -> int:
    if dtype is torch.bfloat16:
        return 0
    if dtype is torch.float16:
        return 1
    raise ValueError(f"lpips: the operand type must be torch.float16 or torch.bfloat16, got {dtype}")


def _nhwc(t, what, C=None):
    _lib.require_cuda(t)
    if t.dim() != 4 or not t.is_contiguous() or (C is not None and t.shape[3] != C):
        raise ValueError(f"lpips: {what} must be a contiguous (N,H,W,C) tensor, got {tuple(t.shape)}")
    return tuple(int(s) for s in t.shape)


# ---- per-layer wrappers ---------------------------------------------------------------------------------------------------------------

def packed_bytes(cout: int, cin: int, mode: int = PACK_FWD) -> int:
    return _util.workspace_bytes("gvf_conv3x3_packed_bytes", cout, cin, mode)


def pack_conv(weight: torch.Tensor, mode: int, dtype) -> torch.Tensor:
    """fp32 (Cout,Cin,3,3) -> the 16-bit image gvf_conv3x3 reads (PACK_FWD) or the image of its input gradient (PACK_DGRAD)."""
    _lib.require_cuda(weight)
    if weight.dim() != 4 or tuple(weight.shape[2:]) != (3, 3):
        raise ValueError(f"lpips: expected a (Cout,Cin,3,3) weight, got {tuple(weight.shape)}")
    w = weight.detach().float().contiguous()
    cout, cin = int(w.shape[0]), int(w.shape[1])
    img = torch.empty(packed_bytes(cout, cin, mode), dtype=torch.uint8, device=w.device)
    _lib.check(_lib.lib().gvf_conv3x3_pack(_lib.ptr(w), cout, cin, mode, _dt(dtype), _lib.ptr(img), img.numel(), _stream(w)), "gvf_conv3x3_pack")
    return img


def conv3x3(x: torch.Tensor, wimg: torch.Tensor, cout: int, bias=None, addend=None, mask_src=None, relu: bool = False) -> torch.Tensor:
    """(N,H,W,Cin) 16-bit -> (N,H,W,cout) of the same type; wimg from pack_conv in x's dtype.  See gvf_conv3x3 for the epilogue."""
    N, H, W, cin = _nhwc(x, "the activation")
    _lib.require_cuda(wimg, bias, addend, mask_src)
    out = torch.empty((N, H, W, cout), dtype=x.dtype, device=x.device)
    for t, what in ((addend, "addend"), (mask_src, "mask_src")):
        if t is not None and (tuple(t.shape) != tuple(out.shape) or not t.is_contiguous() or t.element_size() != 2):
            raise ValueError(f"lpips: {what} must be a contiguous 16-bit tensor of the output's shape {tuple(out.shape)}")
    if addend is not None and addend.dtype != x.dtype:
        raise ValueError("lpips: the addend must have the activation's dtype")
    if wimg.numel() != packed_bytes(cout, cin):
        raise ValueError(f"lpips: the weight image has {wimg.numel()} bytes, not those of a {cout} x {cin} x 3 x 3 weight")
    _lib.check(_lib.lib().gvf_conv3x3(_lib.ptr(x), _lib.ptr(wimg), _lib.ptr(bias), _lib.ptr(addend), _lib.ptr(mask_src), _lib.ptr(out),
                                      N, H, W, cin, cout, CONV_RELU if relu else 0, _dt(x.dtype), _stream(x)), "gvf_conv3x3")
    return out


def first_forward(x: torch.Tensor, wimg: torch.Tensor, bias: torch.Tensor, mean: torch.Tensor, std: torch.Tensor, dtype) -> torch.Tensor:
    """fp32 (N,3,H,W) -> (N,H,W,64) `dtype`: z-score, first convolution, bias, ReLU."""
    _lib.require_cuda(x, wimg, bias, mean, std)
    N, _, H, W = x.shape
    out = torch.empty((N, H, W, 64), dtype=dtype, device=x.device)
    _lib.check(_lib.lib().gvf_lpips_first_forward(_lib.ptr(x), _lib.ptr(wimg), _lib.ptr(bias), _lib.ptr(mean), _lib.ptr(std), _lib.ptr(out),
                                                  N, H, W, _dt(dtype), _stream(x)), "gvf_lpips_first_forward")
    return out


def first_backward(z: torch.Tensor, weight: torch.Tensor, std: torch.Tensor) -> torch.Tensor:
    """bf16 (N,H,W,64) gradient at the first convolution's output -> fp32 (N,3,H,W) gradient of the image (1 / std included)."""
    N, H, W, _ = _nhwc(z, "the gradient", 64)
    _lib.require_cuda(weight, std)
    if z.dtype is not torch.bfloat16:
        raise ValueError("lpips: gradients are bf16")
    dx = torch.empty((N, 3, H, W), dtype=torch.float32, device=z.device)
    _lib.check(_lib.lib().gvf_lpips_first_backward(_lib.ptr(z), _lib.ptr(weight), _lib.ptr(std), _lib.ptr(dx), N, H, W, _stream(z)),
               "gvf_lpips_first_backward")
    return dx


def maxpool2x2(x: torch.Tensor) -> torch.Tensor:
    N, H, W, C = _nhwc(x, "the activation")
    out = torch.empty((N, H // 2, W // 2, C), dtype=x.dtype, device=x.device)
    _lib.check(_lib.lib().gvf_maxpool2x2_forward(_lib.ptr(x), _lib.ptr(out), N, H, W, C, _dt(x.dtype), _stream(x)), "gvf_maxpool2x2_forward")
    return out


def maxpool2x2_backward(a: torch.Tensor, g_pooled: torch.Tensor, tap_grad: torch.Tensor) -> torch.Tensor:
    """z = ([argmax] g_pooled + tap_grad) [a > 0]: a in the forward dtype, the three gradients bf16."""
    N, H, W, C = _nhwc(a, "the activation")
    _lib.require_cuda(g_pooled, tap_grad)
    if g_pooled.dtype is not torch.bfloat16 or tap_grad.dtype is not torch.bfloat16:
        raise ValueError("lpips: gradients are bf16")
    if tuple(g_pooled.shape) != (N, H // 2, W // 2, C) or tuple(tap_grad.shape) != (N, H, W, C) or not g_pooled.is_contiguous() \
            or not tap_grad.is_contiguous():
        raise ValueError("lpips: pool backward shapes do not match the activation")
    z = torch.empty((N, H, W, C), dtype=torch.bfloat16, device=a.device)
    _lib.check(_lib.lib().gvf_maxpool2x2_backward(_lib.ptr(a), _lib.ptr(g_pooled), _lib.ptr(tap_grad), _lib.ptr(z), N, H, W, C, _dt(a.dtype),
                                                  _stream(a)), "gvf_maxpool2x2_backward")
    return z


def _tap_args(ax, ay, lin):
    N, H, W, C = _nhwc(ax, "the activation")
    _lib.require_cuda(ay, lin)
    if tuple(ay.shape) != (N, H, W, C) or ay.dtype != ax.dtype or not ay.is_contiguous():
        raise ValueError("lpips: the two activations of a tap differ in shape or type")
    if lin.dtype is not torch.float32 or lin.numel() != C or not lin.is_contiguous():
        raise ValueError(f"lpips: lin must hold {C} fp32 weights")
    return N, H, W, C


def tap_forward(ax: torch.Tensor, ay: torch.Tensor, lin: torch.Tensor, out: torch.Tensor = None) -> torch.Tensor:
    """The N per-image terms of one tap (fp32)."""
    N, H, W, C = _tap_args(ax, ay, lin)
    scratch = _util.scratch("gvf_lpips_tap_scratch_bytes", ax.device, N, H, W)
    if out is None:
        out = torch.empty(N, dtype=torch.float32, device=ax.device)
    _lib.check(_lib.lib().gvf_lpips_tap_forward(_lib.ptr(ax), _lib.ptr(ay), _lib.ptr(lin), N, H, W, C, _dt(ax.dtype), _lib.ptr(out),
                                                _lib.ptr(scratch), scratch.numel(), _stream(ax)), "gvf_lpips_tap_forward")
    return out


def tap_backward(ax: torch.Tensor, ay: torch.Tensor, lin: torch.Tensor, upstream: torch.Tensor, relu_mask: bool = False) -> torch.Tensor:
    """bf16 (N,H,W,C): upstream[n] d term[n] / d ax; upstream is a device tensor of N fp32."""
    N, H, W, C = _tap_args(ax, ay, lin)
    _lib.require_cuda(upstream)
    if upstream.dtype is not torch.float32 or upstream.numel() != N or not upstream.is_contiguous():
        raise ValueError(f"lpips: upstream must hold {N} fp32 values")
    g = torch.empty((N, H, W, C), dtype=torch.bfloat16, device=ax.device)
    _lib.check(_lib.lib().gvf_lpips_tap_backward(_lib.ptr(ax), _lib.ptr(ay), _lib.ptr(lin), _lib.ptr(upstream), N, H, W, C, _dt(ax.dtype),
                                                 TAP_RELU_MASK if relu_mask else 0, _lib.ptr(g), _stream(ax)), "gvf_lpips_tap_backward")
    return g


# ---- the composition ------------------------------------------------------------------------------------------------------------------

class _Packed:
    """What the kernels read of one module in one forward dtype: packed once, reused every step."""

    def __init__(self, module, dtype):
        convs = [module.net.layers[str(i)] for i, _, _ in VGG_CONVS]
        self.dtype = dtype
        self.w0 = convs[0].weight.detach().float().contiguous()
        self.fwd = [pack_conv(c.weight, PACK_FWD, dtype) for c in convs]
        self.dgrad = [None] + [pack_conv(c.weight, PACK_DGRAD, torch.bfloat16) for c in convs[1:]]
        self.bias = [c.bias.detach().float().contiguous() for c in convs]
        self.mean = module.net.mean.detach().float().reshape(3).contiguous()
        self.std = module.net.std.detach().float().reshape(3).contiguous()
        self.lin = [l[1].weight.detach().float().reshape(-1).contiguous() for l in module.lin]


def _trunk(x, pk, keep_all):
    """The 13 ReLU outputs (keep_all) or the five taps only; every other activation is dropped as soon as its successor exists."""
    acts = []
    a = first_forward(x, pk.fwd[0], pk.bias[0], pk.mean, pk.std, pk.dtype)
    for k in range(13):
        if k:
            a = conv3x3(a, pk.fwd[k], VGG_CONVS[k][2], bias=pk.bias[k], relu=True)
        if keep_all or k in TAPS:
            acts.append(a)
        if k in POOL_AFTER:
            a = maxpool2x2(a)
    return acts


class _LpipsFn(torch.autograd.Function):
    """(x, y) fp32 (n,3,H,W) -> terms (5, n) fp32: the per-tap, per-image terms.  The gradient flows to x only."""

    @staticmethod
    def forward(ctx, x, y, pk):
        n = x.shape[0]
        grad = ctx.needs_input_grad[0]
        ax = _trunk(x, pk, keep_all=grad)
        ay = _trunk(y, pk, keep_all=False)
        taps_x = [ax[k] for k in TAPS] if grad else ax
        terms = torch.empty((5, n), dtype=torch.float32, device=x.device)
        for t in range(5):
            tap_forward(taps_x[t], ay[t], pk.lin[t], out=terms[t])
        if grad:
            ctx.pk, ctx.ax, ctx.ay = pk, ax, ay
        return terms

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g_terms):
        pk, ax, ay = ctx.pk, ctx.ax, ctx.ay
        ctx.ax = ctx.ay = None
        up = g_terms.float().contiguous()
        g = None                                      # gradient at the INPUT of conv k + 1 (pooled resolution where a pool lies between)
        for k in range(12, 0, -1):
            if k in TAPS:
                t = TAPS.index(k)
                if k == 12:
                    z = tap_backward(ax[k], ay[t], pk.lin[t], up[t], relu_mask=True)
                else:
                    z = maxpool2x2_backward(ax[k], g, tap_backward(ax[k], ay[t], pk.lin[t], up[t]))
                ay[t] = None
            else:
                z = g                                 # the ReLU mask of a_k was applied in the epilogue that produced g
            ax[k] = None
            mask = None if (k - 1) in POOL_AFTER else ax[k - 1]
            g = conv3x3(z, pk.dgrad[k], VGG_CONVS[k][1], mask_src=mask)
        return first_backward(g, pk.w0, pk.std), None, None


class _ConvParams(nn.Module):
    def __init__(self, cin, cout, gen):
        super().__init__()
        bound = math.sqrt(6.0 / (9 * cin))
        self.weight = nn.Parameter((torch.rand((cout, cin, 3, 3), generator=gen) * 2 - 1) * bound, requires_grad=False)
        self.bias = nn.Parameter((torch.rand(cout, generator=gen) * 2 - 1) * 0.05, requires_grad=False)


class _LinParams(nn.Module):
    def __init__(self, c, gen):
        super().__init__()
        self.weight = nn.Parameter(torch.rand((1, c, 1, 1), generator=gen) * (2.0 / c), requires_grad=False)


class _Trunk(nn.Module):
    def __init__(self, gen):
        super().__init__()
        self.layers = nn.ModuleDict({str(i): _ConvParams(cin, cout, gen) for i, cin, cout in VGG_CONVS})
        self.register_buffer("mean", torch.tensor([-.030, -.088, -.188])[None, :, None, None])
        self.register_buffer("std", torch.tensor([.458, .448, .450])[None, :, None, None])


class LPIPS(nn.Module):
    """LPIPS with the VGG16 trunk.  forward(x, y): x, y (N,3,H,W) fp32 in [-1, 1] on the GPU, H, W >= 16 -> 0-d loss, differentiable
    in x.  Parameter and buffer names are the reference's (net.layers.<i>.weight / .bias, net.mean, net.std, lin.<t>.1.weight), so a
    checkpoint of the reference's module loads with load_state_dict; until then the weights are a fixed pseudo-random initialisation.
    dtype: the forward operand type (default fp16, the reference's mixed precision; gradients are bf16 either way).  chunk: run the
    images in groups of `chunk` and add their terms, which bounds the saved activations (about 8 GB for 24 x 800^2 at once)."""

    def __init__(self, dtype=torch.float16, chunk=None):
        super().__init__()
        gen = torch.Generator().manual_seed(20261020)
        self.net = _Trunk(gen)
        self.lin = nn.ModuleList([nn.Sequential(nn.Identity(), _LinParams(c, gen)) for c in TAP_CHANNELS])
        self.dtype = precision.parse(dtype)
        if self.dtype is None:
            raise ValueError("lpips: dtype must be torch.float16 or torch.bfloat16")
        if chunk is not None and int(chunk) < 1:
            raise ValueError(f"lpips: chunk must be a positive number of images, got {chunk}")
        self.chunk = None if chunk is None else int(chunk)
        self._packed = {}

    def _apply(self, fn, *args, **kwargs):
        self._packed = {}
        return super()._apply(fn, *args, **kwargs)

    def load_state_dict(self, *args, **kwargs):
        self._packed = {}
        return super().load_state_dict(*args, **kwargs)

    def packed(self, dtype=None):
        """The packed weights of this module for `dtype`: built on first use, again after load_state_dict, .to() or an in-place update."""
        dtype = self.dtype if dtype is None else dtype
        stamp = tuple(p._version for p in self.parameters()) + (self.net.mean.device,)
        hit = self._packed.get(dtype)
        if hit is None or hit[0] != stamp:
            hit = (stamp, _Packed(self, dtype))
            self._packed[dtype] = hit
        return hit[1]

    def forward(self, x: torch.Tensor, y: torch.Tensor) -> torch.Tensor:
        if not isinstance(x, torch.Tensor) or not isinstance(y, torch.Tensor):
            raise TypeError("lpips: x and y must be tensors")
        _lib.require_cuda(x, y)
        if y.requires_grad:
            raise ValueError("lpips: y requires grad; the loss is differentiable in x only (detach the target)")
        if x.dim() != 4 or x.shape[1] != 3:
            raise ValueError(f"lpips: expected (N,3,H,W) images, got shape {tuple(x.shape)}")
        if x.shape != y.shape:
            raise ValueError(f"lpips: x {tuple(x.shape)} and y {tuple(y.shape)} differ in shape")
        if x.device != y.device or x.device != self.net.mean.device:
            raise ValueError("lpips: x, y and the module are on different devices")
        N, _, H, W = x.shape
        if N == 0 or H < MIN_SIDE or W < MIN_SIDE:
            raise ValueError(f"lpips: needs at least one image of at least {MIN_SIDE} x {MIN_SIDE} pixels (four 2x2 pools), got {tuple(x.shape)}")
        x, y = x.float().contiguous(), y.float().contiguous()
        pk = self.packed()
        step = N if self.chunk is None else self.chunk
        terms = [_LpipsFn.apply(x[i:i + step], y[i:i + step], pk) for i in range(0, N, step)]
        return (terms[0] if len(terms) == 1 else torch.cat(terms, dim=1)).sum() / N
