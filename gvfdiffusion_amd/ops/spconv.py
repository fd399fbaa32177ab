"""Submanifold sparse 3x3x3 convolution (include/gvf_spconv.h, csrc/spconv.hip): the reference's sp.SparseConv3d -> spconv.SubMConv3d
as HIP kernels, inference only.  There is no CPU fallback.

    build_neighbor_map(coords)            int32 [T,4] (b, x, y, z) -> int32 [T,27], tap k = kx * 9 + ky * 3 + kz, -1 where absent
    pack_weight(w, dtype)                 fp32 [Cout,3,3,3,Cin] -> the 16-bit MFMA image (once per module and operand type)
    conv3(x, nbr, wimg, cout, ...)        16-bit rows -> fp32 or 16-bit rows, bias and an fp32 addend (a block's skip path) in the epilogue
    ln_act(x, ...)                        fp32 rows -> act(LayerNorm [affine] [modulated]) as the 16-bit operand of the next convolution

MAP_BUILDS counts the neighbour maps built (a sampler builds one per resolution and sample set, not one per step: sparse/conv.py)."""
import ctypes

import torch

from .. import _lib
from . import _util
from ._util import stream as _stream
from .dit_ops import dt_code

_vp, _i, _sz, _f = ctypes.c_void_p, ctypes.c_int, ctypes.c_size_t, ctypes.c_float

ACT_NONE, ACT_SILU = 0, 1       # GVF_ACT_*
C_MAX = 2048
MAP_BUILDS = 0

_lib.register({
    "gvf_spconv_map_workspace_bytes": (_i, [_i, ctypes.POINTER(_sz)]),
    "gvf_spconv_neighbor_map": (_i, [_vp, _i, _vp, _vp, _sz, _vp]),
    "gvf_spconv_packed_bytes": (_i, [_i, _i, ctypes.POINTER(_sz)]),
    "gvf_spconv_pack": (_i, [_vp, _i, _i, _i, _vp, _sz, _vp]),
    "gvf_spconv3": (_i, [_vp, _i, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _vp]),
    "gvf_ln_act_rows": (_i, [_i, _vp, _vp, _i, _i, _f, _vp, _vp, _vp, _vp, _i, _vp]),
})


def map_workspace_bytes(T: int) -> int:
    return _util.workspace_bytes("gvf_spconv_map_workspace_bytes", int(T))


def build_neighbor_map(coords: torch.Tensor) -> torch.Tensor:
    """coords int32 [T,4] (batch, x, y, z), unique, x, y, z in [0, 1024) -> int32 [T,27] on the device, without a host read-back."""
    global MAP_BUILDS
    _lib.require_cuda(coords)
    if coords.dim() != 2 or coords.shape[1] != 4 or coords.dtype != torch.int32 or coords.shape[0] < 1:
        raise ValueError(f"spconv: coords must be a non-empty int32 [T,4] tensor, got {coords.dtype} {tuple(coords.shape)}")
    c = coords.contiguous()
    T = int(c.shape[0])
    ws = _util.scratch("gvf_spconv_map_workspace_bytes", c.device, T)
    nbr = torch.empty((T, 27), dtype=torch.int32, device=c.device)
    _lib.check(_lib.lib().gvf_spconv_neighbor_map(_lib.ptr(c), T, _lib.ptr(nbr), _lib.ptr(ws), ws.numel(), _stream(c)), "gvf_spconv_neighbor_map")
    MAP_BUILDS += 1
    return nbr


def packed_bytes(cout: int, cin: int) -> int:
    return _util.workspace_bytes("gvf_spconv_packed_bytes", int(cout), int(cin))


def pack_weight(w: torch.Tensor, dtype) -> torch.Tensor:
    """fp32 [Cout,3,3,3,Cin] (spconv 2's SubMConv3d.weight) -> the uint8 image conv3 reads, rounded to `dtype`."""
    _lib.require_cuda(w)
    if w.dim() != 5 or tuple(w.shape[1:4]) != (3, 3, 3):
        raise ValueError(f"spconv: expected a [Cout,3,3,3,Cin] weight, got {tuple(w.shape)}")
    wf = w.detach().float().contiguous()
    cout, cin = int(wf.shape[0]), int(wf.shape[4])
    img = torch.empty(packed_bytes(cout, cin), dtype=torch.uint8, device=wf.device)
    _lib.check(_lib.lib().gvf_spconv_pack(_lib.ptr(wf), cout, cin, dt_code(dtype), _lib.ptr(img), img.numel(), _stream(wf)), "gvf_spconv_pack")
    return img


def conv3(x: torch.Tensor, nbr: torch.Tensor, wimg: torch.Tensor, cout: int, bias=None, addend=None, out_dtype=torch.float32,
          cin: int = None, out: torch.Tensor = None) -> torch.Tensor:
    """x 16-bit [T, ld_in] (the first `cin` columns are the operand; default all of them), nbr int32 [T,27], wimg from pack_weight in
    x's type -> [T, cout] fp32 (out_dtype=torch.float32) or x's 16-bit type.  bias fp32 [cout], addend fp32 [T, cout], both optional."""
    _lib.require_cuda(x, nbr, wimg, bias, addend, out)
    if x.dim() != 2 or x.stride(1) != 1:
        raise ValueError(f"spconv: the operand must be 16-bit rows [T, ld], got {tuple(x.shape)}")
    T, ld_in = int(x.shape[0]), int(x.stride(0))
    cin = int(x.shape[1]) if cin is None else int(cin)
    dt = dt_code(x.dtype)
    if nbr.dtype != torch.int32 or tuple(nbr.shape) != (T, 27) or not nbr.is_contiguous():
        raise ValueError(f"spconv: nbr must be a contiguous int32 [{T},27] tensor")
    if wimg.numel() != packed_bytes(cout, cin):
        raise ValueError(f"spconv: the weight image has {wimg.numel()} bytes, not those of a {cout} x 27 x {cin} weight")
    if out_dtype not in (torch.float32, x.dtype):
        raise ValueError(f"spconv: the output is fp32 or the operand's type {x.dtype}, not {out_dtype}")
    if bias is not None and (bias.dtype != torch.float32 or bias.numel() != cout or not bias.is_contiguous()):
        raise ValueError(f"spconv: bias must hold {cout} fp32 values")
    if addend is not None and (addend.dtype != torch.float32 or tuple(addend.shape) != (T, cout) or not addend.is_contiguous()):
        raise ValueError(f"spconv: the addend must be a contiguous fp32 [{T},{cout}] tensor")
    if out is None:
        out = torch.empty((T, cout), dtype=out_dtype, device=x.device)
    elif out.dtype != out_dtype or tuple(out.shape) != (T, cout) or not out.is_contiguous():
        raise ValueError(f"spconv: out must be a contiguous {out_dtype} [{T},{cout}] tensor")
    _lib.check(_lib.lib().gvf_spconv3(_lib.ptr(x), ld_in, _lib.ptr(nbr), _lib.ptr(wimg), _lib.ptr(bias), _lib.ptr(addend), _lib.ptr(out),
                                      int(out_dtype == torch.float32), T, cin, int(cout), dt, _stream(x)), "gvf_spconv3")
    return out


def ln_act(x: torch.Tensor, ln_w=None, ln_b=None, shift=None, scale=None, act: int = ACT_NONE, eps: float = 1e-6, dtype=torch.bfloat16,
           out: torch.Tensor = None) -> torch.Tensor:
    """fp32 rows [T, C] -> `dtype` rows: act(LN_eps(x) [* ln_w + ln_b] [* (1 + scale) + shift]); shift, scale: ONE fp32 row of C each."""
    _lib.require_cuda(x, ln_w, ln_b, shift, scale, out)
    if x.dim() != 2 or x.dtype != torch.float32 or not x.is_contiguous():
        raise ValueError(f"spconv: ln_act takes contiguous fp32 rows [T, C], got {x.dtype} {tuple(x.shape)}")
    T, C = int(x.shape[0]), int(x.shape[1])
    for v, what in ((ln_w, "ln_w"), (ln_b, "ln_b"), (shift, "shift"), (scale, "scale")):
        if v is not None and (v.dtype != torch.float32 or v.numel() != C or v.stride(-1) != 1):
            raise ValueError(f"spconv: {what} must hold {C} contiguous fp32 values")
    if out is None:
        out = torch.empty((T, C), dtype=dtype, device=x.device)
    elif tuple(out.shape) != (T, C) or not out.is_contiguous():
        raise ValueError(f"spconv: out must be a contiguous 16-bit [{T},{C}] tensor")
    _lib.check(_lib.lib().gvf_ln_act_rows(dt_code(out.dtype), _lib.ptr(x), _lib.ptr(out), T, C, float(eps), _lib.ptr(ln_w), _lib.ptr(ln_b),
                                          _lib.ptr(shift), _lib.ptr(scale), int(act), _stream(x)), "gvf_ln_act_rows")
    return out
