"""Dense 3x3x3 convolution and occupancy read-out (include/gvf_conv3d.h, csrc/conv3d.hip): nn.Conv3d(cin, cout, 3, padding=1) of the
reference's sparse-structure decoder as a HIP kernel, inference only.  There is no CPU fallback.

A dense volume is the row matrix [B*X*Y*Z, C], row = ((b*X + x)*Y + y)*Z + z.

    pack_weight(w, dtype)                     fp32 [Cout,Cin,3,3,3] (nn.Conv3d's layout) -> the 16-bit MFMA image (once per module and type)
    conv3(x, grid, wimg, cin, cout, ...)      16-bit rows -> fp32 or 16-bit rows; bias and an fp32 addend in the epilogue; store="shuffle2"
                                              writes pixel_shuffle_3d(., 2) of the result: [B*2X*2Y*2Z, Cout/8]
    occupancy_coords(logits, grid)            fp32 logits -> int32 [n,4] (b, x, y, z) of the cells > 0, in row order (one count read-back)"""
import ctypes

import torch

from .. import _lib
from . import _util
from ._util import stream as _stream
from .dit_ops import dt_code

_vp, _i, _i64, _sz = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64, ctypes.c_size_t

STORE_ROWS, STORE_SHUFFLE2 = 0, 1       # GVF_CONV3D_STORE_*
C_MAX = 2048

_lib.register({
    "gvf_conv3d3_packed_bytes": (_i, [_i, _i, ctypes.POINTER(_sz)]),
    "gvf_conv3d3_pack": (_i, [_vp, _i, _i, _i, _vp, _sz, _vp]),
    "gvf_conv3d3": (_i, [_vp, _i, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _i, _i, _i, _vp]),
    "gvf_occupancy_workspace_bytes": (_i, [_i64, ctypes.POINTER(_sz)]),
    "gvf_occupancy_coords": (_i, [_vp, _i, _i, _i, _i, _vp, _i64, _vp, _vp, _sz, _vp]),
})


def packed_bytes(cout: int, cin: int) -> int:
    return _util.workspace_bytes("gvf_conv3d3_packed_bytes", int(cout), int(cin))


def pack_weight(w: torch.Tensor, dtype) -> torch.Tensor:
    """fp32 [Cout,Cin,3,3,3] (nn.Conv3d.weight) -> the uint8 image conv3 reads, rounded to `dtype`, Cin padded to 32 and Cout to 16."""
    _lib.require_cuda(w)
    if w.dim() != 5 or tuple(w.shape[2:]) != (3, 3, 3):
        raise ValueError(f"conv3d: expected a [Cout,Cin,3,3,3] weight, got {tuple(w.shape)}")
    wf = w.detach().float().contiguous()
    cout, cin = int(wf.shape[0]), int(wf.shape[1])
    img = torch.empty(packed_bytes(cout, cin), dtype=torch.uint8, device=wf.device)
    _lib.check(_lib.lib().gvf_conv3d3_pack(_lib.ptr(wf), cout, cin, dt_code(dtype), _lib.ptr(img), img.numel(), _stream(wf)), "gvf_conv3d3_pack")
    return img


def conv3(x: torch.Tensor, grid, wimg: torch.Tensor, cin: int, cout: int, bias=None, addend=None, out_dtype=torch.float32, store: str = "rows",
          out: torch.Tensor = None) -> torch.Tensor:
    """x 16-bit [B*X*Y*Z, ld_in] with ld_in >= roundup32(cin) and zeros in the columns cin .. roundup32(cin) (they are read); grid = (B, X, Y,
    Z); wimg from pack_weight in x's type -> fp32 (out_dtype=torch.float32) or x's 16-bit type: [rows, cout], or under store="shuffle2"
    [8 rows, cout / 8] on the (B, 2X, 2Y, 2Z) grid.  bias fp32 [cout]; addend fp32 in the output's shape; both optional."""
    _lib.require_cuda(x, wimg, bias, addend, out)
    B, X, Y, Z = (int(v) for v in grid)
    rows = B * X * Y * Z
    if x.dim() != 2 or x.stride(1) != 1 or int(x.shape[0]) != rows:
        raise ValueError(f"conv3d: the operand must be 16-bit rows [{rows}, ld] of the grid {(B, X, Y, Z)}, got {tuple(x.shape)}")
    if store not in ("rows", "shuffle2"):
        raise ValueError(f"conv3d: store is 'rows' or 'shuffle2', not {store!r}")
    cin, cout = int(cin), int(cout)
    ld_in = int(x.stride(0))
    if int(x.shape[1]) < (cin + 31) // 32 * 32:
        raise ValueError(f"conv3d: the operand rows hold {int(x.shape[1])} columns, fewer than {cin} padded to a multiple of 32")
    dt = dt_code(x.dtype)
    if wimg.numel() != packed_bytes(cout, cin):
        raise ValueError(f"conv3d: the weight image has {wimg.numel()} bytes, not those of a {cout} x {cin} x 27 weight")
    if out_dtype not in (torch.float32, x.dtype):
        raise ValueError(f"conv3d: the output is fp32 or the operand's type {x.dtype}, not {out_dtype}")
    if store == "shuffle2" and cout % 8:
        raise ValueError(f"conv3d: the shuffle2 store needs a multiple of 8 output channels, got {cout}")
    shape = (rows * 8, cout // 8) if store == "shuffle2" else (rows, cout)
    if bias is not None and (bias.dtype != torch.float32 or bias.numel() != cout or not bias.is_contiguous()):
        raise ValueError(f"conv3d: bias must hold {cout} fp32 values")
    if addend is not None and (addend.dtype != torch.float32 or tuple(addend.shape) != shape or not addend.is_contiguous()):
        raise ValueError(f"conv3d: the addend must be a contiguous fp32 {list(shape)} tensor")
    if out is None:
        out = torch.empty(shape, dtype=out_dtype, device=x.device)
    elif out.dtype != out_dtype or tuple(out.shape) != shape or not out.is_contiguous():
        raise ValueError(f"conv3d: out must be a contiguous {out_dtype} {list(shape)} tensor")
    _lib.check(_lib.lib().gvf_conv3d3(_lib.ptr(x), ld_in, _lib.ptr(wimg), _lib.ptr(bias), _lib.ptr(addend), _lib.ptr(out),
                                      int(out_dtype == torch.float32), STORE_SHUFFLE2 if store == "shuffle2" else STORE_ROWS, B, X, Y, Z, cin, cout,
                                      dt, _stream(x)), "gvf_conv3d3")
    return out


def occupancy_workspace_bytes(cells: int) -> int:
    return _util.workspace_bytes("gvf_occupancy_workspace_bytes", int(cells))


def occupancy_coords(logits: torch.Tensor, grid) -> torch.Tensor:
    """fp32 logits of the (B, X, Y, Z) grid in row order (any shape with B*X*Y*Z elements) -> int32 [n,4] = (b, x, y, z) of the cells with
    logit > 0, ascending by row: torch.argwhere(dense > 0)[:, [0, 2, 3, 4]].  Reads the count back once (the result's length)."""
    _lib.require_cuda(logits)
    B, X, Y, Z = (int(v) for v in grid)
    cells = B * X * Y * Z
    if logits.dtype != torch.float32 or logits.numel() != cells or not logits.is_contiguous():
        raise ValueError(f"conv3d: occupancy takes {cells} contiguous fp32 logits for the grid {(B, X, Y, Z)}, got {logits.dtype} {tuple(logits.shape)}")
    ws = _util.scratch("gvf_occupancy_workspace_bytes", logits.device, cells)
    coords = torch.empty((cells, 4), dtype=torch.int32, device=logits.device)
    count = torch.empty(1, dtype=torch.int32, device=logits.device)
    _lib.check(_lib.lib().gvf_occupancy_coords(_lib.ptr(logits), B, X, Y, Z, _lib.ptr(coords), cells, _lib.ptr(count), _lib.ptr(ws), ws.numel(),
                                               _stream(logits)), "gvf_occupancy_coords")
    return coords[:int(count.item())]
