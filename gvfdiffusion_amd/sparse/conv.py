"""SparseConv3d (trellis/modules/sparse/conv/conv_spconv.py:7-49): the submanifold case of the reference's spconv wrapper -- kernel size 3
(or 1), stride 1, dilation 1, padding None, i.e. spconv.SubMConv3d -- on the HIP operator of ops/spconv.py.  The parameters live on a child
named `conv` with spconv 2's shapes (`conv.weight [out, k, k, k, in]`, `conv.bias [out]`), so the reference's state-dict keys load strictly.
Strided / dilated / padded convolutions and SparseInverseConv3d are not built and say so.

The neighbour map depends on the coordinates alone: it is cached on the tensor's spatial cache under the tensor's scale, and `replace()`
carries the cache, so a sampler that keeps its coordinates builds one map per resolution, not one per step or layer."""
import math

import torch
import torch.nn as nn

from .basic import SparseTensor
from .linear import linear_rows
from ..ops import precision, spconv

__all__ = ["SparseConv3d", "SparseInverseConv3d", "neighbor_map"]

NBR_KEY = "spconv3_neighbor_map"


def neighbor_map(x: SparseTensor, build=None) -> torch.Tensor:
    """int32 [T,27] of `x`, built once per set of coordinates.  build: the map builder (default ops.spconv.build_neighbor_map).

    The spatial cache is keyed by the tensor's scale, and the scale arithmetic of sparse/spatial.py (the reference's: 1 // 2 = 0, 0 * 2 = 0)
    gives the rows that come back from SparseUpsample the scale of the downsampled ones; the entry is therefore also keyed by the number
    of rows, holds the coordinates it was built from, and is looked up under every scale of the cache.  The same coordinate tensor (replace() and SparseUpsample hand it on) is a hit
    by identity; an equal tensor of another identity (SparseDownsample makes a new one per call) is a hit after one comparison, and
    becomes the entry's tensor, so that the other convolutions of that call hit by identity."""
    key = f"{NBR_KEY}_{x.coords.shape[0]}"
    hit = x.get_spatial_cache(key)
    if hit is None:                                           # the same rows under another scale (before the down / up sampling pair)
        hit = next((per_scale[key] for per_scale in x._spatial_cache.values() if key in per_scale), None)
    if hit is not None and hit[0] is x.coords:
        x.register_spatial_cache(key, hit)
    elif hit is not None:
        same = hit[0].shape == x.coords.shape and hit[0].device == x.coords.device and bool(torch.equal(hit[0], x.coords))
        hit = (x.coords, hit[1]) if same else None
        if same:
            x.register_spatial_cache(key, hit)
    if hit is None:
        hit = (x.coords, (build or spconv.build_neighbor_map)(x.coords))
        x.register_spatial_cache(key, hit)
    return hit[1]


class _SubMConv3dParams(nn.Module):
    """The parameter holder spconv.SubMConv3d is in the reference: weight [out, k, k, k, in], bias [out]; its default initialisation
    (kaiming-uniform with a = sqrt(5) over fan_in = k^3 in, the bias uniform in +- 1 / sqrt(fan_in))."""

    def __init__(self, in_channels, out_channels, kernel_size, bias):
        super().__init__()
        self.in_channels, self.out_channels, self.kernel_size = in_channels, out_channels, (kernel_size,) * 3
        self.weight = nn.Parameter(torch.empty((out_channels, kernel_size, kernel_size, kernel_size, in_channels)))
        self.bias = nn.Parameter(torch.empty(out_channels)) if bias else None
        bound = 1.0 / math.sqrt(in_channels * kernel_size ** 3)
        nn.init.uniform_(self.weight, -bound, bound)
        if bias:
            nn.init.uniform_(self.bias, -bound, bound)


class _LinearView:
    """What sparse/linear.py's linear_rows reads of an nn.Linear, over the parameters of a 1x1x1 convolution (the 16-bit copy of the
    weight is cached on the parameter holder, per parameter version)."""

    def __init__(self, conv: _SubMConv3dParams):
        self.__dict__ = conv.__dict__.setdefault("_gvf_linear_view", {})
        self.weight = conv.weight.detach().reshape(conv.out_channels, conv.in_channels)
        self.bias = None if conv.bias is None else conv.bias.detach()
        self.in_features, self.out_features = conv.in_channels, conv.out_channels


class SparseConv3d(nn.Module):
    def __init__(self, in_channels, out_channels, kernel_size, stride=1, dilation=1, padding=None, bias=True, indice_key=None):
        super().__init__()
        stride3 = tuple(stride) if isinstance(stride, (list, tuple)) else (stride,) * 3
        dil3 = tuple(dilation) if isinstance(dilation, (list, tuple)) else (dilation,) * 3
        if any(s != 1 for s in stride3) or padding is not None:
            raise NotImplementedError("SparseConv3d: only the submanifold convolution (stride 1, padding None) is built; the strided / "
                                      "padded spconv.SparseConv3d is not")
        if any(d != 1 for d in dil3):
            raise NotImplementedError("SparseConv3d: dilation other than 1 is not built")
        if isinstance(kernel_size, (list, tuple)):
            if len(set(kernel_size)) != 1:
                raise NotImplementedError("SparseConv3d: only cubic kernels (3 or 1) are built")
            kernel_size = kernel_size[0]
        if kernel_size not in (1, 3):
            raise NotImplementedError(f"SparseConv3d: kernel_size {kernel_size} is not built (3: the HIP submanifold convolution, 1: a linear)")
        self.conv = _SubMConv3dParams(in_channels, out_channels, kernel_size, bias)
        self.stride, self.padding, self.indice_key = stride3, padding, indice_key
        self._packed = {}

    def packed(self, lp):
        """(weight image or [out, in] 16-bit matrix, fp32 bias) for the operand type `lp`: packed once per parameter version."""
        w, b = self.conv.weight, self.conv.bias
        ver = (w._version, w.data_ptr(), w.device, None if b is None else (b._version, b.data_ptr()))
        hit = self._packed.get(lp)
        if hit is None or hit[0] != ver:
            bias = None if b is None else b.detach().float().contiguous()
            hit = self._packed[lp] = (ver, spconv.pack_weight(w, lp), bias)
        return hit[1], hit[2]

    def forward_rows(self, x16: torch.Tensor, st: SparseTensor, addend=None, out_dtype=torch.float32) -> torch.Tensor:
        """x16: 16-bit rows [T, in] of `st` -> [T, out] fp32 (or x16's type), with `addend` (fp32 [T, out]) added in the epilogue."""
        wimg, bias = self.packed(x16.dtype)
        return spconv.conv3(x16, neighbor_map(st), wimg, self.conv.out_channels, bias=bias, addend=addend, out_dtype=out_dtype,
                            cin=self.conv.in_channels)

    @torch.no_grad()
    def forward(self, x: SparseTensor) -> SparseTensor:
        if self.conv.kernel_size[0] == 1:                     # a 1x1x1 kernel is the existing linear over the rows
            return x.replace(linear_rows(_LinearView(self.conv), x.feats).to(x.dtype))
        cin = self.conv.in_channels
        if cin % 64 or self.conv.out_channels % 64 or cin > spconv.C_MAX or self.conv.out_channels > spconv.C_MAX:
            raise NotImplementedError(f"SparseConv3d: channel counts must be multiples of 64 up to {spconv.C_MAX}, got {cin} -> {self.conv.out_channels}")
        lp = precision.resolve(None, (x.feats,))
        return x.replace(self.forward_rows(x.feats.to(lp).contiguous(), x).to(x.dtype))


class SparseInverseConv3d(nn.Module):
    def __init__(self, *args, **kwargs):
        super().__init__()
        raise NotImplementedError("SparseInverseConv3d is not built: only the submanifold SparseConv3d (stride 1, padding None) is")
