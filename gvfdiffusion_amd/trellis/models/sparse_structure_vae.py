"""SparseStructureDecoder (trellis/models/sparse_structure_vae.py:210-306) with its ResBlock3d and UpsampleBlock3d (:22-47, :75-98): the
dense 3-D convolutional decoder that takes the sparse-structure latent (16^3 x 8 in the released pipeline) to occupancy logits (64^3) --
on the gfx950 operators.  Constructors and the parameter tree are the reference's, so its state dicts load strictly.  Inference only;
norm_type="group", UpsampleBlock3d(mode="nearest") and the encoder are not built.

Route.  A dense volume is a row matrix (B X Y Z, C), row = ((b X + x) Y + y) Z + z -- the rows of a SparseTensor over the full grid in grid
order.  The residual stream is fp32 rows; every convolution operand is 16-bit (`use_fp16` / ops/precision.py choose fp16 or bf16):

  residual block   ln_act(norm1 affine, SiLU) -> conv1 (fp32 out) -> ln_act(norm2 affine, SiLU) -> conv2 with the block's input added in
                   the convolution's epilogue (ChannelLayerNorm32 is an affine LayerNorm over the channels, eps 1e-5: gvf_ln_act_rows)
  up-sampling      cast -> conv (C -> 8 C') whose store is pixel_shuffle_3d(., 2): the fp32 rows of the (2X, 2Y, 2Z) grid, written once
  out layer        ln_act(affine, SiLU) -> conv (C -> out_channels) as fp32 logits

HipOps.dense_conv3 sends the wide convolutions of large grids (both channel counts multiples of 64, a launch that fills the card) through
the submanifold kernel on the full grid's neighbour map, where it measured faster; the operator is the same.

`forward(x)` takes and returns the reference's (B, C, X, Y, Z) tensors; `forward_rows` is the rows-level entry the pipeline uses.  `ops` is
the operator seam of structured_latent_flow.py (None = HipOps); `taps` receives the per-stage rows."""
from typing import *

import torch
import torch.nn as nn

from ...ops import precision
from .structured_latent_flow import ACT_SILU, HipOps

__all__ = ["ChannelLayerNorm32", "ResBlock3d", "UpsampleBlock3d", "SparseStructureDecoder", "SparseStructureEncoder", "to_rows", "to_dense"]


def to_rows(x: torch.Tensor) -> torch.Tensor:
    """(B, C, X, Y, Z) -> (B X Y Z, C)."""
    return x.permute(0, 2, 3, 4, 1).reshape(-1, x.shape[1]).contiguous()


def to_dense(rows: torch.Tensor, grid) -> torch.Tensor:
    """(B X Y Z, C) -> (B, C, X, Y, Z)."""
    B, X, Y, Z = grid
    return rows.reshape(B, X, Y, Z, rows.shape[1]).permute(0, 4, 1, 2, 3).contiguous()


class ChannelLayerNorm32(nn.LayerNorm):
    """The parameter holder of the reference's channel LayerNorm (weight, bias over C, eps 1e-5); computed on rows by ops.ln."""


def norm_layer(norm_type: str, channels: int) -> nn.Module:
    if norm_type == "group":
        raise NotImplementedError("norm_type='group' is not built: the released sparse-structure decoder uses 'layer'")
    if norm_type != "layer":
        raise ValueError(f"Invalid norm type {norm_type}")
    return ChannelLayerNorm32(channels)


class ResBlock3d(nn.Module):
    def __init__(self, channels: int, out_channels: Optional[int] = None, norm_type: str = "layer"):
        super().__init__()
        self.channels = channels
        self.out_channels = out_channels or channels
        self.norm1 = norm_layer(norm_type, channels)
        self.norm2 = norm_layer(norm_type, self.out_channels)
        self.conv1 = nn.Conv3d(channels, self.out_channels, 3, padding=1)
        self.conv2 = nn.Conv3d(self.out_channels, self.out_channels, 3, padding=1)
        for p in self.conv2.parameters():
            nn.init.zeros_(p)
        self.skip_connection = nn.Conv3d(channels, self.out_channels, 1) if channels != self.out_channels else nn.Identity()

    def forward_rows(self, x: torch.Tensor, grid, ops, taps=None) -> torch.Tensor:
        """x: fp32 rows (B X Y Z, channels) of `grid` -> fp32 rows (B X Y Z, out_channels)."""
        if not isinstance(self.skip_connection, nn.Identity):
            raise NotImplementedError("ResBlock3d with a 1x1x1 skip convolution is not built: the decoder's blocks keep their channel count")
        h16 = ops.ln(x, self.norm1.eps, self.norm1.weight, self.norm1.bias, act=ACT_SILU)
        h = ops.dense_conv3(h16, grid, self.conv1)
        if taps is not None:
            taps.append(h)
        h16 = ops.ln(h, self.norm2.eps, self.norm2.weight, self.norm2.bias, act=ACT_SILU)
        return ops.dense_conv3(h16, grid, self.conv2, addend=x)


class UpsampleBlock3d(nn.Module):
    def __init__(self, in_channels: int, out_channels: int, mode: str = "conv"):
        assert mode in ["conv", "nearest"], f"Invalid mode {mode}"
        super().__init__()
        if mode == "nearest":
            raise NotImplementedError("UpsampleBlock3d(mode='nearest') is not built: the decoder up-samples by convolution + pixel shuffle")
        self.in_channels = in_channels
        self.out_channels = out_channels
        self.conv = nn.Conv3d(in_channels, out_channels * 8, 3, padding=1)

    def forward_rows(self, x: torch.Tensor, grid, ops):
        """x: fp32 rows of `grid` -> (fp32 rows (8 B X Y Z, out_channels), the (B, 2X, 2Y, 2Z) grid)."""
        B, X, Y, Z = grid
        return ops.dense_conv3(ops.cast(x), grid, self.conv, store="shuffle2"), (B, 2 * X, 2 * Y, 2 * Z)


class SparseStructureEncoder(nn.Module):
    def __init__(self, *args, **kwargs):
        super().__init__()
        raise NotImplementedError("SparseStructureEncoder is not built: inference starts from the flow model's latent")


class SparseStructureDecoder(nn.Module):
    def __init__(self, out_channels: int, latent_channels: int, num_res_blocks: int, channels: List[int], num_res_blocks_middle: int = 2,
                 norm_type: str = "layer", use_fp16: bool = False):
        super().__init__()
        self.out_channels = out_channels
        self.latent_channels = latent_channels
        self.num_res_blocks = num_res_blocks
        self.channels = channels
        self.num_res_blocks_middle = num_res_blocks_middle
        self.norm_type = norm_type
        self.use_fp16 = use_fp16
        self.dtype = torch.float16 if use_fp16 else torch.float32
        if any(c % 32 for c in channels):
            raise NotImplementedError(f"the decoder's channel counts must be multiples of 32 (the convolution reads whole 32-channel chunks), got {channels}")

        self.input_layer = nn.Conv3d(latent_channels, channels[0], 3, padding=1)
        self.middle_block = nn.Sequential(*[ResBlock3d(channels[0], channels[0], norm_type) for _ in range(num_res_blocks_middle)])
        self.blocks = nn.ModuleList([])
        for i, ch in enumerate(channels):
            self.blocks.extend([ResBlock3d(ch, ch, norm_type) for _ in range(num_res_blocks)])
            if i < len(channels) - 1:
                self.blocks.append(UpsampleBlock3d(ch, channels[i + 1]))
        self.out_layer = nn.Sequential(norm_layer(norm_type, channels[-1]), nn.SiLU(), nn.Conv3d(channels[-1], out_channels, 3, padding=1))
        self.compute_dtype = None
        self._wcache = {}

    @property
    def device(self) -> torch.device:
        return next(self.parameters()).device

    @property
    def upsample_factor(self) -> int:
        return 2 ** (len(self.channels) - 1)

    def set_compute_dtype(self, dtype):
        """torch.float16 / torch.bfloat16 (or "fp16" / "bf16"); None hands the choice back to ops/precision.py."""
        self.compute_dtype = precision.parse(dtype)
        return self

    def _lp(self):
        return precision.resolve(self.compute_dtype, (), torch.float16 if self.use_fp16 else torch.bfloat16)

    def convert_to_fp16(self) -> None:
        """The parameters stay fp32 (packed once per version); from here on the kernels contract fp16 operands."""
        self.use_fp16, self.dtype = True, torch.float16

    def convert_to_fp32(self) -> None:
        self.use_fp16, self.dtype = False, torch.float32

    @torch.no_grad()
    def forward_rows(self, z: torch.Tensor, grid, ops=None, taps: Optional[dict] = None):
        """z: rows (B X Y Z, latent_channels) of `grid` = (B, X, Y, Z) -> (fp32 logit rows (B fX fY fZ, out_channels), the output grid), f =
        upsample_factor.  taps: a dict that receives the per-stage rows ("input", "middle<i>", "block<i>", their "_conv1", "logits")."""
        ops = HipOps(self._lp(), self._wcache) if ops is None else ops
        tap = (lambda name, v: taps.__setitem__(name, v.clone())) if taps is not None else (lambda name, v: None)
        grid = tuple(int(v) for v in grid)
        h = ops.dense_conv3(ops.cast(z), grid, self.input_layer)
        tap("input", h)
        stages = [(f"middle{i}", b) for i, b in enumerate(self.middle_block)] + [(f"block{i}", b) for i, b in enumerate(self.blocks)]
        for name, block in stages:
            if isinstance(block, UpsampleBlock3d):
                h, grid = block.forward_rows(h, grid, ops)
            else:
                inner = [] if taps is not None else None
                h = block.forward_rows(h, grid, ops, inner)
                if inner:
                    tap(name + "_conv1", inner[0])
            tap(name, h)
        norm, conv = self.out_layer[0], self.out_layer[2]
        logits = ops.dense_conv3(ops.ln(h, norm.eps, norm.weight, norm.bias, act=ACT_SILU), grid, conv)
        tap("logits", logits)
        return logits, grid

    @torch.no_grad()
    def forward(self, x: torch.Tensor, ops=None, taps: Optional[dict] = None) -> torch.Tensor:
        """x: (B, latent_channels, X, Y, Z) -> (B, out_channels, fX, fY, fZ) logits in x's type."""
        grid = (x.shape[0], x.shape[2], x.shape[3], x.shape[4])
        logits, grid = self.forward_rows(to_rows(x).float(), grid, ops, taps)
        return to_dense(logits, grid).to(x.dtype)
