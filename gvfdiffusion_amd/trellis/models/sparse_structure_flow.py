"""SparseStructureFlowModel (trellis/models/sparse_structure_flow.py:55-200) and the dense ModulatedTransformerCrossBlock
(trellis/modules/transformer/modulated.py:76-156): the rectified-flow model over the dense sparse-structure latent (16^3 x 8 in the released
pipeline), conditioned on image tokens -- on the gfx950 operators.  Constructors and the parameter tree are the reference's (`pos_emb` is a
registered buffer, as there), so its state dicts load strictly.  Inference only; pe_mode="rope", share_mod=True and attn_mode="windowed" are
not built.

Route.  Patchify and unpatchify are reshapes (plumbing).  The tokens of all samples are one row matrix (B L, C), sample b the rows
[b L, (b + 1) L): input_layer (GEMM, fp32 out) + pos_emb -> the blocks -> non-affine LayerNorm (eps 1e-5) -> out_layer.  The block IS the
route of ModulatedSparseTransformerCrossBlock over equal-length sequences (structured_latent_flow.py: forward_seqs): modulated LayerNorm ->
to_qkv -> varlen attention with the QK-RMSNorm gains fused -> to_out with the gate in the GEMM epilogue -> affine LayerNorm -> cross
attention (the context's to_kv is projected once per block and condition tensor and reused across sampler steps) -> MLP with the gate in
the epilogue.  `ops` is the operator seam of structured_latent_flow.py (None = HipOps); `taps` receives the per-stage rows."""
from typing import *

import torch
import torch.nn as nn

from ...model.sparse_voxel_diffusion.sparse_transformer import AbsolutePositionEmbedder
from ...ops import precision
from .structured_latent_flow import HipOps, ModulatedSparseTransformerCrossBlock, TimestepEmbedder

__all__ = ["ModulatedTransformerCrossBlock", "SparseStructureFlowModel", "patchify", "unpatchify"]


def patchify(x: torch.Tensor, p: int) -> torch.Tensor:
    """(B, C, X, Y, Z) -> (B, C p^3, X / p, Y / p, Z / p): channel ((c p + i) p + j) p + k of cell (x, y, z) is x[b, c, x p + i, y p + j, z p + k]."""
    B, C, X, Y, Z = x.shape
    assert X % p == 0 and Y % p == 0 and Z % p == 0, f"the spatial sizes {(X, Y, Z)} must be divisible by the patch size {p}"
    v = x.reshape(B, C, X // p, p, Y // p, p, Z // p, p).permute(0, 1, 3, 5, 7, 2, 4, 6)
    return v.reshape(B, C * p ** 3, X // p, Y // p, Z // p)


def unpatchify(x: torch.Tensor, p: int) -> torch.Tensor:
    """The inverse of patchify."""
    B, Cp, X, Y, Z = x.shape
    assert Cp % p ** 3 == 0
    v = x.reshape(B, Cp // p ** 3, p, p, p, X, Y, Z).permute(0, 1, 5, 2, 6, 3, 7, 4)
    return v.reshape(B, Cp // p ** 3, X * p, Y * p, Z * p)


class ModulatedTransformerCrossBlock(ModulatedSparseTransformerCrossBlock):
    """The dense block: the sparse block's parameters and route (forward_seqs), called with equal-length sequences."""

    def __init__(self, channels: int, ctx_channels: int, num_heads: int, mlp_ratio: float = 4.0, attn_mode: str = "full",
                 window_size: Optional[int] = None, shift_window: Optional[Tuple[int, int, int]] = None, use_checkpoint: bool = False,
                 use_rope: bool = False, qk_rms_norm: bool = False, qk_rms_norm_cross: bool = False, qkv_bias: bool = True,
                 share_mod: bool = False):
        if attn_mode == "windowed":
            raise NotImplementedError("attn_mode='windowed' is not built: the sparse-structure flow model attends over the full grid")
        super().__init__(channels, ctx_channels, num_heads, mlp_ratio=mlp_ratio, attn_mode=attn_mode, window_size=window_size,
                         shift_window=shift_window, use_checkpoint=use_checkpoint, use_rope=use_rope, qk_rms_norm=qk_rms_norm,
                         qk_rms_norm_cross=qk_rms_norm_cross, qkv_bias=qkv_bias, share_mod=share_mod)

    @torch.no_grad()
    def forward(self, x: torch.Tensor, mod: torch.Tensor, context: torch.Tensor, ops=None) -> torch.Tensor:
        """x: (B, L, C); mod: t_emb (B, C) as the reference's block takes it (the SiLU of adaLN_modulation is applied here)."""
        ops = HipOps(precision.resolve(None, (x,))) if ops is None else ops
        B, L, C = x.shape
        seqs, cu = _equal_seqs(B, L, x.device)
        rows = self.forward_seqs(x.reshape(B * L, C).float().contiguous().clone(), seqs, cu, L, torch.nn.functional.silu(mod.float()).contiguous(),
                                 context, ops)
        return rows.reshape(B, L, C).to(x.dtype)


def _equal_seqs(B: int, L: int, device):
    return [slice(b * L, (b + 1) * L) for b in range(B)], torch.arange(0, (B + 1) * L, L, dtype=torch.int32, device=device)


class SparseStructureFlowModel(nn.Module):
    def __init__(self, resolution: int, in_channels: int, model_channels: int, cond_channels: int, out_channels: int, num_blocks: int,
                 num_heads: Optional[int] = None, num_head_channels: Optional[int] = 64, mlp_ratio: float = 4, patch_size: int = 2,
                 pe_mode: str = "ape", use_fp16: bool = False, use_checkpoint: bool = False, share_mod: bool = False,
                 qk_rms_norm: bool = False, qk_rms_norm_cross: bool = False):
        super().__init__()
        if pe_mode not in ("ape", "rope"):
            raise ValueError(f"unknown pe_mode {pe_mode}")
        if pe_mode == "rope":
            raise NotImplementedError("RoPE is not built")
        if share_mod:
            raise NotImplementedError("share_mod=True is not built")
        self.resolution = resolution
        self.in_channels = in_channels
        self.model_channels = model_channels
        self.cond_channels = cond_channels
        self.out_channels = out_channels
        self.num_blocks = num_blocks
        self.num_heads = num_heads or model_channels // num_head_channels
        self.mlp_ratio = mlp_ratio
        self.patch_size = patch_size
        self.pe_mode = pe_mode
        self.use_fp16 = use_fp16
        self.use_checkpoint = use_checkpoint
        self.share_mod = share_mod
        self.qk_rms_norm = qk_rms_norm
        self.qk_rms_norm_cross = qk_rms_norm_cross
        self.dtype = torch.float16 if use_fp16 else torch.float32

        self.t_embedder = TimestepEmbedder(model_channels)
        r = resolution // patch_size
        coords = torch.stack(torch.meshgrid(*[torch.arange(r) for _ in range(3)], indexing="ij"), dim=-1).reshape(-1, 3)
        self.register_buffer("pos_emb", AbsolutePositionEmbedder(model_channels, 3)(coords))
        self.input_layer = nn.Linear(in_channels * patch_size ** 3, model_channels)
        self.blocks = nn.ModuleList([
            ModulatedTransformerCrossBlock(model_channels, cond_channels, num_heads=self.num_heads, mlp_ratio=self.mlp_ratio, attn_mode="full",
                                           use_checkpoint=self.use_checkpoint, use_rope=False, share_mod=False, qk_rms_norm=self.qk_rms_norm,
                                           qk_rms_norm_cross=self.qk_rms_norm_cross)
            for _ in range(num_blocks)])
        self.out_layer = nn.Linear(model_channels, out_channels * patch_size ** 3)
        self.compute_dtype = None
        self._wcache = {}
        self.initialize_weights()

    @property
    def device(self) -> torch.device:
        return next(self.parameters()).device

    def set_compute_dtype(self, dtype):
        """torch.float16 / torch.bfloat16 (or "fp16" / "bf16"); None hands the choice back to ops/precision.py."""
        self.compute_dtype = precision.parse(dtype)
        return self

    def _lp(self):
        return precision.resolve(self.compute_dtype, (), torch.float16 if self.use_fp16 else torch.bfloat16)

    def convert_to_fp16(self) -> None:
        """The parameters stay fp32 (cast once per version); from here on the kernels contract fp16 operands."""
        self.use_fp16, self.dtype = True, torch.float16

    def convert_to_fp32(self) -> None:
        self.use_fp16, self.dtype = False, torch.float32

    def initialize_weights(self) -> None:
        for m in self.modules():
            if isinstance(m, nn.Linear):
                nn.init.xavier_uniform_(m.weight)
                if m.bias is not None:
                    nn.init.constant_(m.bias, 0)
        nn.init.normal_(self.t_embedder.mlp[0].weight, std=0.02)
        nn.init.normal_(self.t_embedder.mlp[2].weight, std=0.02)
        for block in self.blocks:
            nn.init.constant_(block.adaLN_modulation[-1].weight, 0)
            nn.init.constant_(block.adaLN_modulation[-1].bias, 0)
        nn.init.constant_(self.out_layer.weight, 0)
        nn.init.constant_(self.out_layer.bias, 0)

    @torch.no_grad()
    def forward(self, x: torch.Tensor, t: torch.Tensor, cond: torch.Tensor, ops=None, taps: Optional[dict] = None) -> torch.Tensor:
        """x: (B, in_channels, R, R, R); t: (B,) timesteps (the sampler's 1000 t); cond: (B, L, cond_channels) -> (B, out_channels, R, R, R)
        in x's type.  ops: None = the HIP operators.  taps: a dict that receives the per-stage rows ("input", "block<i>_self", ...)."""
        R, p = self.resolution, self.patch_size
        assert [*x.shape] == [x.shape[0], self.in_channels, R, R, R], \
            f"Input shape mismatch, got {x.shape}, expected {[x.shape[0], self.in_channels, R, R, R]}"
        ops = HipOps(self._lp(), self._wcache) if ops is None else ops
        tap = (lambda name, v: taps.__setitem__(name, v.clone())) if taps is not None else (lambda name, v: None)
        B, r = x.shape[0], R // p
        L = r ** 3
        tokens = patchify(x, p).reshape(B, -1, L).permute(0, 2, 1).reshape(B * L, -1)
        rows = ops.linear(ops.cast(tokens), self.input_layer, "f32")
        rows = rows + self.pos_emb.to(rows.dtype).repeat(B, 1)
        tap("input", rows)
        emb_silu = ops.timestep(t, self.t_embedder)
        seqs, cu = _equal_seqs(B, L, x.device)
        for i, block in enumerate(self.blocks):
            inner = [] if taps is not None else None
            rows = block.forward_seqs(rows, seqs, cu, L, emb_silu, cond, ops, inner)
            if inner:
                tap(f"block{i}_self", inner[0])
                tap(f"block{i}_cross", inner[1])
            tap(f"block{i}", rows)
        hb = ops.ln(rows, 1e-5)                                   # F.layer_norm's default eps, no affine
        out = ops.linear(hb, self.out_layer, "f32")
        tap("out", out)
        out = out.reshape(B, L, -1).permute(0, 2, 1).reshape(B, -1, r, r, r)
        return unpatchify(out, p).contiguous().to(x.dtype)
