"""SLatFlowModel (trellis/models/structured_latent_flow.py:14-262) and its modulated cross-attention block
(trellis/modules/sparse/transformer/modulated.py:81-166): the rectified-flow model that produces the structured latent -- sparse-structure
coordinates + image-condition tokens -> 8 channels per active voxel -- on the gfx950 operators.  Constructors and the parameter tree are
the reference's, so its state dicts load strictly.  Inference only; pe_mode="rope" and share_mod=True are not built.

Route.  The residual stream is fp32 rows (T, C); every matrix operand is 16-bit (`use_fp16` / ops/precision.py choose fp16 or bf16):

  residual block   ln_act(norm1 affine, SiLU) -> conv1 (fp32 out) -> ln_act(norm2, 1 + scale, shift, SiLU) -> conv2 with the skip path
                   (x itself, or one GEMM for `skip_connection`) added in the convolution's epilogue; emb_layers is one fp32 GEMV per call;
                   down / up sampling is sparse/spatial.py.
  transformer      layernorm_modulate -> to_qkv -> varlen attention with the QK-RMSNorm gains fused -> to_out with the gate in the GEMM
                   epilogue -> affine layernorm -> cross attention (the context's to_kv is projected once per block and condition tensor
                   and reused across sampler steps) -> MLP with the gate in the epilogue.

A kernel that takes one modulation row per group is called per sample slice, so ragged batches need no padding.  The neighbour maps are
cached on the tensor's spatial cache per scale (sparse/conv.py): one per resolution for a whole sampling run.

`forward(x, t, cond, ops=...)`: `ops` is the seam through which every operator is reached.  None = HipOps (the kernels); a namespace of the
same signatures on torch operators (tests/slat_flow_ref.py::TorchOps) runs the same route on the CPU for the host test and as the
benchmark's baseline."""
from typing import *

import numpy as np
import torch
import torch.nn as nn

from ... import sparse as sp
from ...model.sparse_voxel_diffusion.sparse_transformer import AbsolutePositionEmbedder, SparseFeedForward, token_partition
from ...ops import conv3d, dit_ops, precision, spconv
from ...sparse.attention.modules import SparseMultiHeadAttention
from ...sparse.conv import neighbor_map

__all__ = ["TimestepEmbedder", "SparseResBlock3d", "ModulatedSparseTransformerCrossBlock", "SLatFlowModel", "HipOps"]

ACT_NONE, ACT_SILU = spconv.ACT_NONE, spconv.ACT_SILU


class HipOps:
    """The operators of the route on the HIP kernels.  lp: the 16-bit operand type; cache: the dict that keeps the 16-bit weight copies
    (per parameter version) between calls -- the model's."""

    def __init__(self, lp, cache=None):
        self.lp = lp
        self.cache = {} if cache is None else cache

    def _w16(self, weight, bias):
        key = (id(weight), self.lp)
        ver = (weight._version, weight.data_ptr(), None if bias is None else (bias._version, bias.data_ptr()))
        hit = self.cache.get(key)
        if hit is None or hit[0] != ver:
            w = dit_ops.cast_pad(weight.detach().float().contiguous(), dit_ops.pad64(weight.shape[1]), dtype=self.lp)
            hit = self.cache[key] = (ver, w, None if bias is None else bias.detach().float().contiguous())
        return hit[1], hit[2]

    def _vec(self, v):
        return None if v is None else v.detach().float().contiguous()

    @staticmethod
    def neighbor_map(coords):
        return spconv.build_neighbor_map(coords)

    def timestep(self, t, embedder):
        """-> silu(TimestepEmbedder(t)), fp32 (B, C): what every SiLU -> Linear modulation head reads."""
        m0, m2 = embedder.mlp[0], embedder.mlp[2]
        return dit_ops.timestep_embed_f32(t.float().contiguous(), m0.weight.detach().float().contiguous(), self._vec(m0.bias),
                                          m2.weight.detach().float().contiguous(), self._vec(m2.bias), embedder.frequency_embedding_size)

    def modulation(self, s, lin):
        return dit_ops.modulation_f32(s, lin.weight.detach().float().contiguous(), self._vec(lin.bias))

    def cast(self, x):
        """fp32 rows -> 16-bit operand rows (columns zero-padded to a multiple of 64)."""
        return dit_ops.cast_pad(x.float().contiguous(), dit_ops.pad64(x.shape[1]), dtype=self.lp)

    def ln(self, x, eps, ln_w=None, ln_b=None, shift=None, scale=None, act=ACT_NONE, out=None):
        """fp32 rows -> 16-bit act(LN(x) [affine] [one shift / scale row])."""
        return spconv.ln_act(x, self._vec(ln_w), self._vec(ln_b), shift, scale, act, eps, self.lp, out)

    def linear(self, a16, lin, kind="f32"):
        """a16 @ W^T + b -> fp32 ("f32"), the operand type ("lp") or tanh-GELU in the operand type ("gelu")."""
        w, b = self._w16(lin.weight, lin.bias)
        out = torch.empty((a16.shape[0], lin.weight.shape[0]), dtype=torch.float32 if kind == "f32" else self.lp, device=a16.device)
        epi = {"f32": dit_ops.EPI_STORE_F32, "lp": dit_ops.EPI_STORE_16, "gelu": dit_ops.EPI_GELU_16}[kind]
        return dit_ops.gemm(a16, w, b, out, epi)

    def linear_resid(self, x, a16, lin, gate=None):
        """x (fp32 rows, in place) += gate * (a16 @ W^T + b); gate: ONE fp32 row or None."""
        w, b = self._w16(lin.weight, lin.bias)
        if gate is None:
            return dit_ops.gemm(a16, w, b, x, dit_ops.EPI_RESID_F32)
        return dit_ops.gemm(a16, w, b, x, dit_ops.EPI_RESID_F32, gate=gate, gate_ld=gate.numel(), rows_per_group=x.shape[0])

    def conv3(self, a16, nbr, conv, addend=None):
        """a16 16-bit rows, conv: a sparse.SparseConv3d -> fp32 rows, `addend` (fp32) added in the epilogue."""
        wimg, bias = conv.packed(self.lp)
        return spconv.conv3(a16, nbr, wimg, conv.conv.out_channels, bias=bias, addend=addend, cin=conv.conv.in_channels)

    def dense_conv3(self, a16, grid, conv, addend=None, store="rows"):
        """a16 16-bit rows of the dense (B, X, Y, Z) grid (zeros in the columns up to the next multiple of 32), conv: an nn.Conv3d(cin, cout,
        3, padding=1) -> fp32 rows, or under store="shuffle2" the fp32 rows of pixel_shuffle_3d(., 2); `addend` (fp32) added in the epilogue.
        The weight image is packed once per (module, operand type) and parameter version.

        Routing (measured): where both channel counts are multiples of 64 and the submanifold kernel's launch on these
        rows fills the card's 256 compute units, the convolution goes through gvf_spconv3 on the full grid's neighbour map (built once per
        grid) and the pixel-shuffle becomes a permuting copy; every other shape takes the dense kernel, shuffle in its store."""
        w, b = conv.weight, conv.bias
        cin, cout = conv.in_channels, conv.out_channels
        sub = self.spconv_route(a16.shape[0], cin, cout) and max(grid[1:]) <= 1024      # the neighbour map's coordinate range
        key = (id(w), self.lp, "spconv3" if sub else "conv3d")
        ver = (w._version, w.data_ptr(), None if b is None else (b._version, b.data_ptr()))
        hit = self.cache.get(key)
        if hit is None or hit[0] != ver:
            img = spconv.pack_weight(w.detach().permute(0, 2, 3, 4, 1).contiguous(), self.lp) if sub else conv3d.pack_weight(w, self.lp)
            hit = self.cache[key] = (ver, img, self._vec(b))
        if not sub:
            return conv3d.conv3(a16, grid, hit[1], cin, cout, bias=hit[2], addend=addend, store=store)
        nbr = self.full_grid_map(grid, a16.device)
        if store == "rows":
            return spconv.conv3(a16, nbr, hit[1], cout, bias=hit[2], addend=addend, cin=cin)
        B, X, Y, Z = grid
        y = spconv.conv3(a16, nbr, hit[1], cout, bias=hit[2], cin=cin).reshape(B, X, Y, Z, cout // 8, 2, 2, 2)
        y = y.permute(0, 1, 5, 2, 6, 3, 7, 4).reshape(8 * B * X * Y * Z, cout // 8)
        return y if addend is None else y + addend

    @staticmethod
    def spconv_route(rows, cin, cout):
        """Whether gvf_spconv3 takes this dense convolution: its workgroups (64 rows x 64, 128 or 256 channels) number at least 256."""
        if cin % 64 or cout % 64 or cin > spconv.C_MAX or cout > spconv.C_MAX:
            return False
        tile = 256 if cout % 256 == 0 else (128 if cout % 128 == 0 else 64)
        return (rows + 63) // 64 * (cout // tile) >= 256

    def full_grid_map(self, grid, device):
        """The neighbour map of the full (B, X, Y, Z) grid in row order, built once per grid and device."""
        key = ("full_grid_map", tuple(grid), str(device))
        hit = self.cache.get(key)
        if hit is None:
            B, X, Y, Z = grid
            ax = [torch.arange(n, dtype=torch.int32, device=device) for n in (B, X, Y, Z)]
            hit = self.cache[key] = spconv.build_neighbor_map(torch.stack(torch.meshgrid(*ax, indexing="ij"), dim=-1).reshape(-1, 4).contiguous())
        return hit

    @staticmethod
    def occupancy(logits, grid):
        """fp32 logits of the dense grid in row order -> int32 (n, 4) coordinates of the cells > 0, row order."""
        return conv3d.occupancy_coords(logits, grid)

    def attention(self, q, k, v, cu_q, cu_k, max_q, max_k, heads, gq=None, gk=None):
        """q (Tq, C), k, v (Tk, C): 16-bit row views with heads packed along C -> (Tq, C)."""
        C = q.shape[1]
        out = torch.empty((q.shape[0], C), dtype=self.lp, device=q.device)
        dit_ops.attention_varlen(q, k, v, out, cu_q, cu_k, max_q, max_k, heads, (0, 0, q.stride(0)), (0, 0, k.stride(0)),
                                 (0, 0, v.stride(0)), (0, 0, C), self._vec(gq), self._vec(gk), head_dim=C // heads)
        return out


class TimestepEmbedder(nn.Module):
    """Sinusoid -> Linear -> SiLU -> Linear (trellis/models/sparse_structure_flow.py:11-52); computed by the timestep kernel."""

    def __init__(self, hidden_size, frequency_embedding_size=256):
        super().__init__()
        self.mlp = nn.Sequential(nn.Linear(frequency_embedding_size, hidden_size, bias=True), nn.SiLU(),
                                 nn.Linear(hidden_size, hidden_size, bias=True))
        self.frequency_embedding_size = frequency_embedding_size


def _slices(st: sp.SparseTensor):
    return [sl for sl in st.layout if sl.stop > sl.start]


def _modulated_ln(ops, x, layout, eps, shift, scale, act=ACT_NONE):
    """LayerNorm with one (shift, scale) row per sample: per sample slice (layout: the samples' row slices)."""
    out = None
    for b, sl in enumerate(layout):
        if sl.stop == sl.start:
            continue
        part = ops.ln(x[sl], eps, None, None, shift[b], scale[b], act)
        if len(layout) == 1:
            return part
        if out is None:
            out = torch.empty((x.shape[0], part.shape[1]), dtype=part.dtype, device=part.device)
        out[sl] = part
    return out


class SparseResBlock3d(nn.Module):
    def __init__(self, channels: int, emb_channels: int, out_channels: Optional[int] = None, downsample: bool = False, upsample: bool = False):
        super().__init__()
        self.channels = channels
        self.emb_channels = emb_channels
        self.out_channels = out_channels or channels
        self.downsample = downsample
        self.upsample = upsample
        assert not (downsample and upsample), "Cannot downsample and upsample at the same time"
        self.norm1 = nn.LayerNorm(channels, elementwise_affine=True, eps=1e-6)
        self.norm2 = nn.LayerNorm(self.out_channels, elementwise_affine=False, eps=1e-6)
        self.conv1 = sp.SparseConv3d(channels, self.out_channels, 3)
        self.conv2 = sp.SparseConv3d(self.out_channels, self.out_channels, 3)
        for p in self.conv2.parameters():
            nn.init.zeros_(p)
        self.emb_layers = nn.Sequential(nn.SiLU(), nn.Linear(emb_channels, 2 * self.out_channels, bias=True))
        self.skip_connection = sp.SparseLinear(channels, self.out_channels) if channels != self.out_channels else nn.Identity()
        self.updown = None
        if self.downsample:
            self.updown = sp.SparseDownsample(2)
        elif self.upsample:
            self.updown = sp.SparseUpsample(2)

    def forward_rows(self, st: sp.SparseTensor, x: torch.Tensor, emb_silu: torch.Tensor, ops, taps=None):
        """st: the tensor whose rows x (fp32 (T, channels)) are; emb_silu: silu(t_emb) fp32 (B, emb_channels) -> (tensor, fp32 rows)."""
        emb = ops.modulation(emb_silu, self.emb_layers[1])
        scale, shift = emb[:, :self.out_channels], emb[:, self.out_channels:]
        if self.updown is not None:
            st = self.updown(st.replace(x))
            x = st.feats.contiguous()
        nbr = neighbor_map(st, ops.neighbor_map)
        h16 = ops.ln(x, self.norm1.eps, self.norm1.weight, self.norm1.bias, act=ACT_SILU)
        h = ops.conv3(h16, nbr, self.conv1)
        if taps is not None:
            taps.append(h)
        h16 = _modulated_ln(ops, h, st.layout, self.norm2.eps, shift, scale, ACT_SILU)
        skip = x if isinstance(self.skip_connection, nn.Identity) else ops.linear(ops.cast(x), self.skip_connection, "f32")
        return st, ops.conv3(h16, nbr, self.conv2, addend=skip)

    @torch.no_grad()
    def forward(self, x: sp.SparseTensor, emb: torch.Tensor, ops=None) -> sp.SparseTensor:
        """emb: t_emb (B, emb_channels), as the reference's block takes it (the SiLU of emb_layers is applied here)."""
        ops = HipOps(precision.resolve(None, (x.feats,))) if ops is None else ops
        st, rows = self.forward_rows(x, x.feats.float().contiguous(), torch.nn.functional.silu(emb.float()).contiguous(), ops)
        return st.replace(rows.to(x.dtype))


class ModulatedSparseTransformerCrossBlock(nn.Module):
    """Sparse transformer block (self attention + cross attention + MLP) with adaLN conditioning."""

    def __init__(self, channels: int, ctx_channels: int, num_heads: int, mlp_ratio: float = 4.0, attn_mode: str = "full",
                 window_size: Optional[int] = None, shift_sequence: Optional[int] = None, shift_window: Optional[Tuple[int, int, int]] = None,
                 serialize_mode=None, use_checkpoint: bool = False, use_rope: bool = False, qk_rms_norm: bool = False,
                 qk_rms_norm_cross: bool = False, qkv_bias: bool = True, share_mod: bool = False):
        super().__init__()
        if share_mod:
            raise NotImplementedError("share_mod=True is not built")
        if use_rope:
            raise NotImplementedError("RoPE is not built")
        if attn_mode != "full":
            raise NotImplementedError(f"the modulated cross block is built for full self attention (the flow model's), not {attn_mode!r}")
        self.use_checkpoint = use_checkpoint
        self.share_mod = share_mod
        self.channels, self.num_heads = channels, num_heads
        self.norm1 = nn.LayerNorm(channels, elementwise_affine=False, eps=1e-6)
        self.norm2 = nn.LayerNorm(channels, elementwise_affine=True, eps=1e-6)
        self.norm3 = nn.LayerNorm(channels, elementwise_affine=False, eps=1e-6)
        self.self_attn = SparseMultiHeadAttention(channels, num_heads=num_heads, type="self", attn_mode="full", qkv_bias=qkv_bias,
                                                  use_rope=use_rope, qk_rms_norm=qk_rms_norm)
        self.cross_attn = SparseMultiHeadAttention(channels, ctx_channels=ctx_channels, num_heads=num_heads, type="cross", attn_mode="full",
                                                   qkv_bias=qkv_bias, qk_rms_norm=qk_rms_norm_cross)
        self.mlp = SparseFeedForward(channels, mlp_ratio=mlp_ratio)
        self.adaLN_modulation = nn.Sequential(nn.SiLU(), nn.Linear(channels, 6 * channels, bias=True))
        self._kv = []                           # [(condition tensor, its version, ops key, kv rows, cu, longest)], most recent last
        self.kv_projections = 0                 # how often to_kv ran (a sampler: once per condition tensor)

    def context_kv(self, cond: torch.Tensor, ops):
        """cond (B, L, ctx_channels) -> (kv 16-bit (B L, 2 C), cu_seqlens, L): projected once per condition tensor and operator set."""
        a = self.cross_attn
        w = a.to_kv.weight
        key = (getattr(ops, "lp", None), type(ops).__name__, w._version, w.data_ptr())
        for c, ver, k, kv, cu, L in self._kv:
            if c is cond and ver == cond._version and k == key:
                return kv, cu, L
        B, L, Cc = cond.shape
        kv = ops.linear(ops.cast(cond.reshape(B * L, Cc)), a.to_kv, "lp")
        cu = torch.arange(0, (B + 1) * L, L, dtype=torch.int32, device=cond.device)
        self.kv_projections += 1
        self._kv = self._kv[-3:] + [(cond, cond._version, key, kv, cu, L)]
        return kv, cu, L

    def forward_rows(self, x: torch.Tensor, st: sp.SparseTensor, emb_silu: torch.Tensor, cond: torch.Tensor, ops, taps=None):
        """x: fp32 (T, C) residual rows of `st`, updated in place and returned."""
        _, _, cu, longest = token_partition(st, "full", None, None, None, None)
        return self.forward_seqs(x, st.layout, cu, longest, emb_silu, cond, ops, taps)

    def forward_seqs(self, x: torch.Tensor, seqs: List[slice], cu: torch.Tensor, longest: int, emb_silu: torch.Tensor, cond: torch.Tensor, ops,
                     taps=None):
        """x: fp32 (T, C) residual rows, sample b's sequence the rows seqs[b]; cu: int32 cu_seqlens of the non-empty sequences, longest: the
        longest of them.  Updated in place and returned.  The dense flow model calls this with equal-length sequences."""
        C, H = self.channels, self.num_heads
        mod = ops.modulation(emb_silu, self.adaLN_modulation[1])                # (B, 6 C): shift, scale, gate of the attention, of the MLP
        m = [mod[:, i * C:(i + 1) * C] for i in range(6)]
        sa, ca = self.self_attn, self.cross_attn
        gains = lambda a: (a.q_rms_norm.gamma, a.k_rms_norm.gamma) if a.qk_rms_norm else (None, None)
        layout = [(b, sl) for b, sl in enumerate(seqs) if sl.stop > sl.start]

        hb = _modulated_ln(ops, x, seqs, self.norm1.eps, m[0], m[1])
        qkv = ops.linear(hb, sa.to_qkv, "lp")
        ao = ops.attention(qkv[:, :C], qkv[:, C:2 * C], qkv[:, 2 * C:], cu, cu, longest, longest, H, *gains(sa))
        for b, sl in layout:
            ops.linear_resid(x[sl], ao[sl], sa.to_out, m[2][b])
        if taps is not None:
            taps.append(x.clone())

        hb = ops.ln(x, self.norm2.eps, self.norm2.weight, self.norm2.bias)
        q = ops.linear(hb, ca.to_q, "lp")
        kv, cu_k, longest_k = self.context_kv(cond, ops)
        ao = ops.attention(q, kv[:, :C], kv[:, C:], cu, cu_k, longest, longest_k, H, *gains(ca))
        ops.linear_resid(x, ao, ca.to_out, None)
        if taps is not None:
            taps.append(x.clone())

        hb = _modulated_ln(ops, x, seqs, self.norm3.eps, m[3], m[4])
        hid = ops.linear(hb, self.mlp.mlp[0], "gelu")
        for b, sl in layout:
            ops.linear_resid(x[sl], hid[sl], self.mlp.mlp[2], m[5][b])
        return x

    @torch.no_grad()
    def forward(self, x: sp.SparseTensor, mod: torch.Tensor, context: torch.Tensor, ops=None) -> sp.SparseTensor:
        """mod: t_emb (B, C) as the reference's block takes it (the SiLU of adaLN_modulation is applied here)."""
        ops = HipOps(precision.resolve(None, (x.feats,))) if ops is None else ops
        rows = self.forward_rows(x.feats.float().contiguous().clone(), x, torch.nn.functional.silu(mod.float()).contiguous(), context, ops)
        return x.replace(rows.to(x.dtype))


class SLatFlowModel(nn.Module):
    def __init__(self, resolution: int, in_channels: int, model_channels: int, cond_channels: int, out_channels: int, num_blocks: int,
                 num_heads: Optional[int] = None, num_head_channels: Optional[int] = 64, mlp_ratio: float = 4, patch_size: int = 2,
                 num_io_res_blocks: int = 2, io_block_channels: List[int] = None, pe_mode: str = "ape", use_fp16: bool = False,
                 use_checkpoint: bool = False, use_skip_connection: bool = True, share_mod: bool = False, qk_rms_norm: bool = False,
                 qk_rms_norm_cross: bool = False):
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
        self.num_io_res_blocks = num_io_res_blocks
        self.io_block_channels = io_block_channels
        self.pe_mode = pe_mode
        self.use_fp16 = use_fp16
        self.use_checkpoint = use_checkpoint
        self.use_skip_connection = use_skip_connection
        self.share_mod = share_mod
        self.qk_rms_norm = qk_rms_norm
        self.qk_rms_norm_cross = qk_rms_norm_cross
        self.dtype = torch.float16 if use_fp16 else torch.float32
        assert int(np.log2(patch_size)) == np.log2(patch_size), "Patch size must be a power of 2"
        assert np.log2(patch_size) == len(io_block_channels), "Number of IO ResBlocks must match the number of stages"

        self.t_embedder = TimestepEmbedder(model_channels)
        self.pos_embedder = AbsolutePositionEmbedder(model_channels)
        self.input_layer = sp.SparseLinear(in_channels, io_block_channels[0])
        self.input_blocks = nn.ModuleList([])
        for chs, next_chs in zip(io_block_channels, io_block_channels[1:] + [model_channels]):
            self.input_blocks.extend([SparseResBlock3d(chs, model_channels, out_channels=chs) for _ in range(num_io_res_blocks - 1)])
            self.input_blocks.append(SparseResBlock3d(chs, model_channels, out_channels=next_chs, downsample=True))
        self.blocks = nn.ModuleList([
            ModulatedSparseTransformerCrossBlock(model_channels, cond_channels, num_heads=self.num_heads, mlp_ratio=self.mlp_ratio,
                                                 attn_mode="full", use_checkpoint=self.use_checkpoint, use_rope=False, share_mod=False,
                                                 qk_rms_norm=self.qk_rms_norm, qk_rms_norm_cross=self.qk_rms_norm_cross)
            for _ in range(num_blocks)])
        self.out_blocks = nn.ModuleList([])
        for chs, prev_chs in zip(reversed(io_block_channels), [model_channels] + list(reversed(io_block_channels[1:]))):
            self.out_blocks.append(SparseResBlock3d(prev_chs * 2 if self.use_skip_connection else prev_chs, model_channels,
                                                    out_channels=chs, upsample=True))
            self.out_blocks.extend([SparseResBlock3d(chs * 2 if self.use_skip_connection else chs, model_channels, out_channels=chs)
                                    for _ in range(num_io_res_blocks - 1)])
        self.out_layer = sp.SparseLinear(io_block_channels[0], out_channels)
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

    def _position_rows(self, st: sp.SparseTensor) -> torch.Tensor:
        """The absolute position embedding of `st`'s rows: step- and layer-invariant, kept on the spatial cache."""
        key = f"ape_{self.model_channels}"
        hit = st.get_spatial_cache(key)
        if hit is None or hit.shape[0] != st.coords.shape[0] or hit.device != st.coords.device:
            hit = self.pos_embedder(st.coords[:, 1:]).float().contiguous()
            st.register_spatial_cache(key, hit)
        return hit

    @torch.no_grad()
    def forward(self, x: sp.SparseTensor, t: torch.Tensor, cond: torch.Tensor, ops=None, taps: Optional[dict] = None) -> sp.SparseTensor:
        """x: (T, in_channels) rows; t: (B,) timesteps (the sampler's 1000 t); cond: (B, L, cond_channels) -> (T, out_channels) rows.
        ops: None = the HIP operators.  taps: a dict that receives the per-stage rows ("input", "res<i>", "conv<i>", "block<i>_self" ...)."""
        ops = HipOps(self._lp(), self._wcache) if ops is None else ops
        tap = (lambda name, v: taps.__setitem__(name, v.clone())) if taps is not None else (lambda name, v: None)
        rows = ops.linear(ops.cast(x.feats), self.input_layer, "f32")
        tap("input", rows)
        emb_silu = ops.timestep(t, self.t_embedder)
        st = x
        skips = []
        for i, block in enumerate(self.input_blocks):
            inner = [] if taps is not None else None
            st, rows = block.forward_rows(st, rows, emb_silu, ops, inner)
            skips.append(rows)
            if inner:
                tap(f"in{i}_conv1", inner[0])
            tap(f"in{i}", rows)
        rows = rows + self._position_rows(st)
        for i, block in enumerate(self.blocks):
            inner = [] if taps is not None else None
            rows = block.forward_rows(rows, st, emb_silu, cond, ops, inner)
            if inner:
                tap(f"block{i}_self", inner[0])
                tap(f"block{i}_cross", inner[1])
            tap(f"block{i}", rows)
        for i, (block, skip) in enumerate(zip(self.out_blocks, reversed(skips))):
            if self.use_skip_connection:
                rows = torch.cat([rows, skip], dim=1)
            st, rows = block.forward_rows(st, rows, emb_silu, ops)
            tap(f"out{i}", rows)
        hb = ops.ln(rows, 1e-5)                                   # F.layer_norm's default eps, no affine (:260)
        out = ops.linear(hb, self.out_layer, "f32")
        return x.replace(out.to(x.feats.dtype))
