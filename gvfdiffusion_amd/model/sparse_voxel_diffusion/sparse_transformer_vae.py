"""SparseTransformerVAE -- the static-VAE backbone (model/sparse_voxel_diffusion/sparse_transformer_vae.py:14-213) on
the MI355X kernels: same constructor keywords, same parameter tree (`input_layer`, `encoder.N.*`, `to_latent`,
`from_latent`, `decoder.N.*`, `out_layer`), `encode(x, sample_posterior, return_raw)`, `decode(latent)` and
`forward(x) -> (out, mean, logvar)`.

Precision placement (the reference casts the torso to fp16 with `use_fp16`, :164,192): the residual stream stays fp32
from the input layer to the output layer; every GEMM / attention operand is 16 bit with fp32 accumulation -- fp16 when the module was
built with `use_fp16=True` / after `convert_to_fp16()` (the reference's own arithmetic type), bf16 otherwise; `set_compute_dtype`,
`GVF_DIT_DTYPE` or an autocast region override it (ops/precision.py).  The elastic
memory controller (gradient checkpointing by memory ratio) is a training device and is accepted but ignored."""
from contextlib import contextmanager
from typing import *

import torch
import torch.nn as nn

from ... import sparse as sp
from ..._lib import require_cuda
from ...ops import dit_ops, precision
from .sparse_transformer import AbsolutePositionEmbedder, build_blocks, edge_weights, run_torso

__all__ = ["SparseTransformerVAE"]


class SparseTransformerVAE(nn.Module):
    def __init__(self, resolution, in_channels, model_channels, out_channels, latent_channels, num_blocks, window_size=1024,
                 num_heads=None, num_head_channels=64, mlp_ratio=4, attn_mode="swin", pe_mode="ape", use_fp16=False,
                 use_checkpoint=False, use_old_attn_impl=True, norm_output=False):
        super().__init__()
        self.resolution = resolution
        self.in_channels = in_channels
        self.model_channels = model_channels
        self.out_channels = out_channels
        self.latent_channels = latent_channels
        self.num_blocks = num_blocks
        self.window_size = window_size
        self.num_heads = num_heads or model_channels // num_head_channels
        self.mlp_ratio = mlp_ratio
        self.attn_mode = attn_mode
        self.pe_mode = pe_mode
        self.use_fp16 = use_fp16
        self.use_checkpoint = use_checkpoint
        self.norm_output = norm_output
        self.dtype = torch.float16 if use_fp16 else torch.float32
        if pe_mode == "ape":
            self.pos_embedder = AbsolutePositionEmbedder(model_channels)
        elif pe_mode == "rope":
            raise NotImplementedError("RoPE is not built (the released static VAE uses pe_mode='ape')")

        def blocks():
            return build_blocks(self, model_channels, self.num_heads, self.mlp_ratio, use_checkpoint, use_old_attn_impl=use_old_attn_impl)

        self.input_layer = sp.SparseLinear(in_channels, model_channels)
        self.encoder = blocks()
        self.to_latent = sp.SparseLinear(model_channels, 2 * latent_channels)
        self.from_latent = sp.SparseLinear(latent_channels, model_channels)
        self.decoder = blocks()
        self.out_layer = sp.SparseLinear(model_channels, out_channels)
        self.initialize_weights()
        self._wcache = None
        self.compute_dtype = None          # None: ops/precision.py's rule with the module default below
        self._train_path, self._train_dtype, self._train_ops = False, None, None      # enable_training()

    @property
    def device(self):
        return next(self.parameters()).device

    def set_compute_dtype(self, dtype):
        """torch.float16 / torch.bfloat16 (or "fp16" / "bf16"); None hands the choice back to ops/precision.py."""
        self.compute_dtype = precision.parse(dtype)
        return self

    def _lp(self):
        return precision.resolve(self.compute_dtype, (), torch.float16 if self.use_fp16 else torch.bfloat16)

    def convert_to_fp16(self):   # the parameters stay fp32 (they are cast once per version); the kernels contract fp16
        self.use_fp16, self.dtype = True, torch.float16

    def convert_to_fp32(self):   # (no fp32 matrix path: 16-bit operands with fp32 accumulation, bf16 by default)
        self.use_fp16, self.dtype = False, torch.float32

    def initialize_weights(self):
        for m in self.modules():
            if isinstance(m, nn.Linear):
                torch.nn.init.xavier_uniform_(m.weight)
                if m.bias is not None:
                    nn.init.constant_(m.bias, 0)
        for lin in (self.to_latent, self.out_layer):
            nn.init.constant_(lin.weight, 0)
            nn.init.constant_(lin.bias, 0)

    def freeze_encoder(self):
        for block in self.encoder:
            block.requires_grad_(False)

    # ---- weights of the four edge layers (bf16, K padded to 64) ----------------------------------------------------------
    def _weights(self):
        lp = self._lp()
        edge = (self.input_layer, self.to_latent, self.from_latent, self.out_layer)
        ver = (tuple((p.data_ptr(), p._version) for lin in edge for p in lin.parameters()), lp)
        if self._wcache is not None and self._wcache[0] == ver:
            return self._wcache[1]
        W = {name: edge_weights(lin, lp) for name, lin in zip(("input", "to_latent", "from_latent", "out"), edge)}
        self._wcache = (ver, W)
        return W

    def _torso(self, st: sp.SparseTensor, rows: torch.Tensor, w_in, blocks, w_out) -> torch.Tensor:
        """rows fp32 (T, K) -> edge GEMM (+ APE) -> blocks -> [LayerNorm] -> edge GEMM: fp32 (T, N_out)."""
        T, C = rows.shape[0], self.model_channels
        if T == 0:                                                                 # an empty voxel list maps to an empty one
            return torch.zeros((0, w_out[0].shape[0]), dtype=torch.float32, device=rows.device)
        lp = w_in[0].dtype
        x = run_torso(st, rows, w_in, self.pos_embedder if self.pe_mode == "ape" else None, blocks, C, lp)
        if self.norm_output:                                                       # F.layer_norm default eps (:166,194)
            hb = torch.empty((T, C), dtype=lp, device=rows.device)
            dit_ops.layernorm_modulate(x, hb, 1e-5)
        else:
            hb = dit_ops.cast_pad(x, C, dtype=lp)
        out = torch.empty((T, w_out[0].shape[0]), dtype=torch.float32, device=rows.device)
        return dit_ops.gemm(hb, *w_out, out, dit_ops.EPI_STORE_F32)

    # ---- training: the differentiable row path (sparse_train.py) ------------------------------------------------------------
    def enable_training(self, on: bool = True, dtype=None, ops=None):
        """An explicit switch, like DiT.enable_training(): with it on AND grad enabled, encode / decode / forward run the differentiable row
        path of sparse_train.py -- fp32 `feats` with a graph to every parameter and to the input features.  Off (the default), or under
        torch.no_grad(), every call is the inference path, bit for bit.  Not keyed on self.training or on requires_grad.
        dtype: the 16-bit operand type of the training path (None: what _lp() resolves).  ops: None = the HIP operators; a torch namespace
        with the same signatures (a test's CPU check, a benchmark's baseline), which may then also name torch.float32 as dtype."""
        self._train_path = bool(on)
        self._train_dtype = precision.parse(dtype) if (dtype is not None and ops is None) else dtype
        self._train_ops = ops
        return self

    def training_enabled(self) -> bool:
        return bool(getattr(self, "_train_path", False))

    def _train_now(self) -> bool:
        return self.training_enabled() and torch.is_grad_enabled()

    def _train_setup(self, ops=None):
        from . import sparse_train
        lp = self._train_dtype if self._train_dtype is not None else self._lp()
        if ops is None:
            ops = sparse_train.resolve_ops(self._train_ops, lp)
        return sparse_train, lp, ops

    def _encode_train(self, x, sample_posterior, return_raw, noise, ops=None, return_kl=False):
        T, lp, ops = self._train_setup(ops)
        if self._train_ops is None:
            require_cuda(x.feats, x.coords)
        f32 = self.input_layer.weight.dtype
        h = T.torso(self, x, x.feats.to(f32), self.input_layer, self.encoder, self.to_latent, lp, ops)
        mean, logvar = h.chunk(2, dim=-1)
        kl = None
        if sample_posterior:
            eps = torch.randn_like(mean) if noise is None else noise.to(h.dtype)
            z, kl = ops.posterior(h, eps)
        else:
            z = mean
        out = (x.replace(z), mean, logvar) if return_raw else (x.replace(z),)
        if return_kl:
            out = out + (kl,)
        return out if len(out) > 1 else out[0]

    def _decode_train(self, latent, ops=None):
        T, lp, ops = self._train_setup(ops)
        if self._train_ops is None:
            require_cuda(latent.feats, latent.coords)
        f32 = self.from_latent.weight.dtype
        return latent.replace(T.torso(self, latent, latent.feats.to(f32), self.from_latent, self.decoder, self.out_layer, lp, ops))

    def encode(self, x: sp.SparseTensor, sample_posterior=True, return_raw=False, noise=None):
        """noise: the posterior's standard-normal draw, fp32 (T, latent_channels) (None: torch.randn_like) -- the training path only."""
        if self._train_now() and x.feats.shape[0] > 0:
            return self._encode_train(x, sample_posterior, return_raw, noise)
        return self._encode_infer(x, sample_posterior, return_raw)

    def decode(self, latent: sp.SparseTensor) -> sp.SparseTensor:
        if self._train_now() and latent.feats.shape[0] > 0:
            return self._decode_train(latent)
        return self._decode_infer(latent)

    @torch.no_grad()
    def _encode_infer(self, x: sp.SparseTensor, sample_posterior=True, return_raw=False):
        require_cuda(x.feats, x.coords)
        W = self._weights()
        h = self._torso(x, x.feats, W["input"], self.encoder, W["to_latent"])
        mean, logvar = h.chunk(2, dim=-1)
        z = mean + torch.exp(0.5 * logvar) * torch.randn_like(mean) if sample_posterior else mean
        z = x.replace(z.to(x.dtype))
        if return_raw:
            return z, mean.to(x.dtype), logvar.to(x.dtype)
        return z

    @torch.no_grad()
    def _decode_infer(self, latent: sp.SparseTensor) -> sp.SparseTensor:
        require_cuda(latent.feats, latent.coords)
        W = self._weights()
        return latent.replace(self._torso(latent, latent.feats, W["from_latent"], self.decoder, W["out"]).to(latent.dtype))

    def forward(self, x: sp.SparseTensor, t=None, c=None, mem_ratio=1.0, noise=None, return_kl=False):
        """-> (out, mean, logvar): ElasticModule.forward around _forward_with_mem_ratio (:206-210).  mem_ratio is accepted and ignored.
        On the training path (enable_training() and grad enabled) out.feats, mean and logvar are fp32 and carry the graph; noise is the
        posterior's draw (None: randn_like) and return_kl=True appends the KL term the posterior operator computed with the sample."""
        if self._train_now() and x.feats.shape[0] > 0:
            _, _, ops = self._train_setup()
            latent, mean, logvar, kl = self._encode_train(x, True, True, noise, ops=ops, return_kl=True)
            out = self._decode_train(latent, ops=ops)
            return (out, mean, logvar, kl) if return_kl else (out, mean, logvar)
        if return_kl:
            raise RuntimeError("SparseTransformerVAE.forward(return_kl=True) belongs to the training path: call enable_training() and run with "
                               "grad enabled")
        latent, mean, logvar = self.encode(x, sample_posterior=True, return_raw=True)
        return self.decode(latent), mean, logvar

    def _get_input_size(self, x: sp.SparseTensor, t=None, c=None):
        return x.feats.shape[0]

    @contextmanager
    def with_mem_raio(self, mem_ratio=1.0):
        yield 1.0
