"""The differentiable forward of the temporal-aware DiT: the computation of the reference's DiT._forward and
ModulatedSparseTransformerCrossBlock._forward (model/dit.py:449-480, 227-278) on the module's own fp32 parameters, with the placement of
torch.autocast: fp32 residual stream, 16-bit sub-layer operands, fp32 small projections.

Between two projections of a sub-layer the reference's composition is a chain of bandwidth-bound launches (layer_norm, the (1 + scale)
multiply, the shift add, the casts, the gate multiply, the residual add, F.normalize and the gain) and as many again in backward, plus the
broadcast-gradient sums over the rows of a sample.  Here each chain is one operator of ops/dit_train.py: `layernorm_modulate` writes the 16-bit
operand, `rmsnorm_heads` normalises q and k in place of the packed projection, `gate_residual` closes the sub-layer on the fp32 stream;
attention is ops/attention_grad.py.  The block projections (to_qkv, to_q, to_kv, to_out, mlp.0, mlp.2) take one of two routes, `linear=`:
"torch" (the default) is torch's library GEMM -- F.linear in the operand type on per-step casts of the fp32 master weights; the casts are
differentiable, so the gradients arrive on the parameters in fp32 after a 16-bit rounding -- and "hip" is ops/linear_grad.py: forward and input
gradient on gvf_gemm, the weight and bias gradients in fp32 from csrc/linear_grad.hip, each weight cast (and transposed) once per step.
tanh-GELU is torch's.  What oracle/dit_ref.py lists as FP32_SITES of the inference path stays fp32 torch here too: input and final layer,
timestep embedder, adaLN projections, condition projections.

`ops` is the seam through which the five operators are reached -- layernorm_modulate, gate_residual, rmsnorm_heads, attention, linear --
as attributes of one object.  None means the HIP ones (HipOps, or HipGemmOps for linear="hip"); the product never substitutes anything else.  A
test or a benchmark hands in a torch composition with the same signatures to check the wiring on the CPU or to time the baseline.  An `ops`
with a `linear_params(x, weight_fp32, bias_fp32, dtype)` attribute is handed the master parameters of a projection instead of their casts."""
import torch
import torch.nn.functional as F
import torch.utils.checkpoint

from ..ops import precision


class HipOps:
    """The five operators on the gfx950 kernels (ops/dit_train.py, ops/attention_grad.py) and torch's library GEMM."""

    @staticmethod
    def layernorm_modulate(x, ln_w=None, ln_b=None, shift=None, scale=None, rows_per_group=None, eps=1e-6, dtype=torch.bfloat16):
        """-> (y in `dtype`, the tensor to use as the residual input)"""
        from ..ops import dit_train
        return dit_train.layernorm_modulate(x, ln_w, ln_b, shift, scale, rows_per_group, eps, dtype, return_residual=True)

    @staticmethod
    def gate_residual(x, h, gate=None, rows_per_group=None):
        from ..ops import dit_train
        return dit_train.gate_residual(x, h, gate, rows_per_group)

    @staticmethod
    def rmsnorm_heads(x, gamma):
        from ..ops import dit_train
        return dit_train.rmsnorm_heads(x, gamma)

    @staticmethod
    def attention(q, k, v):
        from ..ops import attention_grad
        return attention_grad.attention(q, k, v)

    @staticmethod
    def linear(x, weight, bias=None):
        return F.linear(x, weight, bias)


class HipGemmOps(HipOps):
    """HipOps with the block projections on this library's GEMMs (ops/linear_grad.py).  One instance per forward_train call: it owns the 16-bit
    images of that call's weights, keyed by parameter, so every weight is cast once per step and a use_checkpoint recompute reads the same
    images (and gives the same bits)."""

    def __init__(self):
        self.weight_images = {}

    def linear_params(self, x, weight, bias, dtype):
        from ..ops import linear_grad
        return linear_grad.linear(x, weight, bias, dtype=dtype, cache=self.weight_images)


LINEAR_ROUTES = ("torch", "hip")


def _lin(ops, x, lin, lp):
    """A projection in the operand type: on the fp32 master parameters where `ops` takes them, else on casts of them."""
    linear_params = getattr(ops, "linear_params", None)
    if linear_params is not None:
        return linear_params(x, lin.weight, lin.bias, lp)
    return ops.linear(x, lin.weight.to(lp), None if lin.bias is None else lin.bias.to(lp))


def _self_attention(ops, m, h, lp):
    """h [S, L, C] in the operand type -> to_out(attention) [S, L, C] (model/attention/modules.py:112-146, type 'self')."""
    S, L, C = h.shape
    H, d = m.num_heads, m.head_dim
    q, k, v = _lin(ops, h, m.to_qkv, lp).reshape(S, L, 3, H, d).unbind(dim=2)
    if m.qk_rms_norm:
        q, k = ops.rmsnorm_heads(q, m.q_rms_norm.gamma), ops.rmsnorm_heads(k, m.k_rms_norm.gamma)
    return _lin(ops, ops.attention(q, k, v).reshape(S, L, C), m.to_out, lp)


def _cross_attention(ops, m, h, ctx, lp):
    """h [S, L, C], ctx [S, Lk, C] in the operand type."""
    S, L, C = h.shape
    H, d = m.num_heads, m.head_dim
    q = _lin(ops, h, m.to_q, lp).reshape(S, L, H, d)
    k, v = _lin(ops, ctx, m.to_kv, lp).reshape(S, ctx.shape[1], 2, H, d).unbind(dim=2)
    if m.qk_rms_norm:
        q, k = ops.rmsnorm_heads(q, m.q_rms_norm.gamma), ops.rmsnorm_heads(k, m.k_rms_norm.gamma)
    return _lin(ops, ops.attention(q, k, v).reshape(S, L, C), m.to_out, lp)


def _block(ops, blk, lp, x, t_emb, image_emb, static_emb):
    """One ModulatedSparseTransformerCrossBlock: x [B, T, N, C] fp32, t_emb [B, C] fp32, contexts [B * T, L, C] in the operand type."""
    B, T, N, C = x.shape
    rpg = T * N
    silu = F.silu(t_emb)
    sh_s, sc_s, g_s, sh_m, sc_m, g_m = blk.adaLN_modulation[-1](silu).chunk(6, dim=1)
    # spatial self attention over the N tokens of a frame
    h, x = ops.layernorm_modulate(x, shift=sh_s, scale=sc_s, rows_per_group=rpg, dtype=lp)
    h = _self_attention(ops, blk.spatial_self_attn, h.reshape(B * T, N, C), lp)
    x = ops.gate_residual(x, h.reshape(B, T, N, C), g_s, rpg)
    # temporal self attention over the T frames of a token
    if not blk.no_temporal_attn:
        sh_t, sc_t, g_t = blk.adaLN_modulation_temporal[-1](silu).chunk(3, dim=1)
        h, x = ops.layernorm_modulate(x, shift=sh_t, scale=sc_t, rows_per_group=rpg, dtype=lp)
        h = _self_attention(ops, blk.temporal_self_attn, h.transpose(1, 2).reshape(B * N, T, C), lp)
        x = ops.gate_residual(x, h.reshape(B, N, T, C).transpose(1, 2).contiguous(), g_t, rpg)
    # image and static cross attention: affine LayerNorm, no gate
    for norm, attn, ctx in ((blk.norm3, blk.image_cross_attn, image_emb), (blk.norm4, blk.static_cross_attn, static_emb)):
        h, x = ops.layernorm_modulate(x, ln_w=norm.weight, ln_b=norm.bias, dtype=lp)
        h = _cross_attention(ops, attn, h.reshape(B * T, N, C), ctx, lp)
        x = ops.gate_residual(x, h.reshape(B, T, N, C))
    # MLP
    h, x = ops.layernorm_modulate(x, shift=sh_m, scale=sc_m, rows_per_group=rpg, dtype=lp)
    h = F.gelu(_lin(ops, h, blk.mlp.mlp[0], lp), approximate="tanh")
    return ops.gate_residual(x, _lin(ops, h, blk.mlp.mlp[2], lp), g_m, rpg)


def forward_train(model, x, t, cond_images, static_latent, deformation_position_xyz=None, ops=None, dtype=None, linear="torch"):
    """model: a gvfdiffusion_amd.model.dit.DiT; x [B, T, N, Cin], t [B] (float or integer steps), cond_images [B, T, Li, Ci],
    static_latent [B, Ls, Cs], deformation_position_xyz [B, N, 3] -> [B, T, N, out_channels] fp32 with a graph to every parameter.
    dtype: the 16-bit operand type; None resolves it as the inference forward does (ops/precision.py).  torch.float32 is accepted only
    together with an `ops` of the caller's (the CPU check of the wiring).  linear: the route of the block projections when `ops` is None,
    "torch" (library GEMM) or "hip" (ops/linear_grad.py)."""
    if linear not in LINEAR_ROUTES:
        raise ValueError(f"forward_train: linear must be one of {LINEAR_ROUTES}, got {linear!r}")
    lp = dtype if dtype is not None else model._lp()
    if ops is None:
        ops = HipGemmOps() if linear == "hip" else HipOps
        if lp not in precision.LP_DTYPES:
            raise ValueError(f"forward_train: the HIP operators take torch.float16 or torch.bfloat16 operands, got {lp}")
    B, T, N, _ = x.shape
    C = model.model_channels
    f32 = model.input_layer.weight.dtype                     # the master type: fp32 (float64 in a test's reference run)
    h = model.input_layer(x.to(f32))
    t_emb = model.t_embedder.mlp(model.t_embedder.timestep_embedding(t, model.t_embedder.frequency_embedding_size).to(f32))
    image_emb = model.image_cond_proj(cond_images.to(f32)).to(lp).reshape(B * T, -1, C)
    static_emb = model.static_cond_proj(static_latent.to(f32)).to(lp).unsqueeze(1).expand(B, T, -1, C).reshape(B * T, -1, C)    # (dit.py:465 repeats it over T)
    if model.pe_mode == "ape":
        assert deformation_position_xyz is not None, "Deformation position xyz is required for APE mode"
        h = h + model.pos_embedder(deformation_position_xyz).to(f32).unsqueeze(1)
    elif model.pe_mode == "learnable":
        h = h + model.pos_embedder
    h = h.contiguous()
    for blk in model.blocks:
        if blk.use_checkpoint:
            h = torch.utils.checkpoint.checkpoint(_block, ops, blk, lp, h, t_emb, image_emb, static_emb, use_reentrant=False)
        else:
            h = _block(ops, blk, lp, h, t_emb, image_emb, static_emb)
    fl = model.final_layer
    shift, scale = fl.adaLN_modulation[-1](F.silu(t_emb)).chunk(2, dim=1)
    h = F.layer_norm(h, (C,), None, None, 1e-6) * (1 + scale[:, None, None]) + shift[:, None, None]
    return fl.linear(h)
