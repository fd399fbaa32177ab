"""The differentiable row path of the static VAE: the computation of the reference's SparseTransformerBlock._forward
(sparse_transformer.py:165-191, unmodulated branch) and SparseTransformerVAE.encode / decode (sparse_transformer_vae.py:158-196) on the
modules' own fp32 parameters, with the placement of torch.autocast: fp32 residual rows, 16-bit sub-layer operands.

Every step between two rows of the residual stream is one operator with a HIP forward and a HIP backward:
  layernorm_modulate, gate_residual, rmsnorm_heads   ops/dit_train.py (the DiT's)
  linear                                             ops/linear_grad.py on the fp32 masters: one cast per weight and forward through `cache`
  attention_varlen                                   ops/attention_grad.py over the window (or serialisation) order
  gather_rows, gelu_tanh, posterior, bias_grad_tap   ops/sparse_train.py
`ops` is the seam through which they are reached, as attributes of one object: None means HipOps, and the product never substitutes anything
else.  A test or a benchmark hands in a torch composition with the same signatures (tests/sparse_train_ref.py::TorchOps) to differentiate the
same wiring in fp32 on the CPU or to time the baseline.

FP32 sites: an edge layer (input_layer, to_latent, from_latent, out_layer) goes through `linear` only when both of its extents are multiples
of 32 (the contraction constraint of the forward and of the input gradient); the others -- 768 -> 16, 8 -> 768 and 768 -> 112 at the released
shapes -- are fp32 F.linear on the masters.  The position embedding is added in fp32."""
import torch
import torch.nn.functional as F
import torch.utils.checkpoint

from ...ops import precision


class HipOps:
    """The operators on the gfx950 kernels.  One instance per training forward: it owns the 16-bit images of that call's weights (`cache`), so
    every weight is cast once per step and a use_checkpoint recompute reads the same images."""

    def __init__(self, cache=None):
        self.cache = {} if cache is None else cache

    @staticmethod
    def layernorm(x, eps, dtype):
        """-> (LayerNorm(x) without affine in `dtype`, the tensor to use as the residual input)"""
        from ...ops import dit_train
        return dit_train.layernorm_modulate(x, eps=eps, dtype=dtype, return_residual=True)

    def linear(self, x, weight, bias, dtype):
        from ...ops import linear_grad
        return linear_grad.linear(x, weight, bias, dtype=dtype, cache=self.cache)

    @staticmethod
    def gather_rows(x, index, inverse=None):
        from ...ops import sparse_train
        return sparse_train.gather_rows(x, index, inverse)

    @staticmethod
    def rmsnorm_heads(x, gamma):
        from ...ops import dit_train
        return dit_train.rmsnorm_heads(x, gamma)

    @staticmethod
    def attention_varlen(q, k, v, cu, longest):
        from ...ops import attention_grad
        return attention_grad.attention_varlen(q, k, v, cu, cu, longest, longest)

    @staticmethod
    def gate_residual(x, h):
        from ...ops import dit_train
        return dit_train.gate_residual(x, h)

    def residual_linear(self, x, h, weight, bias, dtype):
        """x + (h W^T + bias): the projection that closes a sub-layer.  The bias is added in the GEMM epilogue, and its gradient is taken from
        the fp32 stream gradient (sparse_train.bias_grad_tap), not from the 16-bit rounding of it that the weight gradient contracts."""
        from ...ops import dit_train, sparse_train
        out = dit_train.gate_residual(x, self.linear(h, weight, None if bias is None else bias.detach(), dtype))
        return out if bias is None else sparse_train.bias_grad_tap(out, bias)

    @staticmethod
    def gelu_tanh(u):
        from ...ops import sparse_train
        return sparse_train.gelu_tanh(u)

    @staticmethod
    def posterior(h, eps):
        from ...ops import sparse_train
        return sparse_train.posterior(h, eps)


def resolve_ops(ops, lp, cache=None):
    if ops is None:
        if lp not in precision.LP_DTYPES:
            raise ValueError(f"the HIP training operators take torch.float16 or torch.bfloat16 operands, got {lp}")
        return HipOps(cache)
    return ops


def block_rows(blk, x, st, lp, ops):
    """One unmodulated SparseTransformerBlock on fp32 rows x (T, C) of `st` -> new fp32 rows (nothing is updated in place)."""
    from .sparse_transformer import token_partition
    a = blk.attn
    T, C = x.shape
    H = a.num_heads
    d = C // H
    fwd, bwd, cu, longest = token_partition(st, a.attn_mode, a.window_size, a.shift_sequence, a.shift_window, a.serialize_mode)
    h, x = ops.layernorm(x, blk.norm1.eps, lp)
    qkv = ops.linear(h, a.to_qkv.weight, a.to_qkv.bias, lp)                      # (T, 3C), the module's own channel order
    if fwd is not None:
        # window order: a permutation when every token sits in exactly one sequence (always for windows; for a serialisation only when no
        # sample is split into several windows, whose index repeats rows)
        perm = fwd.numel() == T
        qkv = ops.gather_rows(qkv, fwd, bwd if perm else None)                    # the packed rows in ONE launch
    M = qkv.shape[0]
    if a.use_old_attn_impl:                                                       # channels [head][q|k|v][c] (sparse/attention/modules.py:150-158)
        q, k, v = qkv.view(M, H, 3, d).unbind(dim=2)
    else:                                                                         # channels [q|k|v][head][c]
        q, k, v = qkv.view(M, 3, H, d).unbind(dim=1)
    if a.qk_rms_norm:
        q, k = ops.rmsnorm_heads(q, a.q_rms_norm.gamma), ops.rmsnorm_heads(k, a.k_rms_norm.gamma)
    ao = ops.attention_varlen(q, k, v, cu, longest).reshape(M, C)
    if bwd is not None:
        ao = ops.gather_rows(ao, bwd, fwd if fwd.numel() == T else None)
    x = ops.residual_linear(x, ao, a.to_out.weight, a.to_out.bias, lp)
    h, x = ops.layernorm(x, blk.norm2.eps, lp)
    fc1, fc2 = blk.mlp.mlp[0], blk.mlp.mlp[2]
    u = ops.linear(h, fc1.weight, fc1.bias, lp)                                   # u = h W1^T + b1 rounded to 16 bits: autocast's placement
    return ops.residual_linear(x, ops.gelu_tanh(u), fc2.weight, fc2.bias, lp)


def block_rows_train(blk, x, st, lp, ops):
    if blk.use_checkpoint and torch.is_grad_enabled():
        return torch.utils.checkpoint.checkpoint(block_rows, blk, x, st, lp, ops, use_reentrant=False)
    return block_rows(blk, x, st, lp, ops)


def edge_linear(ops, x, lin, lp):
    """An edge layer on fp32 or 16-bit rows -> fp32 rows: `linear` when both extents are multiples of 32, else fp32 on the masters."""
    if lin.in_features % 32 == 0 and lin.out_features % 32 == 0:
        return ops.linear(x.to(lp), lin.weight, lin.bias, lp).to(lin.weight.dtype)
    return F.linear(x.to(lin.weight.dtype), lin.weight, lin.bias)


def torso(model, st, rows, lin_in, blocks, lin_out, lp, ops):
    """rows (T, K) of `st` -> edge layer (+ position embedding) -> blocks -> [LayerNorm] -> edge layer: (T, N_out) in the masters' type."""
    C = model.model_channels
    x = edge_linear(ops, rows, lin_in, lp)
    if model.pe_mode == "ape":
        x = x + model.pos_embedder(st.coords[:, 1:]).to(x.dtype)
    x = x.contiguous()
    for blk in blocks:
        x = block_rows_train(blk, x, st, lp, ops)
    if model.norm_output:                                                          # F.layer_norm default eps (:166,194)
        h, _ = ops.layernorm(x, 1e-5, lp)
    else:
        h = x.to(lp)
    return edge_linear(ops, h, lin_out, lp)
