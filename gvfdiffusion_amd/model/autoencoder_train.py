"""The differentiable route of the motion VAE: the computation of the reference's GSKLTemporalVariationalAutoEncoder.encode / decode /
forward (model/autoencoder.py:502-627) on the module's own fp32 parameters, with the placement of torch.autocast -- fp32 residual rows and
LayerNorms, 16-bit operands of the projections and of attention -- written against oracle/vae_ref.py line for line.

Every step between two rows of the residual stream is one operator with a HIP forward and a HIP backward:
  layernorm_modulate, gate_residual      ops/dit_train.py (the DiT's; the PreNorm LayerNorms have no affine pair)
  linear                                 ops/linear_grad.py on the fp32 masters: one cast per weight and step through `cache`
  attention                              ops/attention_grad.py, q / k / v read in place as strided slices of the packed projections
  bias_grad_tap                          ops/sparse_train.py: the bias gradient of a projection that closes a sub-layer
  geglu, embed, posterior_groups         ops/vae_train.py
`ops` is the seam through which they are reached, as attributes of one object: None means HipOps, and the product never substitutes anything
else.  A test or a benchmark hands in a torch composition with the same signatures (tests/vae_train_ref.py::TorchOps) to differentiate the
same wiring in fp32 on the CPU or to time the baseline.

FP32 sites: proj (latent_dim -> dim, K = 16 at the released config), to_outputs (dim -> 14) and mean_fc / logvar_fc (dim -> 16) miss the
multiple-of-32 rule of `linear` and are fp32 F.linear on the masters; the embeddings and the posterior are fp32 at every interface.
The query embedding and to_q run once per static Gaussian; attention reads them for every frame through a stride-0 expand, whose backward
(torch's) adds the T per-frame gradients in fp32-accumulating order and rounds once.  There is no training-time fold of to_out into to_outputs.
Not differentiated, as in the reference: the farthest point sampling and the KNN interpolation (model/autoencoder.py:465)."""
import torch
import torch.nn.functional as F
import torch.utils.checkpoint

from ..ops import precision

PRENORM_EPS = 1e-6


class HipOps:
    """The operators on the gfx950 kernels.  One instance per training forward: it owns the 16-bit images of that call's weights (`cache`), so
    every weight is cast once per step and a use_checkpoint recompute reads the same images."""

    def __init__(self, cache=None):
        self.cache = {} if cache is None else cache

    @staticmethod
    def layernorm(x, eps, dtype):
        """-> (LayerNorm(x) without affine in `dtype`, the tensor to use as the residual input)"""
        from ..ops import dit_train
        return dit_train.layernorm_modulate(x, eps=eps, dtype=dtype, return_residual=True)

    def linear(self, x, weight, bias, dtype):
        from ..ops import linear_grad
        return linear_grad.linear(x, weight, bias, dtype=dtype, cache=self.cache)

    @staticmethod
    def attention(q, k, v):
        from ..ops import attention_grad
        return attention_grad.attention(q, k, v)

    def residual_linear(self, x, h, weight, bias, dtype):
        """x + (h W^T + bias): the projection that closes a sub-layer.  The bias is added in the GEMM epilogue, and its gradient is taken from
        the fp32 stream gradient (sparse_train.bias_grad_tap), not from the 16-bit rounding of it that the weight gradient contracts."""
        from ..ops import dit_train, sparse_train
        out = dit_train.gate_residual(x, self.linear(h, weight, None if bias is None else bias.detach(), dtype))
        return out if bias is None else sparse_train.bias_grad_tap(out, bias)

    @staticmethod
    def geglu(u):
        from ..ops import vae_train
        return vae_train.geglu(u)

    @staticmethod
    def embed(r, weight, bias, omega):
        from ..ops import vae_train
        return vae_train.embed(r, weight, bias, omega)

    @staticmethod
    def posterior_groups(mean, logvar, eps, groups):
        from ..ops import vae_train
        return vae_train.posterior_groups(mean, logvar, eps, groups)


class TrainState:
    """What enable_training() leaves on the module: the operand type, the operator namespace (None: HipOps) and the checkpoint switch."""

    def __init__(self, dtype=None, ops=None, use_checkpoint=True):
        self.dtype, self.ops, self.use_checkpoint = precision.parse(dtype), ops, bool(use_checkpoint)


def _begin(m):
    """(operand type, operators) of one training call: a fresh HipOps, hence a fresh weight cache, per call"""
    st = m._train
    if st.ops is not None:
        return (st.dtype if st.dtype is not None else torch.float32), st.ops
    lp = precision.resolve(st.dtype if st.dtype is not None else m.compute_dtype, (), torch.bfloat16)
    if lp not in precision.LP_DTYPES:
        raise ValueError(f"the HIP training operators take torch.float16 or torch.bfloat16 operands, got {lp}")
    return lp, HipOps()


def _omega(m):
    return m.position_encoding[0].omega.detach().float().contiguous()


def _feed_forward(ops, x, ff, lp):
    """x fp32 rows -> x + net.2(GEGLU(net.0(LN(x))))"""
    h, x = ops.layernorm(x, PRENORM_EPS, lp)
    u = ops.linear(h, ff.net[0].weight, ff.net[0].bias, lp)              # u = [x | gates] rounded to 16 bits: autocast's placement
    return ops.residual_linear(x, ops.geglu(u), ff.net[2].weight, ff.net[2].bias, lp)


def _self_block(ops, x, attn, ff, wqkv, BT, L, H, d, lp):
    """one latent block (model/autoencoder.py:596-598): x + attn(LN(x)), then x + ff(LN(x))"""
    C = H * d
    h, x = ops.layernorm(x, PRENORM_EPS, lp)
    q, k, v = ops.linear(h, wqkv, None, lp).view(BT, L, 3, H, d).unbind(dim=2)        # strided slices of the packed rows, read in place
    ao = ops.attention(q, k, v).reshape(BT * L, C)
    x = ops.residual_linear(x, ao, attn.to_out.weight, attn.to_out.bias, lp)
    return _feed_forward(ops, x, ff, lp)


def _decode_latents(m, x, lp, ops):
    BT, L, Dl = x.shape
    h = F.linear(x.reshape(BT * L, Dl).to(m.proj.weight.dtype), m.proj.weight, m.proj.bias)      # K = latent_dim: an FP32 site
    for a, f in m.layers:
        wqkv = torch.cat([a.fn.to_q.weight, a.fn.to_kv.weight], dim=0)   # one master, one cast; autograd splits its gradient
        h = _self_block(ops, h, a.fn, f.fn, wqkv, BT, L, m.heads, m.dim_head, lp)
    return h


def decode_latents(m, x):
    lp, ops = _begin(m)
    return _decode_latents(m, x, lp, ops)


def _decode_chunk(m, ops, lp, rows, k, v):
    """rows (B, n, gs_dim) static Gaussians, k / v (B, T, L, H, d) -> (B, T, n, output_dim)   (process_chunk, model/autoencoder.py:552-577)"""
    B, n = rows.shape[:2]
    T, H, d = k.shape[1], m.heads, m.dim_head
    C = H * d
    dec = m.decoder_cross_attn.fn
    gs = m.gs_embedding[0]
    e = ops.embed(rows.reshape(B * n, -1).to(gs.weight.dtype), gs.weight, gs.bias, _omega(m).to(gs.weight.dtype))
    qn, _ = ops.layernorm(e, PRENORM_EPS, lp)
    q = ops.linear(qn, dec.to_q.weight, None, lp).view(B, n, H, d)        # once per static Gaussian, shared by the T frames
    ao = torch.stack([ops.attention(q[b][None].expand(T, n, H, d), k[b], v[b]) for b in range(B)])
    lat = ops.linear(ao.reshape(B * T * n, C), dec.to_out.weight, dec.to_out.bias, lp)
    y = F.linear(lat.to(m.to_outputs.weight.dtype), m.to_outputs.weight, m.to_outputs.bias)      # N = output_dim: an FP32 site
    return y.view(B, T, n, -1)


def _decode(m, x, queries, lp, ops):
    B, P = queries.shape[:2]
    T, H, d = m.num_timesteps, m.heads, m.dim_head
    BT, L = x.shape[:2]
    if BT != B * T:
        raise ValueError(f"x has {BT} latent sets, queries imply B*T = {B}*{T}")
    h = _decode_latents(m, x, lp, ops)
    hn, _ = ops.layernorm(h, PRENORM_EPS, lp)
    k, v = ops.linear(hn, m.decoder_cross_attn.fn.to_kv.weight, None, lp).view(B, T, L, 2, H, d).unbind(dim=3)
    outs = []
    step = max(1, int(m.chunk_size))
    for p0 in range(0, P, step):
        rows = queries[:, p0:p0 + step]
        if m._train.use_checkpoint and torch.is_grad_enabled():
            outs.append(torch.utils.checkpoint.checkpoint(_decode_chunk, m, ops, lp, rows, k, v, use_reentrant=False))
        else:
            outs.append(_decode_chunk(m, ops, lp, rows, k, v))
    return outs[0] if len(outs) == 1 else torch.cat(outs, dim=2)


def decode(m, x, queries):
    """x (B*T, L, latent_dim), queries (B, P, gs_dim) -> (B, T, P, output_dim), differentiable in x, queries and every decoder parameter"""
    lp, ops = _begin(m)
    return _decode(m, x, queries, lp, ops)


def _encode_rows(m, static_pc, delta_pc, input_static_gs, est, noise, lp, ops):
    from .autoencoder import DiagonalGaussianDistribution
    B, N, _ = static_pc.shape
    T, L = delta_pc.shape[1], input_static_gs.shape[1]
    H, d = m.heads, m.dim_head
    C, M = H * d, B * T * L
    lin = m.input_embedding[0]
    wt = lin.weight.dtype
    static_pc, delta_pc, input_static_gs, est = (t.to(wt) for t in (static_pc, delta_pc, input_static_gs, est))
    # rows [xyz | delta]; the Linear sees only the delta (zero weight columns on xyz, built here so that autograd drops their gradient),
    # PointEmbed only the xyz
    qrows = torch.cat([input_static_gs[:, None].expand(B, T, L, 3), est], dim=-1).reshape(M, 6)
    crows = torch.cat([static_pc[:, None].expand(B, T, N, 3), delta_pc], dim=-1).reshape(B * T * N, 6)
    w6 = torch.cat([torch.zeros_like(lin.weight), lin.weight], dim=1)
    omega = _omega(m).to(wt)
    xq = ops.embed(qrows, w6, lin.bias, omega)
    ctx = ops.embed(crows, w6, lin.bias, omega)
    a, ff = m.cross_attend_blocks[0].fn, m.cross_attend_blocks[1].fn
    hq, xq = ops.layernorm(xq, PRENORM_EPS, lp)
    hc, _ = ops.layernorm(ctx, PRENORM_EPS, lp)                            # (the context rows are needed in their normalised form only)
    q = ops.linear(hq, a.to_q.weight, None, lp).view(B * T, L, H, d)
    k, v = ops.linear(hc, a.to_kv.weight, None, lp).view(B * T, N, 2, H, d).unbind(dim=2)
    x = ops.residual_linear(xq, ops.attention(q, k, v).reshape(M, C), a.to_out.weight, a.to_out.bias, lp)
    x = _feed_forward(ops, x, ff, lp)
    mean = F.linear(x, m.mean_fc.weight, m.mean_fc.bias)                 # N = latent_dim: FP32 sites
    logvar = F.linear(x, m.logvar_fc.weight, m.logvar_fc.bias)
    Dl = mean.shape[1]
    if noise is None:
        noise = torch.randn((M, Dl), dtype=mean.dtype, device=mean.device)
    z, kl = ops.posterior_groups(mean, logvar, noise.reshape(M, Dl).to(mean.dtype), B * T)
    posterior = DiagonalGaussianDistribution(mean.view(B * T, L, Dl), logvar.view(B * T, L, Dl))
    return kl, z.view(B * T, L, Dl), posterior


def encode_rows(m, static_pc, delta_pc, input_static_gs, est, noise=None):
    """The differentiable part of encode: static_pc (B,N,3), delta_pc (B,T,N,3), input_static_gs (B,L,3) the sampled Gaussians' xyz, est
    (B,T,L,3) their KNN-interpolated motion, noise (B*T*L, latent_dim) or None (drawn) -> (kl [B*T], z (B*T, L, latent_dim), posterior)."""
    lp, ops = _begin(m)
    return _encode_rows(m, static_pc, delta_pc, input_static_gs, est, noise, lp, ops)


def _sample(m, static_pc, delta_pc, static_gs_list, random_start):
    """farthest point sampling and KNN interpolation, under no_grad as in the reference; the sampled xyz keep their graph (a gather)"""
    from ..utils.points import sample_gs
    sampled = sample_gs(static_gs_list, m.num_latents, random_start=random_start)                    # (B, L, gs_dim)
    input_static_gs = sampled[..., :3].float()
    with torch.no_grad():
        s, dlt = static_pc.detach().float(), delta_pc.detach().float()
        est = m.compute_delta_interp(input_static_gs.detach().contiguous(), s, dlt + s[:, None], knn_k=m.knn_k, beta=m.beta)
    return sampled, input_static_gs, est


def encode(m, static_pc, delta_pc, static_gs_list, random_start=True, noise=None):
    lp, ops = _begin(m)
    sampled, input_static_gs, est = _sample(m, static_pc, delta_pc, static_gs_list, random_start)
    kl, z, posterior = _encode_rows(m, static_pc, delta_pc, input_static_gs, est, noise, lp, ops)
    return kl, z, posterior, sampled


def forward(m, static_gs, static_pc, delta_pc, noise=None, random_start=True):
    """encode -> decode over the padded static Gaussians with ONE operator namespace (one weight cache) for the whole step"""
    lp, ops = _begin(m)
    sampled, input_static_gs, est = _sample(m, static_pc, delta_pc, static_gs, random_start)
    kl, z, posterior = _encode_rows(m, static_pc, delta_pc, input_static_gs, est, noise, lp, ops)
    padded, _ = m.pad_static_gs(static_gs)
    return {"logits": _decode(m, z, padded, lp, ops).squeeze(-1), "kl": kl, "posterior": posterior}
