"""References for the motion-VAE training operators (csrc/vae_train.hip, gvfdiffusion_amd/ops/vae_train.py), plain torch, any device.

geglu / embed / posterior_groups   each operator's outputs and gradients written out BY FORMULA (no autograd) in a dtype of the caller's:
                                   torch.float64 is the reference every GPU bar is measured against (test_vae_train_host.py holds the formulas
                                   to float64 autograd of the plain torch expression); dtype=torch.float32 is the "yardstick", the same formulas
                                   as a naive fp32 torch composition with the kernels' rounding points (16-bit only at GEGLU's stores), the unit
                                   of the bars (tests/dit_train_ref.py, tests/sparse_train_ref.py).
kl_groups_bound / dkl_bound        the derived bounds the per-group KL terms are held to (a scalar yardstick can be exact by luck)."""
import math

import torch

from dit_train_ref import _r16, rel_l2, worst_rows  # noqa: F401  (re-exported: the two error measures)

EMBED_EPS = 1e-5
LV_MIN, LV_MAX = -30.0, 20.0
GEGLU_CUT = 14.0


# ---- GEGLU --------------------------------------------------------------------------------------------------------------------------------
def geglu(u, da, dtype=torch.float64, lp=None):
    """u [rows, 2F] = x | g and da [rows, F] (16-bit values) -> dict a [rows, F], du [rows, 2F] (rounded to lp for the yardstick)."""
    u, da = u.to(dtype), da.to(dtype)
    F_ = u.shape[1] // 2
    x, g = u[:, :F_], u[:, F_:]
    cdf = 0.5 * (1 + torch.erf(g / math.sqrt(2.0)))
    gel = g * cdf
    gp = torch.where(g.abs() < GEGLU_CUT, g * torch.exp(-0.5 * g * g) / math.sqrt(2 * math.pi), torch.zeros_like(g))   # < 2e-42 beyond
    return {"a": _r16(x * gel, lp), "du": _r16(torch.cat([da * gel, da * (x * (cdf + gp))], dim=1), lp)}


# ---- embedding ----------------------------------------------------------------------------------------------------------------------------
def point_embed(xyz, omega):
    """[P, 3] -> ([P, C] values, [P, C] derivative of each value in its own coordinate): per axis sin(p omega_j), j < E, then cos(p omega_j)"""
    ph = xyz[:, :, None] * omega[None, None, :]                              # [P, 3, E]
    s, c = torch.sin(ph), torch.cos(ph)
    v = torch.cat([s, c], dim=-1).reshape(xyz.shape[0], -1)
    d = torch.cat([c * omega, -s * omega], dim=-1).reshape(xyz.shape[0], -1)
    return v, d


def _ln(t, eps):
    mean = t.mean(dim=1, keepdim=True)
    tc = t - mean
    rstd = 1.0 / torch.sqrt((tc * tc).mean(dim=1, keepdim=True) + eps)
    return tc * rstd, rstd


def _ln_bwd(d, th, rstd):
    return rstd * (d - d.mean(dim=1, keepdim=True) - th * (d * th).mean(dim=1, keepdim=True))


def embed(r, W, b, omega, de, dtype=torch.float64, eps=EMBED_EPS):
    """r [P, qdim], W [C, qdim], b [C], omega [C / 6], de [P, C] -> dict e, dW, db, dr (formulas of include/gvf_vae_train.h)."""
    r, W, b, omega, de = (t.to(dtype) for t in (r, W, b, omega, de))
    C = W.shape[0]
    uh, ru = _ln(r @ W.t() + b, eps)
    v, dvdp = point_embed(r[:, :3], omega)
    vh, rv = _ln(v, eps)
    du, dv = _ln_bwd(de, uh, ru), _ln_bwd(de, vh, rv)
    dr = du @ W
    dr[:, :3] += (dv * dvdp).reshape(-1, 3, C // 3).sum(dim=-1)
    return {"e": uh + vh, "dW": du.t() @ r, "db": du.sum(dim=0), "dr": dr}


# ---- grouped posterior --------------------------------------------------------------------------------------------------------------------
def posterior_groups(mean, logvar, eps, dz, dkl, G, dtype=torch.float64):
    """mean, logvar, eps [G * L, Dl], dz the same shape or None, dkl [G] or None -> dict z, kl [G], dmean, dlogvar."""
    mean, logvar, eps = mean.to(dtype), logvar.to(dtype), eps.to(dtype)
    rows, Dl = mean.shape
    L = rows // G
    n = L * Dl
    lv = logvar.clamp(LV_MIN, LV_MAX)
    inside = ((logvar >= LV_MIN) & (logvar <= LV_MAX)).to(dtype)
    z = mean + torch.exp(0.5 * lv) * eps
    kl = 0.5 * (mean * mean + torch.exp(lv) - 1 - lv).reshape(G, n).sum(dim=1) / n
    gk = torch.zeros(G, dtype=dtype) if dkl is None else dkl.to(dtype)
    gk = gk.reshape(G, 1, 1).expand(G, L, Dl).reshape(rows, Dl)
    dm = gk * mean / n
    dl = 0.5 * gk * (torch.exp(lv) - 1) / n
    if dz is not None:
        dz = dz.to(dtype)
        dm = dm + dz
        dl = dl + dz * 0.5 * torch.exp(0.5 * lv) * eps
    return {"z": z, "kl": kl, "dmean": dm, "dlogvar": dl * inside}


def kl_groups_bound(mean, logvar, G):
    """[G] bounds on |kl[g] - kl64[g]|, sparse_train_ref.kl_bound per group with the clamp in front: 8 * 2^-24 * 0.5 mean(mean^2 + exp(lv) +
    |lv| + 1) -- per element half an ulp for the square, two for expf (documented to 1 ulp; two leaves room), three additions of half an ulp
    each on partial sums no larger than the sum of the magnitudes (the kernel does them and the sum over elements in double, which only
    removes terms), and the result's one rounding to fp32 (half an ulp of kl <= the mean of magnitudes).  The clamp is exact."""
    mean, lv = mean.double(), logvar.double().clamp(LV_MIN, LV_MAX)
    n = mean.numel() // G
    return 8 * 2.0 ** -24 * 0.5 * (mean * mean + torch.exp(lv) + lv.abs() + 1).reshape(G, n).mean(dim=1)


def dkl_bound(mean, logvar, dkl, G):
    """element-wise bounds on the KL part of (dmean, dlogvar) against float64, from the kernel's operations:
    dmean = (dkl m) / n: a product and a quotient, half an ulp each: 2^-24 |dmean| * 2 (taken as 3 for the conversion of n).
    dlogvar = ((0.5 dkl) (expf(lv) - 1)) / n: expf 1 ulp (two half-ulps, doubled for room: 4) of exp(lv), the subtraction half an ulp of its
    result, then product and quotient: 2^-24 |0.5 dkl| / n * (4 exp(lv) + 3 |exp(lv) - 1|)."""
    mean, lv, dkl = mean.double(), logvar.double().clamp(LV_MIN, LV_MAX), dkl.double()
    rows, Dl = mean.shape
    L = rows // G
    n = L * Dl
    gk = dkl.reshape(G, 1, 1).expand(G, L, Dl).reshape(rows, Dl).abs()
    u = 2.0 ** -24
    return 3 * u * gk * mean.abs() / n, u * 0.5 * gk / n * (4 * torch.exp(lv) + 3 * (torch.exp(lv) - 1).abs())


# ---- the network ------------------------------------------------------------------------------------------------------------------------
import torch.nn.functional as F  # noqa: E402


def _acc(t):
    """the type the reference computes a norm or a softmax in: fp32 (float64 in a float64 reference run)"""
    return torch.float64 if t.dtype == torch.float64 else torch.float32


class TorchOps:
    """The operators of model/autoencoder_train.py::HipOps as the torch composition the reference runs under autocast: fp32 inside the norms
    and the softmax, `dtype` (16-bit on the GPU baseline, torch.float32 for the CPU check of the wiring) at the same stores.  attention:
    "math" (softmax written out, differentiated by autograd) or "sdpa" (torch's fused kernel, for timing)."""

    def __init__(self, attention="math"):
        self.attn_impl = attention

    @staticmethod
    def layernorm(x, eps, dtype):
        return F.layer_norm(x, (x.shape[-1],), None, None, eps).to(dtype), x

    @staticmethod
    def linear(x, weight, bias, dtype):
        return F.linear(x, weight.to(dtype), None if bias is None else bias.to(dtype))

    def attention(self, q, k, v):
        """q [N, Lq, H, d], k / v [N, Lk, H, d] -> [N, Lq, H, d]"""
        qs, ks, vs = (t.permute(0, 2, 1, 3) for t in (q, k, v))
        if self.attn_impl == "sdpa":
            return F.scaled_dot_product_attention(qs, ks, vs).permute(0, 2, 1, 3)
        acc = _acc(q)
        s = torch.matmul(qs.to(acc), ks.to(acc).transpose(-1, -2)) * (q.shape[-1] ** -0.5)
        return torch.matmul(torch.softmax(s, dim=-1), vs.to(acc)).to(q.dtype).permute(0, 2, 1, 3)

    @classmethod
    def residual_linear(cls, x, h, weight, bias, dtype):
        return x + cls.linear(h, weight, bias, dtype).to(x.dtype)

    @staticmethod
    def geglu(u):
        x, g = u.chunk(2, dim=-1)
        return x * F.gelu(g)

    @staticmethod
    def embed(r, weight, bias, omega):
        C = weight.shape[0]
        ph = r[:, :3, None] * omega                                          # [P, 3, E]: per axis sin, then cos (PointEmbed)
        pe = torch.cat([torch.sin(ph), torch.cos(ph)], dim=-1).reshape(r.shape[0], C)
        return F.layer_norm(F.linear(r, weight, bias), (C,), None, None, EMBED_EPS) + F.layer_norm(pe, (C,), None, None, EMBED_EPS)

    @staticmethod
    def posterior_groups(mean, logvar, eps, groups):
        lv = torch.clamp(logvar, LV_MIN, LV_MAX)
        kl = 0.5 * (mean.pow(2) + lv.exp() - 1.0 - lv).reshape(groups, -1).mean(dim=1)
        return mean + torch.exp(0.5 * lv) * eps, kl


CFG = dict(depth=2, dim=192, queries_dim=192, output_dim=14, num_inputs=64, num_latents=40, latent_dim=16, heads=3, dim_head=-1,
           num_timesteps=3, chunk_size=8192)
B, P = 2, 70


def model(cfg=CFG, seed=0, **kw):
    """the module with every parameter randomised as tests/test_vae_gpu.py::_model does (so that to_outputs is not zero)"""
    from gvfdiffusion_amd.model.autoencoder import GSKLTemporalVariationalAutoEncoder
    torch.manual_seed(seed)
    m = GSKLTemporalVariationalAutoEncoder(**dict(cfg, **kw))
    with torch.no_grad():
        for _, p in m.named_parameters():
            if p.dim() == 2:
                p.copy_(torch.randn_like(p) * (1.0 / math.sqrt(p.shape[1])))
            else:
                p.copy_(torch.randn_like(p) * 0.1)
    return m


def inputs(cfg=CFG, seed=1, counts=(P, P)):
    """dict of the fixed inputs of both cases: x latents, queries (B, P, 14) padded beyond counts[b] as pad_static_gs pads, static_pc,
    delta_pc, input_static_gs (the first L Gaussians' xyz stand in for the FPS sample), noise, W (the loss weights) with zeros on the padding"""
    g = torch.Generator().manual_seed(seed)
    T, L, N, Dl = cfg["num_timesteps"], cfg["num_latents"], cfg["num_inputs"], cfg["latent_dim"]
    nb, pm = len(counts), max(counts)
    x = torch.randn((nb * T, L, Dl), generator=g)
    q = torch.randn((nb, pm, 14), generator=g)
    q[..., :3] = torch.rand((nb, pm, 3), generator=g) - 0.5
    W = torch.randn((nb, T, pm, cfg["output_dim"]), generator=g)
    for b, n in enumerate(counts):
        q[b, n:] = 0.0
        q[b, n:, 10] = 1.0
        W[b, :, n:] = 0.0
    static_pc = torch.rand((nb, N, 3), generator=g) - 0.5
    delta_pc = torch.randn((nb, T, N, 3), generator=g) * 0.05
    noise = torch.randn((nb * T * L, Dl), generator=g)
    return dict(x=x, queries=q, W=W, static_pc=static_pc, delta_pc=delta_pc, input_static_gs=q[:, :L, :3].clone(), noise=noise)


def oracle_grads(sd, cfg, inp, case, precision="fp32", dtype=torch.float64, knn_k=8, beta=7.0):
    """loss = sum(logits * W) / n (+ kl.mean() for case "encode_decode") through oracle/vae_ref.py on leaves of `dtype` (float64: the
    reference; float32 with precision "bf16" / "fp16": the yardstick of a 16-bit run) -> dict loss, logits, est, grads {name: gradient of
    every parameter the case uses, "queries", and "x" for case "decode"}."""
    from oracle import vae_ref
    T = cfg["num_timesteps"]
    leaves = {k: (v.to(dtype).requires_grad_() if "omega" not in k else v.to(dtype)) for k, v in sd.items()}
    q = inp["queries"].to(dtype).requires_grad_()
    W = inp["W"].to(dtype)
    extra, est = {"queries": q}, None
    if case == "decode":
        x = inp["x"].to(dtype).requires_grad_()
        extra["x"] = x
        logits = vae_ref.vae_decode(leaves, cfg, x, q, T, precision)
        loss = (logits * W).sum() / W.numel()
    else:
        mean, logvar, est = vae_ref.vae_encode(leaves, cfg, inp["static_pc"].to(dtype), inp["delta_pc"].to(dtype), inp["input_static_gs"].to(dtype),
                                               knn_k, beta, precision)
        BT, L, Dl = mean.shape
        lv = torch.clamp(logvar, LV_MIN, LV_MAX)
        z = mean + torch.exp(0.5 * lv) * inp["noise"].to(dtype).view(BT, L, Dl)
        kl = 0.5 * torch.mean(mean.pow(2) + lv.exp() - 1.0 - lv, dim=[1, 2])
        logits = vae_ref.vae_decode(leaves, cfg, z, q, T, precision)
        loss = (logits * W).sum() / W.numel() + kl.mean()
    names = [k for k in leaves if leaves[k].requires_grad] + list(extra)
    grads = torch.autograd.grad(loss, [leaves[k] if k in leaves else extra[k] for k in names], allow_unused=True)
    return dict(loss=loss.detach(), logits=logits.detach(), est=None if est is None else est.detach(),
                grads={k: g for k, g in zip(names, grads) if g is not None})


def model_grads(m, inp, case, est=None, scale=1.0, dev="cpu"):
    """the same loss through the module's training route (enable_training() on, grad enabled) -> dict loss, logits, grads"""
    q = inp["queries"].to(dev).requires_grad_()
    W = inp["W"].to(dev)
    extra = {"queries": q}
    if case == "decode":
        x = inp["x"].to(dev).requires_grad_()
        extra["x"] = x
        logits = m.decode(x, q)
        loss = (logits * W).sum() / W.numel()
    else:
        kl, z, _ = m.encode_rows(inp["static_pc"].to(dev), inp["delta_pc"].to(dev), inp["input_static_gs"].to(dev), est.float().to(dev),
                                 noise=inp["noise"].to(dev))
        logits = m.decode(z, q)
        loss = (logits * W).sum() / W.numel() + kl.mean()
    names, params = zip(*m.named_parameters())
    names = list(names) + list(extra)
    grads = torch.autograd.grad(loss * scale, list(params) + list(extra.values()), allow_unused=True)
    return dict(loss=loss.detach(), logits=logits.detach(), grads={k: g / scale for k, g in zip(names, grads) if g is not None})
