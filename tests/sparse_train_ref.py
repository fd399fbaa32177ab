"""References for the static-VAE training operators (csrc/sparse_train.hip, gvfdiffusion_amd/ops/sparse_train.py), plain torch, any device.

gelu / posterior / reg   each operator's outputs and gradients written out BY FORMULA (no autograd) in a dtype of the caller's: torch.float64
                         is the reference every GPU bar is measured against (test_sparse_train_host.py holds the formulas to float64 autograd
                         of the forward); dtype=torch.float32 is the "yardstick", the same formulas as a naive fp32 composition with the
                         kernels' rounding points (16-bit only at the stores), the unit of the bars (tests/dit_train_ref.py).
kl_bound / reg_bounds    the derived bounds the scalars are held to (a scalar yardstick can be exact by luck).
TorchOps                 the torch namespace for the `ops=` seam of model/sparse_voxel_diffusion/sparse_train.py.
golden / golden_loss     the golden config of tests/golden/sparse_vae_golden.npz with seeded noise and weights, and the float64 reference of
                         loss = sum(out * W) / T + kl through oracle/sparse_vae_ref.py."""
import json
import math
import os

import numpy as np
import torch
import torch.nn.functional as F

from dit_train_ref import _r16, rel_l2, worst_rows  # noqa: F401  (re-exported: the two error measures)

K = math.sqrt(2.0 / math.pi)
C3 = 0.044715


def gelu(u, da, dtype=torch.float64, lp=None):
    """u, da: 16-bit values -> dict a, du (rounded to lp for the yardstick)."""
    u, da = u.to(dtype), da.to(dtype)
    inner = K * (u + C3 * u * u * u)
    t = torch.tanh(inner)
    a = 0.5 * u * (1 + t)
    sech = torch.where(inner.abs() < 10, 0.5 * u * (1 - t * t) * K * (1 + 3 * C3 * u * u), torch.zeros_like(u))   # 1 - t^2 < 2e-8 beyond
    return {"a": _r16(a, lp), "du": _r16(da * (0.5 * (1 + t) + sech), lp)}


def posterior(h, eps, dz, dkl, dtype=torch.float64):
    """h [T, 2L] = mean | logvar, eps / dz [T, L], dkl a float -> dict z, kl, dh."""
    h, eps, dz = h.to(dtype), eps.to(dtype), dz.to(dtype)
    L = eps.shape[1]
    m, lv = h[:, :L], h[:, L:]
    n = m.numel()
    z = m + torch.exp(0.5 * lv) * eps
    kl = 0.5 * (m * m + torch.exp(lv) - lv - 1).sum() / n
    dm = dz + dkl * m / n
    dl = dz * 0.5 * torch.exp(0.5 * lv) * eps + dkl * 0.5 * (torch.exp(lv) - 1) / n
    return {"z": z, "kl": kl, "dh": torch.cat([dm, dl], dim=1)}


def kl_bound(h, L):
    """|kl - kl64| <= 8 * 2^-24 * 0.5 mean(mean^2 + exp(lv) + |lv| + 1): per element half an ulp for the square, two for expf (documented to
    1 ulp; two leaves room), three additions of half an ulp each on partial sums no larger than the sum of the magnitudes -- the kernel does
    the additions and the sum over elements in double, which only removes terms -- and the final scalar's one rounding to fp32 is inside the
    same figure (it is half an ulp of kl <= the mean of magnitudes)."""
    h = h.double()
    m, lv = h[:, :L], h[:, L:]
    return 8 * 2.0 ** -24 * 0.5 * float((m * m + torch.exp(lv) + lv.abs() + 1).mean())


def _act(x, softplus):
    return F.softplus(x) if softplus else torch.exp(x)          # torch's softplus: beta 1, linear above 20


def reg(s, o, bs, bo, kappa, softplus, dvol, dopa, dtype=torch.float64):
    """s [N, 3], o [N] raw -> dict vol, opa, ds, do (formulas of include/gvf_sparse_train.h)."""
    s, o = s.to(dtype), o.to(dtype).reshape(-1)
    N = s.shape[0]
    x = s + bs
    a = _act(x, softplus)
    q = torch.sqrt(a * a + kappa * kappa)
    vol = q.prod(dim=1).sum() / N
    sg = torch.sigmoid(o + bo)
    opa = ((sg - 1) ** 2).sum() / N
    da = (torch.where(x > 20, torch.ones_like(x), torch.sigmoid(x)) if softplus else a)
    r = torch.where(q > 0, a / q, torch.zeros_like(q)) * da
    others = torch.stack([q[:, 1] * q[:, 2], q[:, 0] * q[:, 2], q[:, 0] * q[:, 1]], dim=1)
    return {"vol": vol, "opa": opa, "ds": dvol / N * others * r, "do": dopa / N * 2 * (sg - 1) * sg * (1 - sg)}


def reg_bounds(s, o, bs, bo, kappa, softplus):
    """(bound on |vol - vol64|, bound on |opa - opa64|), derived like kl_bound from the fp32 operations of one Gaussian; sums are in double.
    vol: per factor q = sqrt(a^2 + kappa^2): the bias add (half an ulp of x, which the activation turns into |x| act'(x) / act(x) <= |x|
    relative for exp and <= 1 for softplus -- taken as (|x| + 1) half-ulps), the activation (expf 1 ulp; log1pf(expf) 1 + 1 ulp: 4 half-ulps
    with room), the square, the add and the square root (half an ulp each, the root halving what comes before it: <= 2 half-ulps together);
    per Gaussian three such factors, two products and the final rounding (3 half-ulps):
        |d vol_i| <= 2^-24 vol_i (sum_k (|x_ik| + 1 + 4 + 2) + 3)
    opa: d = sg - 1 with sg = 1 / (1 + expf(-y)), y = o + bo: the add (half an ulp of y, times |d sg / d y| = sg (1 - sg) <= (1 - sg) |...|),
    expf (2 half-ulps), the add and the division (half an ulp each) all act on sg: |d sg| <= 2^-24 sg (|y| (1 - sg) + 4), the subtraction is
    exact or half an ulp of d, the square one more; (d + e)^2 - d^2 ~ 2 |d| e:
        |d opa_i| <= 2^-24 (2 |d_i| sg_i (|y_i| (1 - sg_i) + 4) + 3 d_i^2)
    Both are means of the per-Gaussian bounds plus the result's own rounding (one more half-ulp of the mean)."""
    s, o = s.double(), o.double().reshape(-1)
    x = s + bs
    a = _act(x, softplus)
    q = torch.sqrt(a * a + kappa * kappa)
    v = q.prod(dim=1)
    bv = 2.0 ** -24 * float((v * ((x.abs() + 7).sum(dim=1) + 3)).mean() + v.mean())
    y = o + bo
    sg = torch.sigmoid(y)
    d = (sg - 1).abs()
    bo_ = 2.0 ** -24 * float((2 * d * sg * (y.abs() * (1 - sg) + 4) + 3 * d * d).mean() + (d * d).mean())
    return bv, bo_


def _acc(t):
    """the type the reference computes a norm or a softmax in: fp32 (float64 in a float64 reference run)"""
    return torch.float64 if t.dtype == torch.float64 else torch.float32


class TorchOps:
    """The operators of sparse_train.py::HipOps as the torch composition the reference runs under autocast: fp32 inside the norms, `dtype`
    (16-bit on the GPU baseline, torch.float32 for the CPU check of the wiring) at the same stores.  attention: "math" (fp32 softmax
    written out per sequence, differentiated by autograd) or "sdpa" (torch's fused kernel per sequence, for timing)."""

    def __init__(self, attention="math"):
        self.attn_impl = attention

    @staticmethod
    def layernorm(x, eps, dtype):
        return F.layer_norm(x, (x.shape[-1],), None, None, eps).to(dtype), x

    @staticmethod
    def linear(x, weight, bias, dtype):
        return F.linear(x, weight.to(dtype), None if bias is None else bias.to(dtype))

    @staticmethod
    def gather_rows(x, index, inverse=None):
        return x[index]

    @staticmethod
    def rmsnorm_heads(x, gamma):
        return (F.normalize(x.to(_acc(x)), dim=-1) * gamma * (x.shape[-1] ** 0.5)).to(x.dtype)

    def attention_varlen(self, q, k, v, cu, longest):
        b = cu.tolist()
        outs = []
        for s0, s1 in zip(b[:-1], b[1:]):
            qs, ks, vs = (t[s0:s1].permute(1, 0, 2) for t in (q, k, v))            # (H, n, d)
            if self.attn_impl == "sdpa":
                o = F.scaled_dot_product_attention(qs[None], ks[None], vs[None])[0]
            else:
                acc = _acc(q)
                s = torch.matmul(qs.to(acc), ks.to(acc).transpose(-1, -2)) * (q.shape[-1] ** -0.5)
                o = torch.matmul(torch.softmax(s, dim=-1), vs.to(acc)).to(q.dtype)
            outs.append(o.permute(1, 0, 2))
        return torch.cat(outs)

    @staticmethod
    def gate_residual(x, h):
        return x + h.to(x.dtype)

    @classmethod
    def residual_linear(cls, x, h, weight, bias, dtype):
        return cls.gate_residual(x, cls.linear(h, weight, bias, dtype))

    @staticmethod
    def gelu_tanh(u):
        return F.gelu(u, approximate="tanh")

    @staticmethod
    def posterior(h, eps):
        mean, logvar = h.chunk(2, dim=-1)
        return mean + torch.exp(0.5 * logvar) * eps, 0.5 * torch.mean(mean.pow(2) + logvar.exp() - logvar - 1)


# ---- the golden config ----------------------------------------------------------------------------------------------------------------
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "sparse_vae_golden.npz")


def golden(seed=0):
    """(cfg, state dict, feats, coords, noise [T, L], W [T, out_channels]): the fixture's model and inputs, seeded noise and loss weights."""
    z = np.load(GOLD)
    cfg = json.loads(bytes(z["cfg_json"]).decode())
    sd = {k[3:]: torch.from_numpy(z[k]) for k in z.files if k.startswith("sd.")}
    feats, coords = torch.from_numpy(z["feats"]), torch.from_numpy(z["coords"])
    g = torch.Generator().manual_seed(seed)
    T = feats.shape[0]
    noise = torch.randn((T, cfg["latent_channels"]), generator=g)
    W = torch.randn((T, cfg["out_channels"]), generator=g)
    return cfg, sd, feats, coords, noise, W


def golden_loss(cfg, sd, feats, coords, noise, W, precision="fp32", dtype=torch.float64):
    """loss = sum(out * W) / T + kl through oracle/sparse_vae_ref.py on leaves of `dtype` (float64: the reference; float32 with precision
    "bf16" / "fp16": the yardstick of a 16-bit run) -> (loss, out, {name: gradient} with "feats" the input gradient)."""
    from oracle import sparse_vae_ref as ref
    leaves = {k: v.to(dtype).requires_grad_() for k, v in sd.items()}
    x = feats.to(dtype).requires_grad_()
    mean, logvar = ref.encode(leaves, cfg, x, coords, precision)
    z = mean + torch.exp(0.5 * logvar) * noise.to(dtype)
    out = ref.decode(leaves, cfg, z, coords, precision)
    kl = 0.5 * torch.mean(mean.pow(2) + logvar.exp() - logvar - 1)
    loss = (out * W.to(dtype)).sum() / feats.shape[0] + kl
    names = list(leaves)
    grads = torch.autograd.grad(loss, [leaves[k] for k in names] + [x], allow_unused=True)
    g = {k: v for k, v in zip(names + ["feats"], grads)}
    return loss.detach(), out.detach(), g


def model_loss(model, x, noise, W):
    """the same loss through the model's training forward (enable_training() on, grad enabled)"""
    out, mean, logvar, kl = model(x, noise=noise, return_kl=True)
    return (out.feats * W).sum() / W.shape[0] + kl, out
