"""What the structured-latent flow tests share: the small golden config and the released one, the weights (a NumPy Generator by
parameter name -- never stored), the inputs, the closed-form stand-in model of the sampler goldens, and TorchOps: the operators of
gvfdiffusion_amd/trellis/models/structured_latent_flow.py::HipOps as torch compositions of the same signatures, for the CPU.

TorchOps(lp): `lp` is the type at the operand stores.  torch.float32 / torch.float64: the wiring check against the reference-pinned golden
(nothing is rounded) and the float64 reference of the GPU tests.  torch.float16 / torch.bfloat16: every matrix operand is rounded to lp
where the HIP route rounds it, products are accumulated in fp32 -- the deviation of that run from float64 is the yardstick of the GPU
route (a 16-bit route may deviate twice as far)."""
import math
import os
import zlib

import numpy as np
import torch
import torch.nn.functional as F

import spconv_ref as S

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "slat_flow_golden.npz")
MANIFEST = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "slat_flow_manifest.json")

SMALL = dict(resolution=16, in_channels=8, model_channels=128, cond_channels=64, out_channels=8, num_blocks=2, num_heads=2, mlp_ratio=4,
             patch_size=2, num_io_res_blocks=2, io_block_channels=[64], pe_mode="ape", use_fp16=False, use_skip_connection=True,
             share_mod=False, qk_rms_norm=True, qk_rms_norm_cross=False)
RELEASED = dict(resolution=64, in_channels=8, model_channels=1024, cond_channels=1024, out_channels=8, num_blocks=24, num_heads=16,
                mlp_ratio=4, patch_size=2, num_io_res_blocks=2, io_block_channels=[128], pe_mode="ape", use_fp16=True,
                use_skip_connection=True, share_mod=False, qk_rms_norm=True, qk_rms_norm_cross=False)
COND_TOKENS = 24


def build(cfg, device=None):
    from gvfdiffusion_amd.trellis.models import SLatFlowModel
    if device is None:
        return SLatFlowModel(**cfg).eval()
    with torch.device(device):
        return SLatFlowModel(**cfg).eval()


def make_weights(cfg, seed):
    """name -> fp32 array for every parameter of SLatFlowModel(**cfg): a Generator per name (seed, crc32(name)), so the values do not
    depend on the order of the state dict.  Every tensor the model zero-initialises (conv2, adaLN_modulation, out_layer) is non-zero."""
    shapes = {k: tuple(v.shape) for k, v in build(cfg, "meta").state_dict().items()}
    out = {}
    for name, shape in shapes.items():
        g = np.random.default_rng([seed, zlib.crc32(name.encode())])
        leaf = name.rsplit(".", 1)[-1]
        if leaf == "gamma" or (leaf == "weight" and len(shape) == 1):
            w = 1.0 + 0.1 * g.standard_normal(shape)
        elif leaf == "bias":
            w = 0.1 * g.standard_normal(shape)
        elif len(shape) == 5:                                   # conv weight [out, 3, 3, 3, in]: ~ 13.5 neighbours per row
            w = g.standard_normal(shape) / math.sqrt(13.5 * shape[4])
        elif "adaLN_modulation" in name or "emb_layers" in name:
            w = 0.5 * g.standard_normal(shape) / math.sqrt(shape[1])
        else:
            w = g.standard_normal(shape) / math.sqrt(shape[1])
        out[name] = w.astype(np.float32)
    return out


def load_weights(model, weights):
    sd = {k: torch.from_numpy(v) for k, v in weights.items()}
    model.load_state_dict(sd, strict=True)
    return model


def golden_coords(samples=(0, 1)):
    """Two ragged samples on 16^3: shell(16, 2.5, 4.0) and shell(16, 1.5, 3.5), grid order; `samples` picks and renumbers them."""
    parts = [S.shell(16, 2.5, 4.0, 0), S.shell(16, 1.5, 3.5, 0)]
    out = []
    for n, k in enumerate(samples):
        c = parts[k].clone()
        c[:, 0] = n
        out.append(c)
    return torch.cat(out).contiguous()


def golden_inputs(seed=5, samples=(0, 1)):
    """(coords int32 (T,4), feats fp32 (T,8), t fp32 (B,), cond fp32 (B, COND_TOKENS, 64)) of the golden; a sub-batch keeps its samples' values."""
    g = torch.Generator().manual_seed(seed)
    full = golden_coords()
    feats = torch.randn((full.shape[0], SMALL["in_channels"]), generator=g)
    cond = torch.randn((2, COND_TOKENS, SMALL["cond_channels"]), generator=g)
    t = torch.tensor([700.0, 130.0])
    rows = torch.cat([torch.nonzero(full[:, 0] == k)[:, 0] for k in samples])
    return golden_coords(samples), feats[rows].contiguous(), t[list(samples)].contiguous(), cond[list(samples)].contiguous()


# ---- the closed-form stand-in of the sampler goldens ---------------------------------------------------------------------------------------

def standin_model(x, t, cond):
    """v(x, t, cond) = (0.3 + t / 2000) x - 0.7 cond + 0.1 sin(t / 100): dense (B, C) state, t = 1000 x the sampler's time."""
    a = (0.3 + t / 2000.0)[:, None]
    return a * x - 0.7 * cond + 0.1 * torch.sin(t / 100.0)[:, None]


SAMPLER_CASES = {
    "euler": dict(cls="FlowEulerSampler", kw=dict(steps=5, rescale_t=1.0)),
    "euler_rescaled": dict(cls="FlowEulerSampler", kw=dict(steps=4, rescale_t=3.0)),
    "cfg": dict(cls="FlowEulerCfgSampler", kw=dict(steps=5, rescale_t=1.0, cfg_strength=3.0), neg=True),
    "interval": dict(cls="FlowEulerGuidanceIntervalSampler", kw=dict(steps=6, rescale_t=3.0, cfg_strength=2.5, cfg_interval=(0.5, 0.95)), neg=True),
}


def sampler_inputs():
    g = torch.Generator().manual_seed(9)
    return (torch.randn((2, 5), generator=g, dtype=torch.float64), torch.randn((2, 5), generator=g, dtype=torch.float64),
            torch.randn((2, 5), generator=g, dtype=torch.float64))


# ---- TorchOps ------------------------------------------------------------------------------------------------------------------------------

class TorchOps:
    def __init__(self, lp=torch.float32):
        self.lp = lp
        self.acc = torch.float64 if lp is torch.float64 else torch.float32

    def _a(self, t):
        return None if t is None else t.detach().to(self.acc)

    def _op(self, t):
        """A matrix operand: rounded to lp, widened to the accumulation type."""
        return t.detach().to(self.lp).to(self.acc)

    @staticmethod
    def neighbor_map(coords):
        return S.neighbor_map(coords.cpu()).to(coords.device)

    def t_emb(self, t, embedder):
        """TimestepEmbedder(t) itself: what the reference's blocks take (their SiLU -> Linear heads come after)."""
        half = embedder.frequency_embedding_size // 2
        freqs = torch.exp(-math.log(10000.0) * torch.arange(half, dtype=self.acc, device=t.device) / half)
        args = t.to(self.acc)[:, None] * freqs[None]
        emb = torch.cat([torch.cos(args), torch.sin(args)], dim=-1)
        m0, m2 = embedder.mlp[0], embedder.mlp[2]
        h = F.silu(F.linear(emb, self._a(m0.weight), self._a(m0.bias)))
        return F.linear(h, self._a(m2.weight), self._a(m2.bias))

    def timestep(self, t, embedder):
        return F.silu(self.t_emb(t, embedder))

    def modulation(self, s, lin):
        return F.linear(s.to(self.acc), self._a(lin.weight), self._a(lin.bias))

    def cast(self, x):
        return x.to(self.lp)

    def ln(self, x, eps, ln_w=None, ln_b=None, shift=None, scale=None, act=0, out=None):
        y = F.layer_norm(x.to(self.acc), (x.shape[-1],), self._a(ln_w), self._a(ln_b), eps)
        if scale is not None:
            y = y * (1 + scale.to(self.acc)) + shift.to(self.acc)
        if act == 1:
            y = F.silu(y)
        y = y.to(self.lp)
        if out is not None:
            out.copy_(y)
            return out
        return y

    def linear(self, a16, lin, kind="f32"):
        y = F.linear(a16.to(self.acc), self._op(lin.weight), self._a(lin.bias))
        if kind == "f32":
            return y
        return (F.gelu(y, approximate="tanh") if kind == "gelu" else y).to(self.lp)

    def linear_resid(self, x, a16, lin, gate=None):
        y = F.linear(a16.to(self.acc), self._op(lin.weight), self._a(lin.bias))
        x += y if gate is None else gate.to(self.acc)[None, :] * y
        return x

    def conv3(self, a16, nbr, conv, addend=None):
        c = conv.conv
        T = a16.shape[0]
        a = a16.to(self.acc)
        idx = nbr.long().clamp_min(0)
        g = a[idx.reshape(-1)].reshape(T, 27, c.in_channels) * (nbr >= 0).to(self.acc)[:, :, None]
        y = g.reshape(T, -1) @ self._op(c.weight).reshape(c.out_channels, -1).T
        if c.bias is not None:
            y = y + self._a(c.bias)
        return y if addend is None else y + addend.to(self.acc)

    def attention(self, q, k, v, cu_q, cu_k, max_q, max_k, heads, gq=None, gk=None):
        Tq, C = q.shape
        d = C // heads
        split = lambda t: t.to(self.acc).reshape(t.shape[0], heads, d)
        qh, kh, vh = split(q), split(k), split(v)
        if gq is not None:                                  # the kernel normalises in fp32 and feeds the matrix pipe 16-bit q, k
            qh = self._op(F.normalize(qh, dim=-1) * self._a(gq) * d ** 0.5)
            kh = self._op(F.normalize(kh, dim=-1) * self._a(gk) * d ** 0.5)
        out = torch.empty((Tq, heads, d), dtype=self.acc, device=q.device)
        bq, bk = cu_q.tolist(), cu_k.tolist()
        for i in range(len(bq) - 1):
            qs, ks, vs = qh[bq[i]:bq[i + 1]], kh[bk[i]:bk[i + 1]], vh[bk[i]:bk[i + 1]]
            s = torch.einsum("nhd,mhd->hnm", qs, ks) * d ** -0.5
            p = self._op(torch.softmax(s, dim=-1))           # ... and 16-bit probabilities for P V
            out[bq[i]:bq[i + 1]] = torch.einsum("hnm,mhd->nhd", p, vs)
        return out.reshape(Tq, C).to(self.lp)


def run(model, coords, feats, t, cond, ops, taps=None):
    """model(x, t, cond) through `ops` on whatever device the tensors are on -> output rows."""
    from gvfdiffusion_amd import sparse as sp
    x = sp.SparseTensor(feats, coords)
    return model(x, t, cond, ops=ops, taps=taps).feats
