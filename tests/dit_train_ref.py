"""References for the DiT training operators (csrc/dit_train.hip, gvfdiffusion_amd/ops/dit_train.py), plain torch, any device.

ln_mod / gate / rms      each operator's outputs and gradients written out BY FORMULA (no autograd) in a dtype of the caller's:
                         torch.float64 is the reference every GPU bar is measured against (test_dit_train_host.py holds the formulas to
                         float64 autograd of the forward).  The inputs are the values the kernel reads: fp32 tensors, and 16-bit
                         tensors already rounded.
dtype=torch.float32      the "yardstick": the same formulas as an fp32 composition with the kernels' rounding points (16-bit only at the
                         stores the kernels round at), every reduction a plain running sum in index order (torch.cumsum) -- the naive fp32
                         evaluation.  Its distance from the float64 result is the unit of the GPU bars (twice it: room for another
                         summation order, not for another algorithm), as in tests/attn_bwd_ref.py.
rel_l2 / worst_rows      the two error measures (whole tensor; worst block of 32 rows).
TorchOps                 the five-operator torch namespace for the `ops=` seam of model/dit_train.py::forward_train."""
import torch
import torch.nn.functional as F


def _sum(t, dim):
    """Sum along dim: exact-order-free in float64, a running sum in index order in fp32 (the yardstick)."""
    if t.dtype == torch.float64:
        return t.sum(dim=dim)
    if t.shape[dim] == 0:
        return t.sum(dim=dim)
    return torch.cumsum(t, dim=dim).select(dim, t.shape[dim] - 1)


def _group_rows(rows, rpg, device):
    return torch.arange(rows, device=device) // int(rpg)


def _group_sum(t, rows_per_group):
    """[rows, C] -> [G, C] sums over the rows of each group, rows in order."""
    rows = t.shape[0]
    G = (rows + rows_per_group - 1) // rows_per_group
    return torch.stack([_sum(t[g * rows_per_group:min(rows, (g + 1) * rows_per_group)], 0) for g in range(G)])


def _r16(t, lp):
    """the kernel's one rounding to the 16-bit type (a float64 reference keeps the unrounded value)"""
    return t if (lp is None or t.dtype == torch.float64) else t.to(lp).to(t.dtype)


def ln_mod(x, dy, dres=None, w=None, b=None, shift=None, scale=None, rpg=None, eps=1e-6, dtype=torch.float64, lp=None):
    """x [rows, C] fp32, dy [rows, C] (16-bit values), dres optional fp32, w / b [C], shift / scale [G, C] -> dict y, dx, dshift, dscale, dw, db."""
    dt = dtype
    rows, C = x.shape
    x, dy = x.to(dt), dy.to(dt)
    mean = _sum(x, 1)[:, None] / C
    xc = x - mean
    var = _sum(xc * xc, 1)[:, None] / C
    rstd = 1.0 / torch.sqrt(var + eps)
    xh = xc * rstd
    a = xh * w.to(dt) + b.to(dt) if w is not None else xh
    if scale is not None:
        gi = _group_rows(rows, rpg, x.device)
        m = 1.0 + scale.to(dt)[gi]
        y = a * m + shift.to(dt)[gi]
    else:
        m = torch.ones_like(x)
        y = a
    g = dy * m
    gm = g
    if w is not None:
        g = g * w.to(dt)
    c1 = _sum(g, 1)[:, None] / C
    c2 = _sum(g * xh, 1)[:, None] / C
    dx = rstd * (g - c1 - xh * c2)
    if dres is not None:
        dx = dres.to(dt) + dx
    out = {"y": _r16(y, lp), "dx": dx, "rstd": rstd}
    if scale is not None:
        out["dshift"], out["dscale"] = _group_sum(dy, rpg), _group_sum(dy * a, rpg)
    if w is not None:
        out["dw"], out["db"] = _sum(gm * xh, 0), _sum(gm, 0)
    return out


def gate(x, h, dout, gate=None, rpg=None, dtype=torch.float64, lp=None):
    """x, dout [rows, C] fp32, h [rows, C] (16-bit values), gate [G, C] -> dict out, dh, dgate."""
    dt = dtype
    rows = x.shape[0]
    x, h, dout = x.to(dt), h.to(dt), dout.to(dt)
    if gate is None:
        return {"out": x + h, "dh": _r16(dout, lp)}
    gt = gate.to(dt)[_group_rows(rows, rpg, x.device)]
    return {"out": x + gt * h, "dh": _r16(gt * dout, lp), "dgate": _group_sum(dout * h, rpg)}


def rms(x, dy, gamma, dtype=torch.float64, lp=None):
    """x, dy [rows, H, d] (16-bit values), gamma [H, d] fp32 -> dict y, dx, dgamma."""
    dt = dtype
    d = x.shape[-1]
    x, dy, gm = x.to(dt), dy.to(dt), gamma.to(dt)
    den = torch.sqrt(_sum(x * x, 2))[..., None].clamp_min(1e-12)
    xt = x / den
    sq = float(d) ** 0.5
    y = xt * gm * sq
    u = dy * gm * sq
    dx = (u - xt * _sum(u * xt, 2)[..., None]) / den
    return {"y": _r16(y, lp), "dx": _r16(dx, lp), "dgamma": sq * _sum(dy * xt, 0)}


def rel_l2(x, ref):
    """||x - ref|| / ||ref|| over the whole tensor (0 / 0 = 0)."""
    x, ref = x.double(), ref.double()
    den = ref.norm().item()
    num = (x - ref).norm().item()
    return 0.0 if num == 0.0 else (num / den if den > 0 else float("inf"))


def worst_rows(x, ref, block=32):
    """max over the blocks of 32 rows of a [rows, ...] tensor of that block's relative L2; blocks whose reference is all zero are skipped
    (they are held element-wise by the caller)."""
    x, ref = x.double().reshape(x.shape[0], -1), ref.double().reshape(ref.shape[0], -1)
    worst = 0.0
    for r0 in range(0, x.shape[0], block):
        den = ref[r0:r0 + block].norm().item()
        if den > 0:
            worst = max(worst, (x[r0:r0 + block] - ref[r0:r0 + block]).norm().item() / den)
    return worst


class _AttentionAtKernelPoints(torch.autograd.Function):
    """softmax(q k^T / sqrt(d)) v as an fp32 composition with the rounding points of the HIP attention, forward and backward
    (tests/attn_bwd_ref.py::yardstick: P rounded to the operand type where it feeds dV, dS where it feeds dQ and dK, delta from the rounded
    O, gradients rounded once)."""

    @staticmethod
    def forward(ctx, q, k, v):
        import attn_bwd_ref
        ctx.save_for_backward(q, k, v)
        return attn_bwd_ref.yardstick(q, k, v, torch.zeros_like(q), q.shape[-1] ** -0.5, q.dtype)[0]

    @staticmethod
    def backward(ctx, do):
        import attn_bwd_ref
        q, k, v = ctx.saved_tensors
        return attn_bwd_ref.yardstick(q, k, v, do.contiguous(), q.shape[-1] ** -0.5, q.dtype)[1:]


class TorchOps:
    """The five operators of model/dit_train.py as the torch composition the reference runs under autocast: fp32 inside the norms, 16-bit
    (or whatever `dtype` is: torch.float32 for the CPU check of the wiring) at the same stores.  `attention`: "math" (fp32 softmax written
    out, differentiated by autograd), "kernel_points" (the same with the HIP attention's rounding points in its backward: the yardstick
    of a 16-bit run) or "sdpa" (torch's fused scaled_dot_product_attention, for timing)."""

    def __init__(self, attention="math"):
        self.attn_impl = attention

    @staticmethod
    def layernorm_modulate(x, ln_w=None, ln_b=None, shift=None, scale=None, rows_per_group=None, eps=1e-6, dtype=torch.float32):
        C = x.shape[-1]
        h = F.layer_norm(x, (C,), ln_w, ln_b, eps)
        if scale is not None:
            rows, rpg = x.numel() // C, int(rows_per_group)
            if rows % rpg == 0:                              # whole groups: the reference's broadcast form (unsqueeze)
                h = (h.reshape(-1, rpg, C) * (1 + scale[:, None]) + shift[:, None]).reshape(x.shape)
            else:
                gi = torch.arange(rows, device=x.device) // rpg
                h = (h.reshape(rows, C) * (1 + scale[gi]) + shift[gi]).reshape(x.shape)
        return h.to(dtype), x

    @staticmethod
    def gate_residual(x, h, gate=None, rows_per_group=None):
        if gate is None:
            return x + h.float()
        C = x.shape[-1]
        rows, rpg = x.numel() // C, int(rows_per_group)
        if rows % rpg == 0:
            return x + (h.float().reshape(-1, rpg, C) * gate[:, None]).reshape(x.shape)
        gi = torch.arange(rows, device=x.device) // rpg
        return x + (h.float().reshape(rows, C) * gate[gi]).reshape(x.shape)

    @staticmethod
    def rmsnorm_heads(x, gamma):
        return (F.normalize(x.float(), dim=-1) * gamma * (x.shape[-1] ** 0.5)).to(x.dtype)

    def attention(self, q, k, v):
        if self.attn_impl == "kernel_points":
            return _AttentionAtKernelPoints.apply(q, k, v)
        q, k, v = (t.permute(0, 2, 1, 3) for t in (q, k, v))
        if self.attn_impl == "sdpa":
            o = F.scaled_dot_product_attention(q, k, v)
        else:
            s = torch.matmul(q.float(), k.float().transpose(-1, -2)) * (q.shape[-1] ** -0.5)
            o = torch.matmul(torch.softmax(s, dim=-1), v.float()).to(q.dtype)
        return o.permute(0, 2, 1, 3)

    @staticmethod
    def linear(x, weight, bias=None):
        return F.linear(x, weight, bias)


def load_small(device="cpu"):
    """(model, diffusion, fixture dict) of tests/golden/dit_small_train_golden.npz: this package's DiT with the fixture's weights."""
    import json
    import os
    import numpy as np
    from gvfdiffusion_amd.model.dit import DiT
    from gvfdiffusion_amd.model.gaussian_diffusion import create_gaussian_diffusion
    here = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
    g = np.load(os.path.join(here, "dit_small_golden.npz"))
    fx = dict(np.load(os.path.join(here, "dit_small_train_golden.npz")))
    fx.update(np.load(os.path.join(here, "dit_small_train_golden_b.npz")))
    cfg = json.loads(bytes(g["cfg_json"]).decode())
    model = DiT(**cfg)
    model.load_state_dict({k[3:]: torch.from_numpy(g[k]) for k in g.files if k.startswith("sd.")})
    model = model.to(device)
    diffusion = create_gaussian_diffusion(**json.loads(bytes(fx["diffusion_json"]).decode()))
    fx["x_start"] = g["x"]
    fx["cond"] = {"cond_images": torch.from_numpy(g["cond_images"]).to(device), "static_latent": torch.from_numpy(g["static_latent"]).to(device),
                  "deformation_position_xyz": torch.from_numpy(g["xyz"]).to(device)}
    return model, diffusion, fx
