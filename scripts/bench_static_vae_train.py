"""The static-VAE training operators (ops/sparse_train.py on csrc/sparse_train.hip) against their torch compositions.  GPU only.

  1. each new operator forward + backward against the torch composition a user would write, at the released sizes (20 000 voxels, 768
     channels, mlp 3072, latent 8, 8 Gaussians a voxel), fp16 and bf16 where the operator has a 16-bit type:
       gelu_tanh      F.gelu(u, approximate="tanh") on [T, 3072]
       gather_rows    three x[idx] gathers of the q / k / v slices with their autograd (index_put_ with accumulate) against ONE gather of the
                      packed [T, 3C] rows whose gradient is the same kernel on the inverse permutation
       posterior      z = mean + exp(0.5 logvar) eps and kl = 0.5 mean(mean^2 + exp(logvar) - logvar - 1)
       gaussian_reg   prod(get_scaling).mean() and (get_opacity - 1)^2.mean() on 160 000 Gaussians
  2. the backbone forward + backward at the released config (12 + 12 blocks, 768 channels, 12 heads, swin window 8 on a 64^3 grid, 20 000
     voxels in one sample): the HIP operators; the same wiring with the four new operators as torch compositions (isolates them); and
     tests/sparse_train_ref.py::TorchOps for every element-wise operator and projection, around the HIP attention (thousands of windows: a
     per-window torch attention would time python).
The sides alternate in one process, GVF_ROUNDS times, device events around GVF_STEPS calls; min .. max over the rounds.
GVF_BENCH_SECTIONS (default "ops,full") selects the sections; GVF_BENCH_BLOCKS (default 12) the blocks per stack."""
import os
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from gvfdiffusion_amd import sparse as sp  # noqa: E402
from gvfdiffusion_amd.model.sparse_voxel_diffusion import SparseTransformerVAE, sparse_train  # noqa: E402
from gvfdiffusion_amd.ops import sparse_train as S  # noqa: E402
import sparse_train_ref as R  # noqa: E402

dev = torch.device("cuda:0")
N_STEPS = int(os.environ.get("GVF_STEPS", 20))
ROUNDS = int(os.environ.get("GVF_ROUNDS", 3))
SECTIONS = set(os.environ.get("GVF_BENCH_SECTIONS", "ops,full").split(","))
BLOCKS = int(os.environ.get("GVF_BENCH_BLOCKS", 12))
T, C, HID, L, NG = 20000, 768, 3072, 8, 8


def timed(fn, n):
    fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n


def alternate(sides, n=N_STEPS):
    out = {k: [] for k in sides}
    for _ in range(ROUNDS):
        for k, fn in sides.items():
            out[k].append(timed(fn, n))
    return out


def span(v):
    return f"{min(v):.3f} .. {max(v):.3f}"


def report(title, res, base="torch"):
    print(title)
    for k, v in res.items():
        ratio = "" if k == base else f"   torch / this = {min(res[base]) / min(v):.2f} x"
        print(f"    {k:<22s} {span(v)} ms{ratio}")


def ops_section():
    g = torch.Generator(device=dev).manual_seed(0)
    rnd = lambda *s: torch.randn(s, generator=g, device=dev)   # noqa: E731
    for dt in (torch.float16, torch.bfloat16):
        u = (rnd(T, HID) * 2).to(dt).requires_grad_()
        da = rnd(T, HID).to(dt)

        def gelu(fn):
            def f():
                u.grad = None
                fn(u).backward(da)
            return f
        report(f"gelu_tanh [{T}, {HID}] {dt}: forward + backward", alternate({"torch": gelu(lambda t: F.gelu(t, approximate="tanh")), "hip": gelu(S.gelu_tanh)}))
        qkv = rnd(T, 3 * C).to(dt).requires_grad_()
        perm = torch.randperm(T, generator=g, device=dev)
        inv = torch.empty_like(perm)
        inv[perm] = torch.arange(T, device=dev)
        dq = rnd(T, 3 * C).to(dt)

        def gather_torch():
            qkv.grad = None
            q, k, v = (qkv[:, i * C:(i + 1) * C][perm] for i in range(3))
            torch.autograd.backward([q, k, v], [dq[:, :C], dq[:, C:2 * C], dq[:, 2 * C:]])

        def gather_hip():
            qkv.grad = None
            S.gather_rows(qkv, perm, inv).backward(dq)
        report(f"gather of packed qkv rows [{T}, {3 * C}] {dt}: forward + backward", alternate({"torch": gather_torch, "hip": gather_hip}))
    h = rnd(T, 2 * L).requires_grad_()
    eps, dz = rnd(T, L), rnd(T, L)

    def post_torch():
        h.grad = None
        m, lv = h.chunk(2, dim=-1)
        z = m + torch.exp(0.5 * lv) * eps
        kl = 0.5 * torch.mean(m.pow(2) + lv.exp() - lv - 1)
        torch.autograd.backward([z, kl], [dz, torch.ones_like(kl)])

    def post_hip():
        h.grad = None
        z, kl = S.posterior(h, eps)
        torch.autograd.backward([z, kl], [dz, torch.ones_like(kl)])
    report(f"posterior + KL [{T}, {2 * L}]: forward + backward", alternate({"torch": post_torch, "hip": post_hip}))
    from gvfdiffusion_amd.representations.gaussian.gaussian_model import GaussianModel
    for act in ("exp", "softplus"):
        gm = GaussianModel(mininum_kernel_size=9e-4, scaling_bias=0.004, opacity_bias=0.1, scaling_activation=act, device=dev)
        gm._scaling = (rnd(T * NG, 3) * 0.5).requires_grad_()
        gm._opacity = rnd(T * NG, 1).requires_grad_()
        bs, bo = float(gm.scale_bias), float(gm.opacity_bias)

        def reg_torch():
            gm._scaling.grad = gm._opacity.grad = None
            (torch.prod(gm.get_scaling, dim=1).mean() + (gm.get_opacity - 1).pow(2).mean()).backward()

        def reg_hip():
            gm._scaling.grad = gm._opacity.grad = None
            vol, opa = S.gaussian_reg(gm._scaling, gm._opacity, bs, bo, gm.mininum_kernel_size, act)
            (vol + opa).backward()
        report(f"volume + opacity regularisers, {T * NG} Gaussians, {act}: forward + backward", alternate({"torch": reg_torch, "hip": reg_hip}))


class FourInTorch(sparse_train.HipOps):
    """HipOps with the four new operators as the torch compositions they replace"""
    gelu_tanh = staticmethod(R.TorchOps.gelu_tanh)
    gather_rows = staticmethod(R.TorchOps.gather_rows)
    posterior = staticmethod(R.TorchOps.posterior)


class TorchAroundHipAttention(R.TorchOps):
    attention_varlen = staticmethod(sparse_train.HipOps.attention_varlen)


def full_section():
    g = torch.Generator().manual_seed(1)
    c = torch.unique(torch.randint(0, 64, (3 * T, 3), generator=g), dim=0)
    c = c[torch.randperm(c.shape[0], generator=g)[:T]]
    coords = torch.cat([torch.zeros((c.shape[0], 1), dtype=torch.long), c], dim=1).int().to(dev)
    feats = torch.randn((coords.shape[0], 1024), generator=g).to(dev)
    noise = torch.randn((coords.shape[0], L), generator=g).to(dev)
    W = torch.randn((coords.shape[0], 112), generator=g).to(dev)
    torch.manual_seed(0)
    m = SparseTransformerVAE(resolution=64, in_channels=1024, model_channels=C, out_channels=112, latent_channels=L, num_blocks=BLOCKS,
                             num_heads=12, mlp_ratio=4, attn_mode="swin", window_size=8, use_fp16=True, use_old_attn_impl=True, norm_output=True)
    for lin in (m.to_latent, m.out_layer):
        torch.nn.init.xavier_uniform_(lin.weight)
    m = m.to(dev)
    x = sp.SparseTensor(feats, coords)
    for dt in (torch.float16, torch.bfloat16):
        def step(make_ops):
            def f():
                m.enable_training(dtype=dt, ops=make_ops())
                for p in m.parameters():
                    p.grad = None
                loss, _ = R.model_loss(m, x, noise, W)
                loss.backward()
            return f
        res = alternate({"torch": step(TorchAroundHipAttention), "four in torch": step(FourInTorch), "hip": step(lambda: None)}, n=max(2, N_STEPS // 5))
        report(f"backbone forward + backward, {BLOCKS} + {BLOCKS} blocks, {C} channels, {coords.shape[0]} voxels, {dt}", res)


if __name__ == "__main__":
    print(torch.cuda.get_device_name(0))
    if "ops" in SECTIONS:
        ops_section()
    if "full" in SECTIONS:
        full_section()
