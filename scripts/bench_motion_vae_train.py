"""The motion-VAE training route (model/autoencoder_train.py on ops/vae_train.py, csrc/vae_train.hip) against its torch compositions.  GPU only.

  1. each new operator forward + backward against the torch composition a user would write, at the released sizes (dim 768, 512 latents,
     8192 inputs, T = 24, B = 1), fp16 and bf16 where the operator has a 16-bit type:
       geglu             x * F.gelu(g) on the [12288, 6144] output of net.0
       embed             LN(Linear(r)) + LN(PointEmbed(xyz)): the 8192 decoder queries (14 columns, with the gradient of the rows) and the
                         196 608 encoder context rows (6 columns, without)
       posterior_groups  clamp, sample and the 24 per-frame KL terms on [12288, 16]
  2. forward + backward at the released config (tests/golden/vae_manifest.json: depth 12, dim 768, 12 heads): decode with P = one chunk of
     8192 queries and with four chunks, and encode_rows -> decode; the HIP operators against tests/vae_train_ref.py::TorchOps for every
     element-wise operator and projection around the SAME HIP attention (so the difference is the new route's operators, not attention).
The sides alternate in one process, GVF_ROUNDS times, device events around GVF_STEPS calls; min .. max over the rounds.
GVF_BENCH_SECTIONS (default "ops,full") selects the sections; GVF_BENCH_DEPTH (default 12) the latent blocks."""
import os
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from gvfdiffusion_amd.model import autoencoder_train as AT  # noqa: E402
from gvfdiffusion_amd.model.autoencoder import GSKLTemporalVariationalAutoEncoder  # noqa: E402
from gvfdiffusion_amd.ops import vae_train as V  # noqa: E402
import vae_train_ref as R  # noqa: E402

dev = torch.device("cuda:0")
N_STEPS = int(os.environ.get("GVF_STEPS", 20))
ROUNDS = int(os.environ.get("GVF_ROUNDS", 3))
SECTIONS = set(os.environ.get("GVF_BENCH_SECTIONS", "ops,full").split(","))
DEPTH = int(os.environ.get("GVF_BENCH_DEPTH", 12))
C, HEADS, L, N, T, DL, HID, CHUNK = 768, 12, 512, 8192, 24, 16, 3072, 8192


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


def report(title, res, base="torch"):
    print(title)
    for k, v in res.items():
        ratio = "" if k == base else f"   torch / this = {min(res[base]) / min(v):.2f} x"
        print(f"    {k:<22s} {min(v):.3f} .. {max(v):.3f} ms{ratio}", flush=True)


def ops_section():
    g = torch.Generator(device=dev).manual_seed(0)
    rnd = lambda *s: torch.randn(s, generator=g, device=dev)   # noqa: E731
    M = T * L
    for dt in (torch.float16, torch.bfloat16):
        u = (rnd(M, 2 * HID) * 2).to(dt).requires_grad_()
        da = rnd(M, HID).to(dt)

        def geglu(fn):
            def f():
                u.grad = None
                fn(u).backward(da)
            return f
        report(f"geglu [{M}, {2 * HID}] {dt}: forward + backward", alternate({"torch": geglu(R.TorchOps.geglu), "hip": geglu(V.geglu)}))
    E = C // 6
    omega = (1.0 / 10000 ** (torch.arange(E, dtype=torch.float64) / (E / 2.0))).float().to(dev)
    for P, qdim, want_dr in ((CHUNK, 14, True), (T * N, 6, False)):
        r = rnd(P, qdim) * 0.5
        r[:, :3] = torch.rand((P, 3), generator=g, device=dev) - 0.5
        r.requires_grad_(want_dr)
        W, b = (rnd(C, qdim) * 0.3).requires_grad_(), (rnd(C) * 0.1).requires_grad_()
        de = rnd(P, C)

        def emb(fn):
            def f():
                r.grad = W.grad = b.grad = None
                fn(r, W, b, omega).backward(de)
            return f
        report(f"embed [{P}, {qdim}] -> [{P}, {C}], rows' gradient {'on' if want_dr else 'off'}: forward + backward",
               alternate({"torch": emb(R.TorchOps.embed), "hip": emb(V.embed)}))
    mean, logvar = rnd(M, DL).requires_grad_(), (rnd(M, DL) - 1).requires_grad_()
    eps, dz, dkl = rnd(M, DL), rnd(M, DL), torch.ones(T, device=dev)

    def post(fn):
        def f():
            mean.grad = logvar.grad = None
            z, kl = fn(mean, logvar, eps, T)
            torch.autograd.backward([z, kl], [dz, dkl])
        return f
    report(f"posterior_groups [{M}, {DL}], {T} groups: forward + backward", alternate({"torch": post(R.TorchOps.posterior_groups), "hip": post(V.posterior_groups)}))


class TorchAroundHipAttention(R.TorchOps):
    attention = staticmethod(AT.HipOps.attention)


def full_section():
    g = torch.Generator().manual_seed(1)
    torch.manual_seed(0)
    m = GSKLTemporalVariationalAutoEncoder(depth=DEPTH, dim=C, queries_dim=C, output_dim=14, num_inputs=N, num_latents=L, latent_dim=DL, heads=HEADS,
                                           num_timesteps=T, chunk_size=CHUNK)
    with torch.no_grad():
        m.to_outputs.weight.normal_(std=0.02)
    m = m.to(dev)
    x = torch.randn((T, L, DL), generator=g).to(dev)
    static_pc = (torch.rand((1, N, 3), generator=g) - 0.5).to(dev)
    delta_pc = (torch.randn((1, T, N, 3), generator=g) * 0.05).to(dev)
    sampled = (torch.rand((1, L, 3), generator=g) - 0.5).to(dev)
    est = (torch.randn((1, T, L, 3), generator=g) * 0.05).to(dev)
    noise = torch.randn((T * L, DL), generator=g).to(dev)
    for dt in (torch.float16, torch.bfloat16):
        for P in (CHUNK, 4 * CHUNK):
            q = torch.randn((1, P, 14), generator=g)
            q[..., :3] = torch.rand((1, P, 3), generator=g) - 0.5
            q = q.to(dev)
            W = torch.randn((1, T, P, 14), generator=g).to(dev)

            def step(make_ops, with_encoder):
                def f():
                    m.enable_training(dtype=dt, ops=make_ops())
                    for p in m.parameters():
                        p.grad = None
                    if with_encoder:
                        kl, z, _ = m.encode_rows(static_pc, delta_pc, sampled, est, noise=noise)
                        loss = (m.decode(z, q) * W).sum() / W.numel() + kl.mean()
                    else:
                        loss = (m.decode(x, q) * W).sum() / W.numel()
                    loss.backward()
                    f.loss = loss.detach()
                return f
            for with_encoder in ((False, True) if P == CHUNK else (False,)):
                sides = {"torch": step(TorchAroundHipAttention, with_encoder), "hip": step(lambda: None, with_encoder)}
                res = alternate(sides, n=max(2, N_STEPS // 5))
                what = "encode_rows -> decode" if with_encoder else "decode"
                report(f"{what} forward + backward, depth {DEPTH}, dim {C}, {L} latents, T = {T}, P = {P} ({P // CHUNK} chunk(s)), {dt}", res)
                print("    loss: " + ", ".join(f"{k} {float(fn.loss):.6f}" for k, fn in sides.items()), flush=True)


if __name__ == "__main__":
    print(torch.cuda.get_device_name(0))
    if "ops" in SECTIONS:
        ops_section()
    if "full" in SECTIONS:
        full_section()
