"""Generates tests/golden/dit_small_train_golden.npz (+ dit_small_train_golden_b.npz): the REFERENCE's own diffusion training loss and
parameter gradients on the reduced DiT of dit_small_golden.npz.  Like make_golden.py it imports the reference, runs only in the build
container and never travels; the files it writes are data.

    python tests/golden/make_dit_train_golden.py

The reference's DiT(**DIT_SMALL) with the weights and inputs of dit_small_golden.npz (its `x` is the clean latent x_start) and the
reference's create_gaussian_diffusion(**configs/diffusion.yml:diffusion) -> training_losses at integer steps t = [998, 431] with a seeded
noise.  Stored: the diffusion settings, t, noise, x_t, the target, terms["mse"], terms["loss"], the fp32 gradient of loss.mean() for every parameter ("grad.<name>"),
and -- scalars only -- what the reference's own mixed-precision runs deviate from that: torch.autocast("cpu", bf16), and fp16 with the loss
scaled by 1024 and the gradients unscaled (without a scale the fp16 run loses the gradients of the RMS gains): per-parameter and
whole-gradient relative L2 ("rel_bf16.<name>", "rel_bf16_total", ...), the relative deviation of the loss ("loss_rel_bf16", ...).
A committed file stays below 1 MiB, so the gradients of the second block travel in the _b file."""
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden import DIT_SMALL, REF, install_stubs  # noqa: E402

FP16_LOSS_SCALE = 1024.0
T_STEPS = [998, 431]


def main():
    import yaml
    install_stubs()
    from model.dit import DiT
    from utils.script_util import create_gaussian_diffusion
    g = np.load(os.path.join(HERE, "dit_small_golden.npz"))
    torch.manual_seed(0)
    model = DiT(**DIT_SMALL)
    model.load_state_dict({k[3:]: torch.from_numpy(g[k]) for k in g.files if k.startswith("sd.")})
    dcfg = yaml.safe_load(open(f"{REF}/configs/diffusion.yml"))["diffusion"]
    diffusion = create_gaussian_diffusion(**dcfg)
    x_start = torch.from_numpy(g["x"])
    kw = dict(cond_images=torch.from_numpy(g["cond_images"]), static_latent=torch.from_numpy(g["static_latent"]),
              deformation_position_xyz=torch.from_numpy(g["xyz"]))
    t = torch.tensor(T_STEPS, dtype=torch.long)
    noise = torch.randn(x_start.shape, generator=torch.Generator().manual_seed(7))
    names = [n for n, _ in model.named_parameters()]

    def run(scale=1.0):
        model.zero_grad(set_to_none=True)
        terms, aux = diffusion.training_losses(lambda x, ts, **k: model._forward(x, ts, **k), x_start, t, model_kwargs=kw, noise=noise)
        loss = terms["loss"].float().mean()
        (loss * scale).backward()
        return terms, aux, loss.detach(), {n: p.grad.detach().float() / scale for n, p in model.named_parameters()}

    terms, aux, loss, grads = run()
    assert all(float(grads[n].abs().max()) > 0 for n in names), [n for n in names if float(grads[n].abs().max()) == 0]
    target = diffusion.get_v(x_start, noise, t) if diffusion.model_mean_type.name == "V" else None
    assert target is not None
    out = {"t": t.numpy(), "noise": noise.numpy(), "x_t": aux["x_t"].numpy(), "target": target.numpy(), "mse": terms["mse"].detach().numpy(),
           "loss_terms": terms["loss"].detach().numpy(), "loss": np.float32(loss), "model_output": aux["model_output"].detach().numpy(),
           "fp16_loss_scale": np.float64(FP16_LOSS_SCALE), "diffusion_json": np.frombuffer(json.dumps(dcfg).encode(), dtype=np.uint8), "n_params": np.int64(sum(grads[n].numel() for n in names))}
    out_b = {}
    for n in names:
        (out_b if n.startswith("blocks.1.") else out)["grad." + n] = grads[n].numpy()
    flat = torch.cat([grads[n].reshape(-1) for n in names]).double()
    for name, dt, scale in (("bf16", torch.bfloat16, 1.0), ("fp16", torch.float16, FP16_LOSS_SCALE)):
        with torch.autocast("cpu", dtype=dt):
            _, _, l_a, g_a = run(scale)
        out[f"loss_rel_{name}"] = np.float64(abs(float(l_a) - float(loss)) / abs(float(loss)))
        for n in names:
            out[f"rel_{name}.{n}"] = np.float64(float((g_a[n].double() - grads[n].double()).norm() / grads[n].double().norm()))
        fa = torch.cat([g_a[n].reshape(-1) for n in names]).double()
        out[f"rel_{name}_total"] = np.float64(float((fa - flat).norm() / flat.norm()))
        rels = [float(out[f"rel_{name}.{n}"]) for n in names]
        print(f"{name}: loss rel {float(out[f'loss_rel_{name}']):.3e}, whole gradient {float(out[f'rel_{name}_total']):.3e}, per tensor "
              f"{min(rels):.3e} .. {max(rels):.3e} (largest: {names[int(np.argmax(rels))]})")
    np.savez_compressed(os.path.join(HERE, "dit_small_train_golden.npz"), **out)
    np.savez_compressed(os.path.join(HERE, "dit_small_train_golden_b.npz"), **out_b)
    for f in ("dit_small_train_golden.npz", "dit_small_train_golden_b.npz"):
        print(f, os.path.getsize(os.path.join(HERE, f)), "bytes")
    print("loss", float(loss), "params", int(out["n_params"]))


if __name__ == "__main__":
    main()
