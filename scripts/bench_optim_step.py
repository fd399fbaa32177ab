"""Fused clip + AdamW + EMA optimizer step (ops/optim.py::FusedAdamW: norm, finalize and update launches plus the fill of the flat
gradient buffer) against the same step composed in torch, on the parameter shapes of the DiT of tests/golden/dit_manifest.json
(446 tensors, 105.5 M fp32 parameters), one EMA at 0.9999, clip at 1.0.  GPU only.

Two compositions, alternated with the fused step in one process on one box:
  reference   the reference's own optimize(): clip_grad_norm_, AdamW.step() with its defaults, zero_grad(), and update_ema written out
              (a Python loop of mul_().add_() per tensor);
  torch-best  the fastest stock torch offers: clip_grad_norm_ (foreach), AdamW(fused=True), torch._foreach_mul_ / _foreach_add_ for
              the EMA, zero_grad(set_to_none=True).
Every variant starts each step from the same gradient values (one flat device copy, inside the timed region of all three, so it
cancels in the differences and is reported on its own).  A plain device copy of 44 B x N / 2 bytes (read + write = 44 B x N moved) is
the box's yardstick.  Prints ms, the two ratios, TB/s on the counted 44 B per parameter and the fraction of the copy rate.
GVF_BENCH_MODE=f runs the fused step alone (for a kernel trace)."""
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from gvfdiffusion_amd.ops.optim import FlatGrads, FusedAdamW  # noqa: E402

dev = torch.device("cuda:0")
N_STEPS = int(os.environ.get("GVF_STEPS", 20))
ROUNDS = int(os.environ.get("GVF_ROUNDS", 3))
MODE = os.environ.get("GVF_BENCH_MODE", "all")
LR, BETAS, EPS, WD, RATE, CLIP = 1e-4, (0.9, 0.999), 1e-8, 0.01, 0.9999, 1.0
BYTES_PER_PARAM = 44      # norm pass 4 (g), update pass 36 (p, g, m, v, e read; p, m, v, e written), fill 4


def dit_params(seed):
    shapes = json.load(open(os.path.join(ROOT, "tests", "golden", "dit_manifest.json")))["state_dict"]
    g = torch.Generator(device=dev).manual_seed(seed)
    return [torch.nn.Parameter(0.02 * torch.randn(tuple(s), generator=g, device=dev)) for s in shapes.values()]


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


params_f = dit_params(0)
N = sum(p.numel() for p in params_f)
print(f"{len(params_f)} tensors, {N} parameters ({min(p.numel() for p in params_f)} .. {max(p.numel() for p in params_f)} elements)", flush=True)

fused = FusedAdamW(params_f, lr=LR, betas=BETAS, eps=EPS, weight_decay=WD, ema_rates=(RATE,), max_grad_norm=CLIP)
grad_src = 1e-3 * torch.randn(fused.flat_grads.buffer.numel(), device=dev)      # the gradients of every step, in the flat layout


def step_fused():
    fused.flat_grads.buffer.copy_(grad_src)
    fused.step()
    fused.zero_grad()


def step_copy_only():
    fused.flat_grads.buffer.copy_(grad_src)


variants = {"fused": step_fused}
if MODE == "all":
    def composed(make_opt, ema_update, set_to_none):
        ps = dit_params(0)
        flat = FlatGrads(ps)          # only to load the same gradient values with one copy; the optimizers below see ordinary .grad tensors
        opt = make_opt(ps)
        ema = [p.detach().clone() for p in ps]

        def step():
            flat.attach()             # zero_grad dropped the .grad tensors (a training step's backward would allocate new ones)
            flat.buffer.copy_(grad_src)
            torch.nn.utils.clip_grad_norm_(ps, CLIP)
            opt.step()
            if set_to_none:
                opt.zero_grad(set_to_none=True)
            else:
                opt.zero_grad()       # the reference's call; torch's default drops the gradients as well
            ema_update(ema, ps)
        return step

    def ema_loop(ema, ps):            # the reference's update_ema
        for e, p in zip(ema, ps):
            e.mul_(RATE).add_(p.detach(), alpha=1 - RATE)

    def ema_foreach(ema, ps):
        torch._foreach_mul_(ema, RATE)
        torch._foreach_add_(ema, [p.detach() for p in ps], alpha=1 - RATE)

    variants["reference"] = composed(lambda ps: torch.optim.AdamW(ps, lr=LR, betas=BETAS, eps=EPS, weight_decay=WD), ema_loop, False)
    variants["torch-best"] = composed(lambda ps: torch.optim.AdamW(ps, lr=LR, betas=BETAS, eps=EPS, weight_decay=WD, fused=True),
                                      ema_foreach, True)
    half = torch.empty(BYTES_PER_PARAM * N // 8, dtype=torch.float32, device=dev)
    dst = torch.empty_like(half)
    variants["copy-44B"] = lambda: dst.copy_(half)
    variants["grad-load"] = step_copy_only
    attach_flat = FlatGrads(dit_params(0))

    def step_attach_only():           # the host cost of handing the gradients back, which the two compositions carry and the fused step does not
        for p in attach_flat.params:
            p.grad = None
        attach_flat.attach()
    variants["grad-attach"] = step_attach_only

best = {k: float("inf") for k in variants}
for r in range(ROUNDS):               # alternate: every variant sees the same box in the same minute
    for name, fn in variants.items():
        t = timed(fn, N_STEPS)
        best[name] = min(best[name], t)
        print(f"round {r}: {name} {t:.3f} ms", flush=True)

tf = best["fused"]
if MODE == "all":
    load = best["grad-load"]
    net = {k: best[k] - load for k in ("fused", "reference", "torch-best")}
    print(f"best of {ROUNDS} rounds x {N_STEPS} steps, the gradient load ({load:.3f} ms) subtracted (the compositions also carry "
          f"{best['grad-attach']:.3f} ms of host time for re-attaching the dropped gradients, not subtracted):")
    print(f"  fused step + fill          {net['fused']:.3f} ms")
    print(f"  reference composition      {net['reference']:.3f} ms   {net['reference'] / net['fused']:.2f}x the fused step")
    print(f"  torch's best composition   {net['torch-best']:.3f} ms   {net['torch-best'] / net['fused']:.2f}x the fused step")
    moved = BYTES_PER_PARAM * N
    rate, copy_rate = moved / net["fused"] / 1e9, moved / best["copy-44B"] / 1e9
    print(f"  device copy of {moved / 1e9:.2f} GB moved {best['copy-44B']:.3f} ms = {copy_rate:.2f} TB/s")
    print(f"  fused: {rate:.2f} TB/s on the counted {BYTES_PER_PARAM} B per parameter, {rate / copy_rate:.2f} of the copy rate")
    print("  fused is " + ("FASTER than both compositions" if net["fused"] < min(net["reference"], net["torch-best"])
                           else "NOT faster than both compositions"))
else:
    print(f"fused step + fill + gradient load: {tf:.3f} ms")
