"""The DiT training operators (ops/dit_train.py on csrc/dit_train.hip) against the torch composition of the same operator with the same
storage types, both reached through the `ops=` seam of model/dit_train.py (tests/dit_train_ref.py::TorchOps is the baseline namespace).
GPU only.

  1. each operator forward + backward at the DiT's shapes: rows = B * 24 * 512, C = 512, H = 16, d = 32, B in {1, 4}, fp16 and bf16;
     LayerNorm + adaLN modulate with the shift / scale chunk views of a [B, 6C] tensor, the gated residual with its gate view, the RMSNorm on
     the q slice of a packed [rows, 3C] projection.  The two sides alternate in one process, ROUNDS times; min .. max over the rounds.
  2. the three backward entry points alone (partials kernel + finaliser) on preallocated buffers: counted bytes / time, next to the
     optimizer step's 5.2 TB/s (profiles/r13_optim_step.txt).
  3. one full-size DiT forward + backward (tests/golden/dit_manifest.json = configs/diffusion.yml, B 1, T 24, N 512, seed-generated weights):
     the HIP operators; the torch element-wise operators around the HIP attention (isolates the three operators); torch everywhere
     (scaled_dot_product_attention).
Counted bytes per element (compulsory traffic: every row read or written once): LayerNorm fwd 6 (x 4, y 2) + bwd 10 (x 4, dy 2, dx 4);
gate fwd 10 (x 4, h 2, out 4) + bwd 8 (dout 4, h 2, dh 2); RMSNorm fwd 4 + bwd 6."""
import ctypes
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from gvfdiffusion_amd import _lib, synthetic  # noqa: E402
from gvfdiffusion_amd.model import dit_train  # noqa: E402
from gvfdiffusion_amd.model.dit import DiT  # noqa: E402
from gvfdiffusion_amd.ops import dit_ops  # noqa: E402
from gvfdiffusion_amd.ops import dit_train as T  # noqa: E402
import dit_train_ref as R  # noqa: E402

dev = torch.device("cuda:0")
N_STEPS = int(os.environ.get("GVF_STEPS", 20))
ROUNDS = int(os.environ.get("GVF_ROUNDS", 3))
FULL = os.environ.get("GVF_BENCH_FULL", "1") != "0"
C, H, D, TN = 512, 16, 32, 24 * 512
HIP, TORCH = dit_train.HipOps, R.TorchOps()


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
    """{name: [ms per round]}: the sides take turns, ROUNDS times"""
    out = {k: [] for k in sides}
    for _ in range(ROUNDS):
        for k, fn in sides.items():
            out[k].append(timed(fn, n))
    return out


def span(v):
    return f"{min(v):.3f} .. {max(v):.3f}"


def op_sides(B, dt):
    rows = B * TN
    g = torch.Generator(device=dev).manual_seed(B)
    rnd = lambda *s: torch.randn(s, generator=g, device=dev)
    x = rnd(B, TN, C).requires_grad_()
    mod = (0.3 * rnd(B, 6 * C)).requires_grad_()
    sh, sc, gt = mod.chunk(6, dim=1)[:3]
    dy16, dout = rnd(B, TN, C).to(dt), rnd(B, TN, C)
    h16 = rnd(B, TN, C).to(dt).requires_grad_()
    qkv = rnd(rows, 3, H, D).to(dt).requires_grad_()
    gamma = (1 + 0.1 * rnd(H, D)).requires_grad_()
    dq = rnd(rows, H, D).to(dt)
    leaves = (x, mod, h16, qkv, gamma)

    def clear():
        for t in leaves:
            t.grad = None

    def ln(ops):
        def f():
            clear()
            y, _ = ops.layernorm_modulate(x, shift=sh, scale=sc, rows_per_group=TN, dtype=dt)
            y.backward(dy16)
        return f

    def gate(ops):
        def f():
            clear()
            ops.gate_residual(x, h16, gt, TN).backward(dout)
        return f

    def rms(ops):
        def f():
            clear()
            ops.rmsnorm_heads(qkv[:, 0], gamma).backward(dq)
        return f
    n = rows * C
    return {"layernorm_modulate": (ln, 16 * n), "gate_residual": (gate, 18 * n), "rmsnorm_heads": (rms, 10 * n)}


def backward_kernels(B, dt):
    """the three backward entry points alone, on buffers of the caller's"""
    rows = B * TN
    code = dit_ops.dt_code(dt)
    p = lambda t: None if t is None else ctypes.c_void_p(t.data_ptr())
    x, dres, dout = (torch.randn((rows, C), device=dev) for _ in range(3))
    dy, h = torch.randn((rows, C), device=dev).to(dt), torch.randn((rows, C), device=dev).to(dt)
    mod = 0.3 * torch.randn((B, 6 * C), device=dev)
    dx, dh = torch.empty_like(x), torch.empty_like(h)
    ds, dc, dg = (torch.empty((B, C), device=dev) for _ in range(3))
    qkv, dq = torch.randn((rows, 3 * C), device=dev).to(dt), torch.randn((rows, C), device=dev).to(dt)
    dxq, gamma, dgamma = torch.empty_like(dq), torch.ones((H, D), device=dev), torch.empty((H, D), device=dev)
    ws = {n: T._workspace(n, dev, *a) for n, a in (("gvf_ln_mod_bwd_workspace_bytes", (rows, C, TN)), ("gvf_gate_residual_bwd_workspace_bytes", (rows, C, TN)),
                                                   ("gvf_rmsnorm_heads_bwd_workspace_bytes", (rows, H, D)))}
    l, st = _lib.lib(), _lib.current_stream(dev)
    w0, w1, w2 = ws.values()
    sides = {
        "ln_mod_bwd": lambda: _lib.check(l.gvf_ln_mod_bwd(code, p(x), p(dy), p(dres), p(dx), rows, C, 1e-6, None, None, p(mod[:, C:]), 6 * C, TN, p(ds), p(dc),
                                                          None, None, p(w0), w0.numel(), st), "ln"),
        "gate_residual_bwd": lambda: _lib.check(l.gvf_gate_residual_bwd(code, p(dout), p(h), p(mod[:, 2 * C:]), 6 * C, TN, p(dh), p(dg), rows, C, p(w1), w1.numel(), st), "gate"),
        "rmsnorm_heads_bwd": lambda: _lib.check(l.gvf_rmsnorm_heads_bwd(code, p(qkv), 3 * C, p(dq), C, p(gamma), p(dxq), C, p(dgamma), rows, H, D, p(w2), w2.numel(), st), "rms"),
    }
    n = rows * C
    nbytes = {"ln_mod_bwd": 14 * n, "gate_residual_bwd": 8 * n, "rmsnorm_heads_bwd": 6 * n}     # (ln: x 4, dy 2, dres 4, dx 4)
    return sides, nbytes


def full_model():
    man = json.load(open(os.path.join(ROOT, "tests", "golden", "dit_manifest.json")))
    net = DiT(**man["config"])
    net.load_state_dict(synthetic.dit_state_dict(man["state_dict"], seed=0))
    net = net.to(dev)
    inp = {k: v.to(dev) for k, v in synthetic.dit_inputs(B=1, T=24, seed=1).items()}
    target = torch.randn_like(inp["x"])

    class TorchAroundHipAttention(R.TorchOps):
        def attention(self, q, k, v):
            return HIP.attention(q, k, v)

    def step(ops, dt):
        def f():
            net.zero_grad(set_to_none=True)
            y = dit_train.forward_train(net, inp["x"], inp["t"], inp["cond_images"], inp["static_latent"], inp["deformation_position_xyz"], ops=ops, dtype=dt)
            ((y - target) ** 2).mean().backward()
        return f
    for dt, name in ((torch.float16, "fp16"), (torch.bfloat16, "bf16")):
        sides = {"hip operators": step(None, dt), "torch operators + hip attention": step(TorchAroundHipAttention(), dt),
                 "torch operators + torch sdpa": step(R.TorchOps(attention="sdpa"), dt)}
        try:
            sides["torch operators + torch sdpa"]()
        except Exception as e:                                   # noqa: BLE001  (a torch build without a fused attention backward for this shape)
            print(f"  torch sdpa side not runnable here: {type(e).__name__}: {e}")
            del sides["torch operators + torch sdpa"]
        res = alternate(sides, n=max(2, N_STEPS // 5))
        base = min(res["hip operators"])
        print(f"full-size DiT forward + backward, B 1 T 24 N 512, {name}:")
        for k, v in res.items():
            print(f"  {k:34s} {span(v)} ms   ({min(v) / base:.2f} x the hip operators)")


def main():
    print(torch.cuda.get_device_name(0), _lib.lib().gvf_version().decode(), f"; {N_STEPS} steps x {ROUNDS} rounds, ms per call: min .. max of the rounds", flush=True)
    for dt, name in ((torch.float16, "fp16"), (torch.bfloat16, "bf16")):
        for B in (1, 4):
            print(f"operators forward + backward, rows = {B} x 24 x 512, C 512, H 16, d 32, {name}:")
            for op, (make, nbytes) in op_sides(B, dt).items():
                res = alternate({"hip": make(HIP), "torch": make(TORCH)})
                print(f"  {op:20s} hip {span(res['hip'])} ms  torch {span(res['torch'])} ms  torch / hip {min(res['torch']) / min(res['hip']):.2f} x   "
                      f"hip {nbytes / min(res['hip']) / 1e9:.2f} TB/s on {nbytes / 1e6:.0f} MB counted", flush=True)
            sides, nb = backward_kernels(B, dt)
            res = alternate(sides)
            for k, v in res.items():
                print(f"  {k:20s} alone {span(v)} ms  {nb[k] / min(v) / 1e9:.2f} TB/s on {nb[k] / 1e6:.0f} MB counted (optimizer step: 5.2 TB/s)", flush=True)
    if FULL:
        full_model()


if __name__ == "__main__":
    main()
