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
     (scaled_dot_product_attention); and the HIP operators with linear="hip" (the block projections on this library's GEMMs,
     ops/linear_grad.py), alternated with linear="torch" in the same process.
  4. each block projection at the released shapes (C 512, M = 24 x 512; to_kv at M = 24 x 1370 and 24 x 4096): forward (gvf_gemm), input
     gradient (gvf_gemm on the transposed image) and weight + bias gradient (gvf_gemm_wgrad) alone, time and TFLOP/s (2 M N K each), next to
     torch's F.linear forward + backward on pre-cast 16-bit weights (the linear="torch" route without its casts); the weight gradient also over
     a sweep of split counts; and the per-step cast_transpose over all block weights of the released model.
GVF_BENCH_SECTIONS (default "ops,full,linear") selects the sections.
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
from gvfdiffusion_amd.ops import _util, dit_ops  # noqa: E402
from gvfdiffusion_amd.ops import dit_train as T  # noqa: E402
import dit_train_ref as R  # noqa: E402

dev = torch.device("cuda:0")
N_STEPS = int(os.environ.get("GVF_STEPS", 20))
ROUNDS = int(os.environ.get("GVF_ROUNDS", 3))
FULL = os.environ.get("GVF_BENCH_FULL", "1") != "0"
SECTIONS = set(os.environ.get("GVF_BENCH_SECTIONS", "ops,full,linear").split(","))
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
    ws = {n: _util.scratch(n, dev, *a) for n, a in (("gvf_ln_mod_bwd_workspace_bytes", (rows, C, TN)), ("gvf_gate_residual_bwd_workspace_bytes", (rows, C, TN)),
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

    def step(ops, dt, linear="torch"):
        def f():
            net.zero_grad(set_to_none=True)
            y = dit_train.forward_train(net, inp["x"], inp["t"], inp["cond_images"], inp["static_latent"], inp["deformation_position_xyz"], ops=ops, dtype=dt,
                                        linear=linear)
            ((y - target) ** 2).mean().backward()
        return f
    for dt, name in ((torch.float16, "fp16"), (torch.bfloat16, "bf16")):
        sides = {"hip operators": step(None, dt), "hip operators, linear=hip": step(None, dt, "hip"),
                 "torch operators + hip attention": step(TorchAroundHipAttention(), dt),
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


# (name, M, N, K) of the released model's block projections (C 512, B 1, T 24, N 512; 1370 image tokens, 4096 static tokens per frame)
PROJECTIONS = [("to_qkv", TN, 1536, 512), ("to_out / to_q", TN, 512, 512), ("to_kv image", 24 * 1370, 1024, 512), ("to_kv static", 24 * 4096, 1024, 512),
               ("mlp.0", TN, 2048, 512), ("mlp.2", TN, 512, 2048)]


def linear_projections():
    import torch.nn.functional as F
    from gvfdiffusion_amd.ops import linear_grad
    for dt, name in ((torch.float16, "fp16"), (torch.bfloat16, "bf16")):
        print(f"block projections, {name}: ms (TFLOP/s at 2 M N K per product)")
        for proj, M, N, K in PROJECTIONS:
            g = torch.Generator(device=dev).manual_seed(M + N)
            x = torch.randn((M, K), generator=g, device=dev).to(dt)
            dy = torch.randn((M, N), generator=g, device=dev).to(dt)
            w = torch.randn((N, K), generator=g, device=dev) / K ** 0.5
            b = torch.randn((N,), generator=g, device=dev)
            w16, w16t = linear_grad.cast_transpose(w, dt)
            y, dx = torch.empty((M, N), dtype=dt, device=dev), torch.empty((M, K), dtype=dt, device=dev)
            dw, db = torch.empty((N, K), device=dev), torch.empty((N,), device=dev)
            auto = linear_grad.wgrad_splits(M, N, K)
            ws = torch.empty(max(linear_grad.wgrad_workspace_bytes(M, N, K, s) for s in (auto, 2 * auto, 4 * auto)), dtype=torch.uint8, device=dev)
            xt, wt, bt = x.clone().requires_grad_(), w16.clone().requires_grad_(), b.to(dt).requires_grad_()

            def torch_fb():
                xt.grad = wt.grad = bt.grad = None
                F.linear(xt, wt, bt).backward(dy)
            sides = {"forward": lambda: dit_ops.gemm(x, w16, b, y, dit_ops.EPI_STORE_16), "dgrad": lambda: dit_ops.gemm(dy, w16t, None, dx, dit_ops.EPI_STORE_16),
                     "torch fwd+bwd": torch_fb}
            cands = sorted({max(1, auto // 2), auto, 2 * auto, 4 * auto})
            for s_ in cands:
                sides[f"wgrad s={s_}"] = (lambda s_=s_: linear_grad.wgrad(dy, x, True, s_, out=dw, out_bias=db, workspace=ws))
            res = alternate(sides)
            fl = 2.0 * M * N * K
            hip3 = min(res["forward"]) + min(res["dgrad"]) + min(res[f"wgrad s={auto}"])
            print(f"  {proj:14s} M {M:6d} N {N:5d} K {K:5d}: " + "  ".join(f"{k} {span(v)} ({fl / min(v) / 1e9:.0f})" for k, v in res.items() if k != "torch fwd+bwd"))
            print(f"  {'':14s} auto splits {auto}; forward + dgrad + wgrad {hip3:.3f} ms ({3 * fl / hip3 / 1e9:.0f} TFLOP/s)  torch F.linear fwd+bwd {span(res['torch fwd+bwd'])} ms "
                  f"({3 * fl / min(res['torch fwd+bwd']) / 1e9:.0f} TFLOP/s)  torch / hip {min(res['torch fwd+bwd']) / hip3:.2f} x", flush=True)
        man = json.load(open(os.path.join(ROOT, "tests", "golden", "dit_manifest.json")))
        nb = int(man["config"]["num_blocks"])
        shapes = [(1536, 512), (512, 512)] * 2 + [(512, 512), (1024, 512), (512, 512)] * 2 + [(2048, 512), (512, 2048)]
        ws_ = [torch.randn(s, device=dev) for s in shapes]
        t = timed(lambda: [linear_grad.cast_transpose(w_, dt) for w_ in ws_], N_STEPS)
        n_el = sum(a * b_ for a, b_ in shapes)
        print(f"  cast_transpose of one block's 12 weights ({n_el / 1e6:.2f} M elements, 8 bytes each counted): {t:.3f} ms = {8 * n_el / t / 1e9:.2f} TB/s; "
              f"x {nb} blocks = {t * nb:.2f} ms per step", flush=True)


def main():
    print(torch.cuda.get_device_name(0), _lib.lib().gvf_version().decode(), f"; {N_STEPS} steps x {ROUNDS} rounds, ms per call: min .. max of the rounds", flush=True)
    for dt, name in ((torch.float16, "fp16"), (torch.bfloat16, "bf16")) if "ops" in SECTIONS else ():
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
    if "linear" in SECTIONS:
        linear_projections()
    if FULL and "full" in SECTIONS:
        full_model()


if __name__ == "__main__":
    main()
