"""Attention backward (ops/attention_grad.py: csrc/attn_bwd.hip) at the six model shapes, fp16 and bf16, against
  - this package's own forward at the same shape (the ratio: 3.5x is the FLOP ratio of 7 products plus the statistics pass to the
    forward's 2),
  - torch's backward of softmax(q k^T * scale) v composed in the same dtype (matmul, softmax, matmul; chunked over the batch where the
    score matrix would not fit the chunk budget): the only backward a user of this package had before,
  - torch.nn.functional.scaled_dot_product_attention's backward, where this build has a fused one that runs here (reported, no bar).
GPU only.  All sides alternate in one process: ROUNDS windows of GVF_STEPS / ROUNDS calls per side (default 20 calls), device events
around each window, after a warm-up call of every side.  Prints ms, the ratios and the achieved TFLOP/s on flash-attn's count of
10 N^2 D per (sequence, head) for the backward (4 N^2 D for the forward); our backward executes 16 (7 products plus the statistics
pass) of which 10 are counted."""
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from gvfdiffusion_amd.ops import attention_grad as AG, dit_ops  # noqa: E402

dev = torch.device("cuda:0")
N_STEPS = int(os.environ.get("GVF_STEPS", 20))
ROUNDS = 4
SCORE_BUDGET = 1 << 28                              # score elements per chunk of the composed backward

SHAPES = [("DiT spatial", 24, 512, 512, 16, 32), ("DiT temporal", 512, 24, 24, 16, 32), ("image cross", 4, 512, 1370, 16, 32),
          ("static cross", 2, 512, 4096, 16, 32), ("VAE self", 2, 512, 512, 12, 64), ("VAE decoder cross", 1, 8192, 512, 12, 64)]


def timed(fns, n):
    """ms per call of every function: ROUNDS alternating windows of n / ROUNDS calls each, after one warm-up call of each."""
    for f in fns:
        f()
    torch.cuda.synchronize()
    per = max(1, n // ROUNDS)
    tot = [0.0] * len(fns)
    for _ in range(ROUNDS):
        for i, f in enumerate(fns):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(per):
                f()
            e1.record()
            torch.cuda.synchronize()
            tot[i] += e0.elapsed_time(e1)
    return [t / (per * ROUNDS) for t in tot]


def composed_graph(q, k, v, scale):
    """Forward of the composition kept as autograd graphs (one per batch chunk); returns a function that runs their backward."""
    N, Lq, H, _ = q.shape
    per = max(1, min(N, SCORE_BUDGET // (H * Lq * k.shape[1])))
    leaves, outs = [], []
    for n0 in range(0, N, per):
        ql, kl, vl = (t[n0:n0 + per].detach().permute(0, 2, 1, 3).contiguous().requires_grad_(True) for t in (q, k, v))
        p = torch.softmax(torch.matmul(ql, kl.transpose(-1, -2)) * scale, dim=-1)
        outs.append(torch.matmul(p, vl))
        leaves.append((ql, kl, vl))
    return leaves, outs, per


def sdpa_fused_available(q, k, v):
    try:
        from torch.nn.attention import SDPBackend, sdpa_kernel
        ql, kl, vl = (t[:1].detach().permute(0, 2, 1, 3).contiguous().requires_grad_(True) for t in (q, k, v))
        with sdpa_kernel([SDPBackend.FLASH_ATTENTION, SDPBackend.EFFICIENT_ATTENTION]):
            torch.nn.functional.scaled_dot_product_attention(ql, kl, vl).sum().backward()
        torch.cuda.synchronize()
        return True
    except Exception as e:                           # no fused kernel in this build / for this GPU: say so and go on
        print(f"  (torch SDPA fused backward not available here: {type(e).__name__}: {str(e).splitlines()[0][:120]})", flush=True)
        return False


def main():
    print(f"attention backward, {N_STEPS} timed calls per side in {ROUNDS} alternating windows; TFLOP/s on 10 N^2 D (backward), 4 N^2 D (forward)")
    have_sdpa = None
    for dt in (torch.float16, torch.bfloat16):
        for name, N, Lq, Lk, H, C in SHAPES:
            g = torch.Generator().manual_seed(Lq + Lk)
            q, k, v, do = (torch.randn((N, L, H, C), generator=g).to(dev, dt) for L in (Lq, Lk, Lk, Lq))
            scale = C ** -0.5
            out = torch.empty_like(q)
            st = AG._st

            def fwd():
                dit_ops.attention(q, k, v, out, N, 1, Lq, Lk, H, st(q), st(k), st(v), st(out), scale=scale, head_dim=C)

            fwd()

            def bwd():
                AG.attention_backward(q, k, v, out, do, scale)

            leaves, outs, per = composed_graph(q, k, v, scale)
            do_hf = do.permute(0, 2, 1, 3).contiguous()

            def composed():
                for i, (o, ls) in enumerate(zip(outs, leaves)):
                    torch.autograd.grad(o, ls, do_hf[i * per:(i + 1) * per], retain_graph=True)

            fns = [bwd, fwd, composed]
            if have_sdpa is None:
                have_sdpa = sdpa_fused_available(q, k, v)
            if have_sdpa:
                from torch.nn.attention import SDPBackend, sdpa_kernel
                ql, kl, vl = (t.detach().permute(0, 2, 1, 3).contiguous().requires_grad_(True) for t in (q, k, v))
                with sdpa_kernel([SDPBackend.FLASH_ATTENTION, SDPBackend.EFFICIENT_ATTENTION]):
                    o_sdpa = torch.nn.functional.scaled_dot_product_attention(ql, kl, vl, scale=scale)
                fns.append(lambda: torch.autograd.grad(o_sdpa, (ql, kl, vl), do_hf, retain_graph=True))
            ms = timed(fns, N_STEPS)
            fl_b, fl_f = 10.0 * N * H * Lq * Lk * C, 4.0 * N * H * Lq * Lk * C
            line = (f"{name:18s} {str(dt)[6:]:8s} ({N}, {Lq}, {Lk}, H {H}, d {C}): backward {ms[0]:.3f} ms = {fl_b / ms[0] / 1e9:.1f} TFLOP/s; "
                    f"forward {ms[1]:.3f} ms = {fl_f / ms[1] / 1e9:.1f} TFLOP/s, backward / forward {ms[0] / ms[1]:.2f}x; "
                    f"torch composed backward{'' if per >= N else f' (batch chunks of {per})'} {ms[2]:.3f} ms, {ms[2] / ms[0]:.1f}x ours")
            if have_sdpa:
                line += f"; torch SDPA fused backward {ms[3]:.3f} ms, {ms[3] / ms[0]:.2f}x ours (no bar)"
            print(line, flush=True)
            del leaves, outs


if __name__ == "__main__":
    main()
