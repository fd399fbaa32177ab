"""Ragged attention, forward + backward (ops/attention_grad.py::attention_varlen: csrc/attn.hip + the ragged form of csrc/attn_bwd.hip) at the
static VAE's windowed-attention shape -- about 20 000 tokens in 200 windows of at most 218 tokens, 12 heads of 64 -- in fp16 and bf16, against
  (a) torch.nn.functional.scaled_dot_product_attention forward + backward over the same windows padded to the longest, the padded keys
      masked out: the composition a user of this package would otherwise write (the padding itself is not timed),
  (b) this library's dense `attention` forward + backward on an equal-length batch of the same token count (200 sequences of T / 200
      tokens): what the same kernels do without the ragged decode, idle tail workgroups and uneven sequences.
GPU only.  All sides alternate in one process: ROUNDS windows of GVF_STEPS / ROUNDS calls per side (default 2000 calls), device events around
each window (200 calls of 0.2 - 1 ms), after warm-up calls of every side.  These are times per CALL as a training step sees it: five launches
and their Python per forward + backward; GVF_SIDES=ragged (or sdpa, dense) with few GVF_STEPS under rocprofv3 --kernel-trace --stats gives
the kernel times of one side alone.  Prints ms per call (median, fastest and slowest window), the two ratios and the score-matrix
elements sum_s Lq_s Lk_s each side covers; one JSON line per type at the end (GVF_BENCH_OUT: also written to that file)."""
import json
import os
import statistics
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from gvfdiffusion_amd.ops import attention_grad as AG  # noqa: E402

dev = torch.device("cuda:0")
N_STEPS = int(os.environ.get("GVF_STEPS", 2000))
SIDES = [s for s in os.environ.get("GVF_SIDES", "ragged,sdpa,dense").split(",") if s]      # a subset: kernel times of one side under a profiler
ROUNDS = 10
N_WIN, MAX_L, H, C = 200, 218, 12, 64


def window_lengths():
    """200 window populations between 1 and 218 voxels, seeded; about 20 000 tokens in all."""
    g = torch.Generator().manual_seed(218)
    return [int(n) for n in torch.randint(1, MAX_L + 1, (N_WIN,), generator=g)]


def timed(fns, n):
    """Per function, the ms per call of each of ROUNDS alternating windows of n / ROUNDS calls, after three warm-up calls of each."""
    for f in fns:
        for _ in range(3):
            f()
    torch.cuda.synchronize()
    per = max(1, n // ROUNDS)
    ms = [[] for _ in fns]
    for _ in range(ROUNDS):
        for i, f in enumerate(fns):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(per):
                f()
            e1.record()
            torch.cuda.synchronize()
            ms[i].append(e0.elapsed_time(e1) / per)
    return ms


def main():
    lens = window_lengths()
    T, longest = sum(lens), max(lens)
    L_eq = round(T / N_WIN)
    work = sum(n * n for n in lens)
    print(f"ragged attention forward + backward: {N_WIN} windows, {T} tokens, longest {longest}, H {H}, d {C}; score elements per head: ragged "
          f"{work}, padded {N_WIN * longest * longest} ({N_WIN * longest * longest / work:.2f}x), equal-length {N_WIN} x {L_eq}: "
          f"{N_WIN * L_eq * L_eq} ({N_WIN * L_eq * L_eq / work:.2f}x); {N_STEPS} timed calls per side in {ROUNDS} alternating windows")
    lines = []
    for dt in (torch.float16, torch.bfloat16):
        g = torch.Generator().manual_seed(T)
        q, k, v, do = (torch.randn((T, H, C), generator=g).to(dev, dt) for _ in range(4))
        q, k, v = (t.requires_grad_(True) for t in (q, k, v))
        cu = torch.tensor([0] + list(torch.tensor(lens).cumsum(0)), dtype=torch.int32, device=dev)
        scale = C ** -0.5

        def ragged():
            out = AG.attention_varlen(q, k, v, cu, cu, longest, longest, scale)
            torch.autograd.grad(out, (q, k, v), do)

        # (a) the windows padded to the longest, [N_WIN, H, longest, C], padded keys masked
        pad = [torch.zeros((N_WIN, longest, H, C), dtype=dt, device=dev) for _ in range(4)]
        mask = torch.zeros((N_WIN, 1, 1, longest), dtype=torch.bool, device=dev)
        at = 0
        for i, n in enumerate(lens):
            for p, t in zip(pad, (q, k, v, do)):
                p[i, :n] = t.detach()[at:at + n]
            mask[i, ..., :n] = True
            at += n
        qp, kp, vp, dop = (p.permute(0, 2, 1, 3).contiguous() for p in pad)
        qp, kp, vp = (t.requires_grad_(True) for t in (qp, kp, vp))

        def padded_sdpa():
            out = F.scaled_dot_product_attention(qp, kp, vp, attn_mask=mask, scale=scale)
            torch.autograd.grad(out, (qp, kp, vp), dop)

        # (b) the dense operator on N_WIN sequences of L_eq tokens
        qe, ke, ve, doe = (torch.randn((N_WIN, L_eq, H, C), generator=g).to(dev, dt) for _ in range(4))
        qe, ke, ve = (t.requires_grad_(True) for t in (qe, ke, ve))

        def dense_equal():
            out = AG.attention(qe, ke, ve, scale)
            torch.autograd.grad(out, (qe, ke, ve), doe)

        if len(SIDES) < 3:
            timed([f for s, f in (("ragged", ragged), ("sdpa", padded_sdpa), ("dense", dense_equal)) if s in SIDES], N_STEPS)
            continue
        ms = timed([ragged, padded_sdpa, dense_equal], N_STEPS)
        med = [statistics.median(m) for m in ms]
        name = str(dt)[6:]
        for what, m, md in zip(("ragged (this library)", "(a) torch SDPA, padded + masked", "(b) dense, equal lengths"), ms, med):
            print(f"  {name:8s} {what:34s} {md:.3f} ms per call (windows {min(m):.3f} .. {max(m):.3f})", flush=True)
        print(f"  {name:8s} (a) / ragged {med[1] / med[0]:.2f}x;  ragged / (b) {med[0] / med[2]:.2f}x in time, "
              f"{(med[0] / work) / (med[2] / (N_WIN * L_eq * L_eq)):.2f}x per score element", flush=True)
        lines.append({"bench": "attn_varlen_fwd_bwd", "dtype": name, "windows": N_WIN, "tokens": T, "longest": longest, "heads": H, "head_dim": C,
                      "equal_length": L_eq, "score_elements": {"ragged": work, "padded": N_WIN * longest * longest, "equal": N_WIN * L_eq * L_eq},
                      "ms": {"ragged": med[0], "sdpa_padded": med[1], "dense_equal": med[2]},
                      "ms_windows": {"ragged": [min(ms[0]), max(ms[0])], "sdpa_padded": [min(ms[1]), max(ms[1])], "dense_equal": [min(ms[2]), max(ms[2])]},
                      "sdpa_padded_over_ragged": med[1] / med[0], "ragged_over_dense_equal": med[0] / med[2], "steps": N_STEPS, "rounds": ROUNDS})
    text = "\n".join(json.dumps(l) for l in lines)
    print(text)
    if os.environ.get("GVF_BENCH_OUT"):
        with open(os.environ["GVF_BENCH_OUT"], "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
