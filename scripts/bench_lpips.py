"""LPIPS (VGG16) term of the render loss (ops/lpips.py) against the same loss composed in torch -- F.conv2d on channels_last tensors under
fp16 autocast, max_pool2d, the tap formula, autograd backward: what a user would otherwise run -- forward + backward at the step's
own shape 24 x 3 x 800^2 (GVF_N, GVF_S), both in groups of GVF_CHUNK images (default 8), alternated in one process.  Then every
convolution layer alone: gvf_conv3x3 forward and input gradient against F.conv2d forward on the same shape, with the achieved TFLOP/s of
the 2 * 9 * Cin * Cout * pixels FLOP the layer needs.  GPU only (there is no fallback); prints text, one line per figure."""
import os
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from gvfdiffusion_amd.ops import lpips as LP  # noqa: E402

assert torch.cuda.is_available(), "bench_lpips.py needs an MI355X"
dev = torch.device("cuda:0")
N, S = int(os.environ.get("GVF_N", 24)), int(os.environ.get("GVF_S", 800))
CHUNK = int(os.environ.get("GVF_CHUNK", 8))
ROUNDS = int(os.environ.get("GVF_ROUNDS", 3))
DT = torch.float16


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


def torch_trunk(x, convs, mean, std):
    a = ((x - mean) / std).contiguous(memory_format=torch.channels_last)
    taps = []
    for k, (w, b) in enumerate(convs):
        a = F.relu(F.conv2d(a, w, b, padding=1))
        if k in LP.TAPS:
            taps.append(a)
        if k in LP.POOL_AFTER:
            a = F.max_pool2d(a, 2, 2)
    return taps


def torch_lpips(x, y, convs, lins, mean, std):
    total = 0.0
    for i in range(0, x.shape[0], CHUNK):
        with torch.autocast("cuda", dtype=DT):
            tx = torch_trunk(x[i:i + CHUNK], convs, mean, std)
            with torch.no_grad():
                ty = torch_trunk(y[i:i + CHUNK], convs, mean, std)
        part = 0.0
        for a, b, l in zip(tx, ty, lins):
            a, b = a.float(), b.float()
            u = a / (torch.sqrt((a * a).sum(1, keepdim=True)) + 1e-10)
            v = b / (torch.sqrt((b * b).sum(1, keepdim=True)) + 1e-10)
            part = part + (((u - v) ** 2) * l).sum(1).mean((1, 2)).sum()
        (part / x.shape[0]).backward()          # per group: its activations are freed before the next group runs
        total = total + part.detach()
    return total / x.shape[0]


m = LP.LPIPS(dtype=DT, chunk=CHUNK).to(dev)
convs = [(m.net.layers[str(i)].weight.to(memory_format=torch.channels_last), m.net.layers[str(i)].bias) for i, _, _ in LP.VGG_CONVS]
lins = [l[1].weight for l in m.lin]
g = torch.Generator().manual_seed(0)
y = (torch.rand((N, 3, S, S), generator=g) * 2 - 1).to(dev)
x = (y + 0.1 * torch.randn((N, 3, S, S), generator=g).to(dev)).clamp(-1, 1).requires_grad_(True)


def ours():
    x.grad = None
    m(x, y).backward()


def composed():
    x.grad = None
    torch_lpips(x, y, convs, lins, m.net.mean, m.net.std)


print(f"LPIPS forward + backward, {N} x 3 x {S}^2, fp16 forward, groups of {CHUNK} images", flush=True)
l_ours = float(m(x, y).detach())
l_torch = float(torch_lpips(x, y, convs, lins, m.net.mean, m.net.std))
g_torch = x.grad.clone()
ours()
# an unscaled fp16 autocast backward can underflow: the norms and the non-finite count say what the comparison is worth
n_hip, n_torch, bad = float(x.grad.double().norm()), float(g_torch.double().norm()), int((~torch.isfinite(g_torch)).sum())
rel = float((x.grad - g_torch).double().norm()) / n_torch if n_torch > 0 and bad == 0 else float("nan")
print(f"same inputs: loss HIP {l_ours:.6e}, torch fp16 autocast {l_torch:.6e}; gradient norm HIP {n_hip:.4e}, torch {n_torch:.4e} "
      f"({bad} non-finite elements, {int((g_torch == 0).sum())} of {g_torch.numel()} exactly zero), relative L2 difference {rel:.2e}", flush=True)
t_ours, t_torch = [], []
for r in range(ROUNDS):
    t_ours.append(timed(ours, 2))
    t_torch.append(timed(composed, 2))
    print(f"round {r}: HIP {t_ours[-1]:.1f} ms, torch-composed {t_torch[-1]:.1f} ms", flush=True)
to, tt = sorted(t_ours)[len(t_ours) // 2], sorted(t_torch)[len(t_torch) // 2]
print(f"median: HIP {to:.1f} ms, torch-composed {tt:.1f} ms, torch / HIP = {tt / to:.2f}", flush=True)
print(f"peak memory allocated: {torch.cuda.max_memory_allocated() / 2 ** 30:.1f} GiB", flush=True)
del x, y, g_torch
torch.cuda.empty_cache()

# every convolution layer alone, at the resolution it runs at, CHUNK images
pk = m.packed()
side = S
print(f"per layer, {CHUNK} images: gvf_conv3x3 forward (fp16) | gvf_conv3x3 input gradient (bf16) | F.conv2d forward (fp16, channels_last)", flush=True)
for k, (_, cin, cout) in enumerate(LP.VGG_CONVS):
    if k:
        flop = 2.0 * 9 * cin * cout * CHUNK * side * side
        a = torch.rand((CHUNK, side, side, cin), device=dev).to(DT)
        z = torch.rand((CHUNK, side, side, cout), device=dev).to(torch.bfloat16)
        tf = timed(lambda: LP.conv3x3(a, pk.fwd[k], cout, bias=pk.bias[k], relu=True), 20)
        tb = timed(lambda: LP.conv3x3(z, pk.dgrad[k], cin, mask_src=a), 20)
        at = a.permute(0, 3, 1, 2)                # NCHW view of NHWC memory = channels_last
        w16, b16 = convs[k][0].to(DT), convs[k][1].to(DT)
        tc = timed(lambda: F.conv2d(at, w16, b16, padding=1), 20)
        print(f"conv {k + 1:2d} {cin:3d}->{cout:3d} @ {side}^2: {tf:7.2f} ms {flop / tf / 1e9:6.1f} TFLOP/s | {tb:7.2f} ms {flop / tb / 1e9:6.1f} TFLOP/s"
              f" | {tc:7.2f} ms {flop / tc / 1e9:6.1f} TFLOP/s", flush=True)
        del a, z, at
    if k in LP.POOL_AFTER:
        side //= 2
