"""Forward + backward of 24 views at the BASELINE shape (262 144 Gaussians, 800 x 800, SH degree 2), as the VAE training step renders them
(train_vae.py:313-352: render(static_gs, cam, delta_pc=pred_delta_b) per view, image loss back-propagated into the deltas and the static
Gaussians); GPU only.  (a) 24 calls of the single-frame path (GaussianRenderer.render: torch activations -> _RasterizeFn), (b) one
render_frames + backward with 24 delta slices, (c) the same with 6 slices x 4 cameras (shared activation engages).  Prints ms per step."""
import os, sys, torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from gvfdiffusion_amd import synthetic
from gvfdiffusion_amd.renderers import GaussianRenderer

dev = torch.device("cuda:0")
P, S, deg, V = int(os.environ.get("GVF_P", 262144)), int(os.environ.get("GVF_S", 800)), 2, 24
MODE = os.environ.get("GVF_BENCH_MODE", "abc")           # which of (a) (b) (c) to time (the kernel trace takes one)
attrs = synthetic.random_gaussians(P, sh_degree=deg, seed=0, scale_lo=0.002, scale_hi=0.01)
gm = synthetic.gaussian_model_from(attrs, deg, dev)
for k in ("_xyz", "_features_dc", "_scaling", "_rotation", "_opacity"):
    setattr(gm, k, getattr(gm, k).detach().contiguous().requires_grad_(True))
rend = GaussianRenderer({"resolution": S, "near": synthetic.NEAR, "far": synthetic.FAR, "ssaa": 1, "bg_color": (1, 1, 1)})
rend.pipe.use_mip_gaussian = True
rend.pipe.kernel_size = synthetic.KERNEL_2D
K = synthetic.intrinsics().to(dev)
ext = torch.stack([synthetic.orbit_w2c(15.0 * v, 10.0) for v in range(V)]).to(dev)
delta = (synthetic.random_deltas(V, P, seed=1, std=0.01)).to(dev).requires_grad_(True)
w = torch.randn((V, 3, S, S), device=dev)

def per_frame(_):
    for v in range(V):
        (rend.render(gm, ext[v], K, delta_pc=delta[v]).rgb * w[v]).sum().backward()

def batched(index):
    def run(_):
        (rend.render_frames(gm, ext, K, delta_pc=delta, delta_index=index).rgb * w).sum().backward()
    return run

def timed(fn, n):
    fn(0)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for i in range(n): fn(i)
    e1.record(); torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n

n = int(os.environ.get("GVF_STEPS", 5))
res = {}
if "a" in MODE: res["a"] = timed(per_frame, n)
if "b" in MODE: res["b"] = timed(batched(list(range(V))), n)
if "c" in MODE: res["c"] = timed(batched([v // 4 for v in range(V)]), n)
names = {"a": "(a) 24 single-frame calls", "b": "(b) render_frames, 24 slices", "c": "(c) render_frames, 6 slices x 4 cameras"}
print(f"P={P} {S}x{S} SH{deg}, {V} views, forward + backward per step ({n} steps):")
for k, t in res.items():
    extra = f"   {res['a'] / t:.2f}x over (a)" if "a" in res and k != "a" else ""
    print(f"  {names[k]:42s} {t:8.2f} ms  ({t / V:.3f} ms/view, {1000.0 * V / t:.0f} views/s){extra}")
