"""CLIP's ViT-B/32 image tower (model/clip.py on csrc/clip.hip, gemm.hip, attn.hip) and the alignment score that uses it.  GPU only.

  1. Encoder, fp16, random weights, 224 x 224, B = 1 and B = 60 (one render chunk of the alignment): uint8 pixels -> features on the HIP route
     against the torch fp16 composition of the same model (fp16 parameters and activations, as the reference's clip.load on a GPU: F.conv2d,
     F.layer_norm, F.scaled_dot_product_attention, F.linear) fed the normalised fp16 pixels; then per launch group -- front (patch
     convolution + token assembly + ln_pre), the 12 blocks, head (ln_post + proj + unit vector + cosine) -- and the patch GEMM alone against
     F.conv2d with its achieved FLOP/s (2 * 49 B * 768 * 3072).
  2. align_gaussian_to_canonical over the 360 azimuths of the in-the-wild path (512 x 512 renders of a 6000-Gaussian object, chunks of 60):
     clip_model= (batched), clip_score= (the per-view callback around the same model) and no CLIP term.
The sides alternate in one process, GVF_ROUNDS times, device events around GVF_STEPS calls; min .. max over the rounds (part 2: wall clock
around whole calls, which end in a host read)."""
import os
import sys
import time
from types import SimpleNamespace

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "scripts"))
from gvfdiffusion_amd import synthetic  # noqa: E402
from gvfdiffusion_amd.model.clip import CLIPVisionTransformer  # noqa: E402
from gvfdiffusion_amd.ops import clip as clip_ops  # noqa: E402
from bench_slat_flow import alternate, report, N_STEPS, ROUNDS  # noqa: E402
import clip_ref as C  # noqa: E402

dev = torch.device("cuda:0")
D, DEPTH, GRID, E, HEADS = 768, 12, 7, 512, 12
L = 1 + GRID * GRID
DT = torch.float16


def build():
    sd = C.random_state_dict(D, DEPTH, GRID, E, seed=0)
    m = CLIPVisionTransformer(dtype=DT)
    m.load_state_dict(sd, strict=True)
    return m.to(dev), {k: v.to(dev).half() for k, v in sd.items()}


def t_front(p, pix):
    conv = F.conv2d(pix, p["conv1.weight"], None, stride=32).flatten(2).transpose(1, 2)
    x = torch.cat([p["class_embedding"].expand(conv.shape[0], 1, D), conv], 1) + p["positional_embedding"]
    return F.layer_norm(x, (D,), p["ln_pre.weight"], p["ln_pre.bias"], C.EPS)


def t_blocks(p, x):
    B = x.shape[0]
    for i in range(DEPTH):
        g = lambda n: p[f"transformer.resblocks.{i}.{n}"]
        h = F.layer_norm(x, (D,), g("ln_1.weight"), g("ln_1.bias"), C.EPS)
        q, k, v = F.linear(h, g("attn.in_proj_weight"), g("attn.in_proj_bias")).view(B, L, 3, HEADS, 64).permute(2, 0, 3, 1, 4)
        a = F.scaled_dot_product_attention(q, k, v).permute(0, 2, 1, 3).reshape(B, L, D)
        x = x + F.linear(a, g("attn.out_proj.weight"), g("attn.out_proj.bias"))
        u = F.linear(F.layer_norm(x, (D,), g("ln_2.weight"), g("ln_2.bias"), C.EPS), g("mlp.c_fc.weight"), g("mlp.c_fc.bias"))
        x = x + F.linear(u * torch.sigmoid(1.702 * u), g("mlp.c_proj.weight"), g("mlp.c_proj.bias"))
    return x


def t_head(p, x, gref):
    f = F.layer_norm(x[:, 0], (D,), p["ln_post.weight"], p["ln_post.bias"], C.EPS) @ p["proj"]
    f = f / f.norm(dim=-1, keepdim=True)
    return f @ gref


def encoder_section(m, p, B):
    img = torch.randint(0, 256, (B, 3, 224, 224), generator=torch.Generator().manual_seed(B), dtype=torch.uint8).to(dev)
    pix = C.normalise_u8(img.cpu()).half().to(dev)
    gref = torch.randn(E, generator=torch.Generator().manual_seed(1))
    gref = (gref / gref.norm()).to(dev)
    g16 = gref.half()
    im = m.weight_images()
    with torch.no_grad():
        a = m.encode(img, gref)[2]
        b = t_head(p, t_blocks(p, t_front(p, pix)), g16)
        print(f"uint8 pixels -> similarity, B = {B}: max |hip - torch fp16| = {float((a - b.float()).abs().max()):.2e}")
        n = max(1, N_STEPS // (2 if B > 1 else 1))
        flops = B * (2 * (L - 1) * 3072 * D + DEPTH * (2 * L * D * 12 * D + 4 * L * L * D) + 2 * D * E)
        report(f"ViT-B/32 pixels -> similarity, B = {B} ({flops / 1e9:.1f} GFLOP)",
               alternate({"torch": lambda: t_head(p, t_blocks(p, t_front(p, pix)), g16), "hip": lambda: m.encode(img, gref)}, n=n), flops=flops)
        xs = t_front(p, pix)
        x_hip = m.forward_stream(img)
        report(f"  front (patch convolution + tokens + ln_pre), B = {B}",
               alternate({"torch": lambda: t_front(p, pix),
                          "hip": lambda: clip_ops.ln_rows(clip_ops.patch_embed(img, im["patch_w"], im["cls"], im["pos"], im["lut"]), *im["ln_pre"])}, n=n))
        full = alternate({"torch": lambda: t_blocks(p, xs), "hip": lambda: m.forward_stream(img)}, n=n)
        report(f"  blocks, B = {B} (hip: front + blocks, the stream is updated in place)", full)
        report(f"  head (ln_post + proj + unit vector + cosine), B = {B}",
               alternate({"torch": lambda: t_head(p, xs, g16),
                          "hip": lambda: clip_ops.head(x_hip, im["ln_post"][0], im["ln_post"][1], im["proj"], gref)}, n=n))
        gf = 2 * (L - 1) * B * D * 3072
        report(f"  patch GEMM alone, B = {B} ({gf / 1e9:.2f} GFLOP; hip = table lookup + gather + GEMM + token assembly)",
               alternate({"torch": lambda: F.conv2d(pix, p["conv1.weight"], None, stride=32),
                          "hip": lambda: clip_ops.patch_embed(img, im["patch_w"], im["cls"], im["pos"], im["lut"])}, n=n), flops=gf)


def align_section(m):
    from gvfdiffusion_amd.attrdict import edict
    from gvfdiffusion_amd.renderers import GaussianRenderer
    from gvfdiffusion_amd.utils.inference_utils import align_gaussian_to_canonical, azimuth_cameras
    P = 6000
    g = torch.Generator().manual_seed(5)
    attrs = synthetic.random_gaussians(P, sh_degree=0, seed=13, scale_lo=0.006, scale_hi=0.015)
    xyz = (torch.rand(P, 3, generator=g) - 0.5) * torch.tensor([0.5, 0.12, 0.35])
    xyz[: P // 3] = (torch.rand(P // 3, 3, generator=g) - 0.5) * torch.tensor([0.1, 0.3, 0.1]) + torch.tensor([0.2, 0.2, 0.1])
    attrs["means3D"] = xyz
    attrs["opacities"] = attrs["opacities"].clamp(min=0.6)
    rend = GaussianRenderer({"resolution": 512, "near": synthetic.NEAR, "far": synthetic.FAR, "bg_color": (1, 1, 1)})
    rend.pipe.kernel_size = synthetic.KERNEL_2D
    K = synthetic.intrinsics().to(dev)
    vae = SimpleNamespace(renderers=edict({"MipGS": rend}))
    with torch.no_grad():
        canon = rend.render_frames(synthetic.gaussian_model_from(attrs, 0, dev), azimuth_cameras([37]).to(dev), K, want_alpha_depth=True)
    rgb, alpha = canon.rgb[0].clamp(0, 1), canon.alpha[0]
    forms = {"no CLIP term": {}, "clip_score= (per view)": dict(clip_score=lambda i, c: m.similarity(i[None], c)[0]), "clip_model= (batched)": dict(clip_model=m)}
    times = {k: [] for k in forms}
    stdout = sys.stdout
    for r in range(ROUNDS + 1):                          # round 0 warms up
        for k, kw in forms.items():
            gm = synthetic.gaussian_model_from(attrs, 0, dev)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            sys.stdout = open(os.devnull, "w")
            try:
                align_gaussian_to_canonical(gm, rgb, alpha, K, vae, id=0, device=dev, in_the_wild=True, **kw)
            finally:
                sys.stdout.close()
                sys.stdout = stdout
            torch.cuda.synchronize()
            if r:
                times[k].append((time.perf_counter() - t0) * 1e3)
    print("align_gaussian_to_canonical, 360 azimuths, 512 x 512, 6000 Gaussians, chunks of 60 (wall clock per call)")
    for k, v in times.items():
        print(f"    {k:<24s} {min(v):.1f} .. {max(v):.1f} ms", flush=True)


if __name__ == "__main__":
    t0 = time.time()
    print(f"{torch.cuda.get_device_name(0)}; {ROUNDS} rounds of {N_STEPS} calls; CLIP ViT-B/32 at 224 x 224, {L} tokens per image, fp16")
    m, p = build()
    for B in (1, 60):
        encoder_section(m, p, B)
    if os.environ.get("GVF_BENCH_ALIGN", "1") != "0":
        align_section(m)
    print(f"({time.time() - t0:.0f} s)")
