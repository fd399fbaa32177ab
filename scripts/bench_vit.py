"""The DINOv2 image encoder (model/dinov2.py on csrc/vit.hip, gemm.hip, attn.hip) against torch's composition.  GPU only.

ViT-L/14 with 4 registers at 518 x 518 (1374 tokens per image, 24 blocks of width 1024), random weights, B = 1 and B = 24 (the DiT's 24
condition frames), fp16 and bf16.
  1. pixels -> x_prenorm: the HIP route against F.conv2d + F.layer_norm + F.linear + F.scaled_dot_product_attention on fp32 parameters under
     torch.autocast (the composition a user of the hub model runs); ms per image.
  2. per kernel at the encoder's shapes, time and TFLOP/s: the patch embedding (against unfold -> gvf_gemm and against F.conv2d in the operand
     type), the four projections of a block (qkv and fc1 with the LayerNorm folded in, proj and fc2 with LayerScale, the residual update and
     the row statistics), the attention, and the read-out.
The sides alternate in one process, GVF_ROUNDS times, device events around GVF_STEPS calls; min .. max over the rounds.
GVF_BENCH_BATCHES (default "1,24") and GVF_BENCH_BLOCKS (default 24) shrink the run."""
import os
import sys
import time

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "scripts"))
from gvfdiffusion_amd.model.dinov2 import DinoVisionTransformer  # noqa: E402
from gvfdiffusion_amd.ops import dit_ops, vit as vit_ops  # noqa: E402
from bench_slat_flow import alternate, report, N_STEPS, ROUNDS  # noqa: E402
import vit_ref as V  # noqa: E402

dev = torch.device("cuda:0")
BATCHES = [int(b) for b in os.environ.get("GVF_BENCH_BATCHES", "1,24").split(",")]
BLOCKS = int(os.environ.get("GVF_BENCH_BLOCKS", 24))
D, HEADS, GRID, REG = 1024, 16, 37, 4
L = 1 + REG + GRID * GRID


def build(dt):
    sd = {k: v.to(dev) for k, v in V.random_state_dict(D, BLOCKS, GRID, REG, seed=0).items()}
    m = DinoVisionTransformer(img_size=GRID * 14, embed_dim=D, depth=BLOCKS, num_heads=HEADS, num_register_tokens=REG, dtype=dt)
    m.load_state_dict(sd, strict=True)
    return m.to(dev), sd


def torch_forward(sd, img, dt):
    """tests/vit_ref.py::forward_autocast on the device."""
    mean = torch.tensor(V.IMAGENET_MEAN, device=dev).view(1, 3, 1, 1)
    std = torch.tensor(V.IMAGENET_STD, device=dev).view(1, 3, 1, 1)
    with torch.no_grad(), torch.autocast("cuda", dtype=dt):
        conv = F.conv2d((img - mean) / std, sd["patch_embed.proj.weight"], sd["patch_embed.proj.bias"], stride=14).flatten(2).transpose(1, 2)
        x = V.assemble(sd, conv.float(), REG, torch.float32)
        B = x.shape[0]
        for i in range(BLOCKS):
            g = lambda n: sd[f"blocks.{i}.{n}"]
            h = F.layer_norm(x, (D,), g("norm1.weight"), g("norm1.bias"), 1e-6)
            q, k, v = F.linear(h, g("attn.qkv.weight"), g("attn.qkv.bias")).view(B, L, 3, HEADS, 64).permute(2, 0, 3, 1, 4)
            a = F.scaled_dot_product_attention(q, k, v).permute(0, 2, 1, 3).reshape(B, L, D)
            x = x + g("ls1.gamma") * F.linear(a, g("attn.proj.weight"), g("attn.proj.bias")).float()
            h = F.layer_norm(x, (D,), g("norm2.weight"), g("norm2.bias"), 1e-6)
            x = x + g("ls2.gamma") * F.linear(F.gelu(F.linear(h, g("mlp.fc1.weight"), g("mlp.fc1.bias"))), g("mlp.fc2.weight"), g("mlp.fc2.bias")).float()
    return x


def model_section(dt, m, sd, B):
    img = torch.rand((B, 3, GRID * 14, GRID * 14), generator=torch.Generator(device=dev).manual_seed(B), device=dev)
    a, b = m.forward_stream(img), torch_forward(sd, img, dt)
    flops = B * (2 * L * 588 * D * (L - 1 - REG) / L + BLOCKS * (2 * L * D * 12 * D + 4 * L * L * D))
    print(f"pixels -> x_prenorm, B = {B}, {dt}: hip vs torch composition rel-L2 {V.rel_l2(a, b):.2e}")
    res = alternate({"torch": lambda: torch_forward(sd, img, dt), "hip": lambda: m.forward_stream(img)}, n=max(1, N_STEPS // (2 if B > 1 else 1)))
    report(f"ViT-L/14-reg forward, {BLOCKS} blocks, B = {B} ({flops / 1e12:.2f} TFLOP)", res, flops=flops)
    print(f"    per image: torch {min(res['torch']) / B:.3f} ms, hip {min(res['hip']) / B:.3f} ms")


def kernel_section(dt, m, sd, B):
    g = torch.Generator(device=dev).manual_seed(100 + B)
    img = torch.rand((B, 3, GRID * 14, GRID * 14), generator=g, device=dev)
    im = m.weight_images()
    M, n = B * L, GRID * GRID
    # ---- patch embedding
    w16 = sd["patch_embed.proj.weight"].to(dt)
    wflat = torch.zeros((D, vit_ops.PATCH_KPAD), dtype=dt, device=dev)
    wflat[:, :588] = w16.reshape(D, 588)
    mean = torch.tensor(V.IMAGENET_MEAN, device=dev).view(1, 3, 1, 1)
    std = torch.tensor(V.IMAGENET_STD, device=dev).view(1, 3, 1, 1)
    rows = torch.zeros((B * n, vit_ops.PATCH_KPAD), dtype=dt, device=dev)
    conv_out = torch.empty((B * n, D), dtype=torch.float32, device=dev)

    def unfold_gemm():
        rows[:, :588] = V.patch_rows(((img - mean) / std).to(dt))
        return dit_ops.gemm(rows, wflat, im["patch_b"], conv_out, dit_ops.EPI_STORE_F32)
    b16 = sd["patch_embed.proj.bias"].to(dt)
    flops = 2 * B * n * 588 * D
    report(f"patch embedding B = {B} ({flops / 1e9:.1f} GFLOP; hip = z-score + gather + GEMM + token assembly + statistics; the others stop at the convolution)",
           alternate({"torch": lambda: F.conv2d(((img - mean) / std).to(dt), w16, b16, stride=14),
                      "unfold+gemm": unfold_gemm,
                      "hip": lambda: vit_ops.patch_embed(img, im["patch_w"], im["patch_b"], im["cls"], im["reg"], im["pos"])}), flops=flops)
    # ---- one block's launches at M = B * 1374
    x, stats = vit_ops.patch_embed(img, im["patch_w"], im["patch_b"], im["cls"], im["reg"], im["pos"])
    x = x.view(M, D)
    b = im["blocks"][0]
    n_part = dit_ops.gemm_stats_parts(D)
    qkv = torch.empty((M, 3 * D), dtype=dt, device=dev)
    ab = torch.empty((M, D), dtype=dt, device=dev)
    hid = torch.empty((M, 4 * D), dtype=dt, device=dev)
    s_qkv, s_o = (L * 3 * D, 0, 3 * D), (L * D, 0, D)
    fp = lambda p: sd[f"blocks.0.{p}"]
    h16 = torch.randn((M, D), generator=g, device=dev).to(dt)
    hid.copy_(torch.randn((M, 4 * D), generator=g, device=dev).to(dt))
    ab.copy_(h16)
    q4 = qkv.view(B, L, 3, HEADS, 64)

    def t_ln_linear(nw, nb, w, bb, act=None):
        h = F.layer_norm(x, (D,), fp(nw), fp(nb), 1e-6).to(dt)
        y = F.linear(h, w, bb)
        return y if act is None else act(y)

    def t_resid(a16, w, bb, gamma):
        return x + fp(gamma) * F.linear(a16, w, bb).float()
    W = {k: fp(k + ".weight").to(dt) for k in ("attn.qkv", "attn.proj", "mlp.fc1", "mlp.fc2")}
    Bs = {k: fp(k + ".bias").to(dt) for k in W}
    items = [
        ("qkv = norm1 -> 1024 x 3072 (LayerNorm folded in)", 2 * M * D * 3 * D,
         lambda: t_ln_linear("norm1.weight", "norm1.bias", W["attn.qkv"], Bs["attn.qkv"]),
         lambda: dit_ops.gemm_ln_bf16(x, stats, n_part, b["qkv"][0], b["qkv"][1], qkv, dit_ops.EPI_STORE_16, eps=1e-6, ln_w=b["n1"][0], ln_b=b["n1"][1])),
        ("attention, 16 heads of 64, 1374 x 1374", 4 * B * L * L * D,
         lambda: F.scaled_dot_product_attention(q4[:, :, 0].transpose(1, 2), q4[:, :, 1].transpose(1, 2), q4[:, :, 2].transpose(1, 2)),
         lambda: dit_ops.attention(qkv, qkv[:, D:], qkv[:, 2 * D:], ab, B, 1, L, L, HEADS, s_qkv, s_qkv, s_qkv, s_o, head_dim=64)),
        ("proj 1024 x 1024 + LayerScale + residual (+ statistics)", 2 * M * D * D,
         lambda: t_resid(h16, W["attn.proj"], Bs["attn.proj"], "ls1.gamma"),
         lambda: dit_ops.gemm_resid_stats(h16, b["proj"][0], b["proj"][1], x, stats, gate=b["ls1"], gate_ld=D, rows_per_group=M)),
        ("fc1 = norm2 -> 1024 x 4096 + erf GELU (LayerNorm folded in)", 2 * M * D * 4 * D,
         lambda: t_ln_linear("norm2.weight", "norm2.bias", W["mlp.fc1"], Bs["mlp.fc1"], F.gelu),
         lambda: dit_ops.gemm_ln_bf16(x, stats, n_part, b["fc1"][0], b["fc1"][1], hid, dit_ops.EPI_GELU_ERF_16, eps=1e-6, ln_w=b["n2"][0], ln_b=b["n2"][1])),
        ("fc2 4096 x 1024 + LayerScale + residual (+ statistics)", 2 * M * D * 4 * D,
         lambda: t_resid(hid, W["mlp.fc2"], Bs["mlp.fc2"], "ls2.gamma"),
         lambda: dit_ops.gemm_resid_stats(hid, b["fc2"][0], b["fc2"][1], x, stats, gate=b["ls2"], gate_ld=D, rows_per_group=M)),
    ]
    # the residual launches update x in place: start every timed side from a small stream so that 10^2 repeats stay finite
    x.mul_(1e-3)
    for title, flops, tor, hip in items:
        report(f"{title}, M = {M}", alternate({"torch": tor, "hip": hip}), flops=flops)
    x3 = x.view(B, L, D)
    report(f"read-out B = {B}: TRELLIS LayerNorm, all tokens, fp32 (torch: F.layer_norm)",
           alternate({"torch": lambda: F.layer_norm(x3, (D,)), "hip": lambda: vit_ops.tokens_out(x3, REG, vit_ops.OUT_LN)}))
    report(f"read-out B = {B}: patches then cls, fp16 (torch: cat + half)",
           alternate({"torch": lambda: torch.cat([x3[:, REG + 1:], x3[:, :1]], 1).half(),
                      "hip": lambda: vit_ops.tokens_out(x3, REG, vit_ops.OUT_COPY, vit_ops.ORDER_PATCHES_CLS, torch.float16)}))


if __name__ == "__main__":
    t0 = time.time()
    print(f"{torch.cuda.get_device_name(0)}; {ROUNDS} rounds of {N_STEPS} calls; ViT-L/14-reg at 518 x 518, {L} tokens per image")
    for dt in (torch.float16, torch.bfloat16):
        m, sd = build(dt)
        for B in BATCHES:
            model_section(dt, m, sd, B)
        if dt == torch.float16:
            for B in BATCHES:
                kernel_section(dt, m, sd, B)
        del m, sd
    print(f"({time.time() - t0:.0f} s)")
