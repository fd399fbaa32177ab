"""Plain torch restatement of the DINOv2 ViT the image encoder implements (gvfdiffusion_amd/model/dinov2.py, csrc/vit.hip), the key map to
the Hugging Face implementation it is checked against (tests/test_vit_ref.py), and the error bounds of the new kernels.

forward() is the whole model in one dtype (float64 for the reference): z-score, 14 x 14 stride-14 convolution, token assembly
[cls + pos[0] | registers (no position) | patches + pos[1:]], the blocks x += ls1 proj(attn(norm1 x)); x += ls2 fc2(gelu_erf(fc1(norm2 x)))
(LayerNorm eps 1e-6, heads of 64, softmax scale 1/8), and the three read-outs the callers consume: x_prenorm, x_norm = norm(x_prenorm)
(eps 1e-6, affine) and the TRELLIS condition F.layer_norm(x_prenorm) (eps 1e-5, no affine).  `mutant` switches ONE of the model's decisions
to a plausible wrong one; the comparison of tests/test_vit_ref.py must reject each.

Everything here runs on torch CPU tensors."""
import math

import torch
import torch.nn.functional as F

import gemm_ref

IMAGENET_MEAN, IMAGENET_STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
PATCH, PATCH_K, PATCH_KPAD = 14, 588, 608
U32 = gemm_ref.U32
EPI_GELU_ERF_16 = 5
MUTANTS = ("reg_pos", "cls_last", "gelu_tanh", "no_layerscale", "eps_1e-5", "zscore_after_rounding")


# ---- weights ----------------------------------------------------------------------------------------------------------------------------
def state_dict_keys(depth: int, R: int):
    """The hub checkpoint's parameter names (from memory of the public checkpoint: unpinned)."""
    keys = ["cls_token", "pos_embed"] + (["register_tokens"] if R else []) + ["mask_token", "patch_embed.proj.weight", "patch_embed.proj.bias"]
    for i in range(depth):
        keys += [f"blocks.{i}.{n}" for n in ("norm1.weight", "norm1.bias", "attn.qkv.weight", "attn.qkv.bias", "attn.proj.weight", "attn.proj.bias",
                                             "ls1.gamma", "norm2.weight", "norm2.bias", "mlp.fc1.weight", "mlp.fc1.bias", "mlp.fc2.weight",
                                             "mlp.fc2.bias", "ls2.gamma")]
    return keys + ["norm.weight", "norm.bias"]


def random_state_dict(D: int, depth: int, grid: int, R: int, seed: int = 0, mlp_ratio: int = 4):
    """Deterministic fp32 weights of a (D, depth, grid x grid patches, R registers) model: Linear / conv weights ~ N(0, 1 / fan_in) so that
    activations keep unit scale, LayerNorm gains around 1, ls*.gamma ~ U(0.5, 1.5) (a LayerScale that does something)."""
    g = torch.Generator().manual_seed(seed)
    rn = lambda *s, std=1.0: torch.randn(*s, generator=g) * std
    sd = {"cls_token": rn(1, 1, D), "pos_embed": rn(1, 1 + grid * grid, D, std=0.5), "mask_token": torch.zeros(1, D),
          "patch_embed.proj.weight": rn(D, 3, PATCH, PATCH, std=PATCH_K ** -0.5), "patch_embed.proj.bias": rn(D, std=0.1)}
    if R:
        sd["register_tokens"] = rn(1, R, D)
    Hd = D * mlp_ratio
    for i in range(depth):
        p = f"blocks.{i}."
        for n, (o, k) in (("attn.qkv", (3 * D, D)), ("attn.proj", (D, D)), ("mlp.fc1", (Hd, D)), ("mlp.fc2", (D, Hd))):
            sd[p + n + ".weight"] = rn(o, k, std=k ** -0.5)
            sd[p + n + ".bias"] = rn(o, std=0.1)
        for n in ("norm1", "norm2"):
            sd[p + n + ".weight"] = 1.0 + rn(D, std=0.1)
            sd[p + n + ".bias"] = rn(D, std=0.1)
        for n in ("ls1", "ls2"):
            sd[p + n + ".gamma"] = 0.5 + torch.rand(D, generator=g)
    sd["norm.weight"] = 1.0 + rn(D, std=0.1)
    sd["norm.bias"] = rn(D, std=0.1)
    return {k: sd[k] for k in state_dict_keys(depth, R)}


def to_hf(sd: dict) -> dict:
    """The same weights under the names of transformers' Dinov2Model / Dinov2WithRegistersModel (qkv split into query / key / value)."""
    out = {"embeddings.cls_token": sd["cls_token"], "embeddings.mask_token": sd["mask_token"], "embeddings.position_embeddings": sd["pos_embed"],
           "embeddings.patch_embeddings.projection.weight": sd["patch_embed.proj.weight"],
           "embeddings.patch_embeddings.projection.bias": sd["patch_embed.proj.bias"],
           "layernorm.weight": sd["norm.weight"], "layernorm.bias": sd["norm.bias"]}
    if "register_tokens" in sd:
        out["embeddings.register_tokens"] = sd["register_tokens"]
    names = {"norm1.weight": "norm1.weight", "norm1.bias": "norm1.bias", "norm2.weight": "norm2.weight", "norm2.bias": "norm2.bias",
             "attn.proj.weight": "attention.output.dense.weight", "attn.proj.bias": "attention.output.dense.bias",
             "ls1.gamma": "layer_scale1.lambda1", "ls2.gamma": "layer_scale2.lambda1",
             "mlp.fc1.weight": "mlp.fc1.weight", "mlp.fc1.bias": "mlp.fc1.bias", "mlp.fc2.weight": "mlp.fc2.weight", "mlp.fc2.bias": "mlp.fc2.bias"}
    i = 0
    while f"blocks.{i}.norm1.weight" in sd:
        for a, b in names.items():
            out[f"encoder.layer.{i}.{b}"] = sd[f"blocks.{i}.{a}"]
        D = sd[f"blocks.{i}.attn.qkv.weight"].shape[1]
        for j, n in enumerate(("query", "key", "value")):
            out[f"encoder.layer.{i}.attention.attention.{n}.weight"] = sd[f"blocks.{i}.attn.qkv.weight"][j * D:(j + 1) * D]
            out[f"encoder.layer.{i}.attention.attention.{n}.bias"] = sd[f"blocks.{i}.attn.qkv.bias"][j * D:(j + 1) * D]
        i += 1
    return out


def depth_of(sd) -> int:
    i = 0
    while f"blocks.{i}.norm1.weight" in sd:
        i += 1
    return i


# ---- the operands of the patch convolution -------------------------------------------------------------------------------------------------
def zscore(img: torch.Tensor, dtype=torch.float32) -> torch.Tensor:
    """(img - mean_c) / std_c in `dtype` (fp32: the kernel's arithmetic -- subtract, then divide, correctly rounded each)."""
    m = torch.tensor(IMAGENET_MEAN, dtype=dtype).view(1, 3, 1, 1)
    s = torch.tensor(IMAGENET_STD, dtype=dtype).view(1, 3, 1, 1)
    return (img.to(dtype) - m) / s


def patch_operand(img: torch.Tensor, dt, mutant=None) -> torch.Tensor:
    """The 16-bit A operand image of the patch GEMM as float64 (B, 3, H, W): the fp32 z-score rounded ONCE.
    mutant 'zscore_after_rounding': the pixels are rounded first and z-scored after."""
    if mutant == "zscore_after_rounding":
        return zscore(img.float().to(dt).float()).double()
    return zscore(img.float()).to(dt).double()


def patch_rows(a: torch.Tensor) -> torch.Tensor:
    """(B, 3, H, W) -> (B * n, 588): row = patch in raster order, column k = c * 196 + dy * 14 + dx (the conv weight's own flattening)."""
    B, C, H, W = a.shape
    u = a.unfold(2, PATCH, PATCH).unfold(3, PATCH, PATCH)                 # (B, 3, gh, gw, 14, 14)
    return u.permute(0, 2, 3, 1, 4, 5).reshape(B * (H // PATCH) * (W // PATCH), C * PATCH * PATCH)


# ---- the model -----------------------------------------------------------------------------------------------------------------------------
def gelu_tanh(x):
    return 0.5 * x * (1.0 + torch.tanh(math.sqrt(2.0 / math.pi) * (x + 0.044715 * x ** 3)))


def assemble(sd, conv, R, dtype, mutant=None):
    """conv (B, n, D) (with bias) -> the token stream (B, 1 + R + n, D)."""
    B = conv.shape[0]
    pos = sd["pos_embed"].to(dtype)
    cls = (sd["cls_token"].to(dtype) + pos[:, :1]).expand(B, -1, -1)
    toks = [cls]
    if R:
        reg = sd["register_tokens"].to(dtype)
        if mutant == "reg_pos":
            reg = reg + pos[:, :1]
        toks.append(reg.expand(B, -1, -1))
    toks.append(conv + pos[:, 1:])
    if mutant == "cls_last":
        toks = toks[1:] + toks[:1]
    return torch.cat(toks, 1)


def blocks(sd, x, mutant=None):
    dtype = x.dtype
    B, L, D = x.shape
    H = D // 64
    eps = 1e-5 if mutant == "eps_1e-5" else 1e-6
    act = gelu_tanh if mutant == "gelu_tanh" else gemm_ref.gelu_erf
    for i in range(depth_of(sd)):
        p = lambda n: sd[f"blocks.{i}.{n}"].to(dtype)
        ls1, ls2 = (1.0, 1.0) if mutant == "no_layerscale" else (p("ls1.gamma"), p("ls2.gamma"))
        h = F.layer_norm(x, (D,), p("norm1.weight"), p("norm1.bias"), eps)
        q, k, v = (h @ p("attn.qkv.weight").T + p("attn.qkv.bias")).view(B, L, 3, H, 64).permute(2, 0, 3, 1, 4)
        a = torch.softmax(q @ k.transpose(-1, -2) * 0.125, -1) @ v
        x = x + ls1 * (a.permute(0, 2, 1, 3).reshape(B, L, D) @ p("attn.proj.weight").T + p("attn.proj.bias"))
        h = F.layer_norm(x, (D,), p("norm2.weight"), p("norm2.bias"), eps)
        x = x + ls2 * (act(h @ p("mlp.fc1.weight").T + p("mlp.fc1.bias")) @ p("mlp.fc2.weight").T + p("mlp.fc2.bias"))
    return x


def readouts(sd, x):
    D = x.shape[-1]
    return {"x_prenorm": x, "x_norm": F.layer_norm(x, (D,), sd["norm.weight"].to(x.dtype), sd["norm.bias"].to(x.dtype), 1e-6),
            "trellis": F.layer_norm(x, (D,), None, None, 1e-5)}


def forward(sd, img, R, dtype=torch.float64, operand_dtype=None, normalized=False, mutant=None):
    """img (B, 3, H, W) in [0, 1] (normalized=True: z-scored already) -> {"x_prenorm", "x_norm", "trellis"} (B, 1 + R + n, D) in `dtype`.
    operand_dtype: the patch convolution contracts the 16-bit roundings of its two operands (patch_operand and the rounded weight), as the
    kernel does; None: no rounding anywhere."""
    w = sd["patch_embed.proj.weight"]
    if normalized:
        a = img.to(dtype)
    elif operand_dtype is not None:
        a = patch_operand(img, operand_dtype, mutant).to(dtype)
    else:
        a = zscore(img, dtype)
    if operand_dtype is not None:
        w = w.float().to(operand_dtype)
    conv = F.conv2d(a, w.to(dtype), sd["patch_embed.proj.bias"].to(dtype), stride=PATCH).flatten(2).transpose(1, 2)
    return readouts(sd, blocks(sd, assemble(sd, conv, R, dtype, mutant), mutant))


def cond_layout(x, R):
    """scripts/encode_img_cond_dinov2_feature.py:52-58: the patch tokens, then the cls token; registers dropped."""
    return torch.cat([x[:, R + 1:], x[:, :1]], 1)


def forward_autocast(sd, img, R, dt):
    """The torch composition a user of the reference runs -- F.conv2d, F.layer_norm, F.linear, F.scaled_dot_product_attention on fp32 parameters
    under torch.autocast('cpu', dt), fp32 residual stream: the yardstick of the whole-model test."""
    D = sd["cls_token"].shape[-1]
    H = D // 64
    p = {k: v.float() for k, v in sd.items()}
    with torch.no_grad(), torch.autocast("cpu", dtype=dt):
        conv = F.conv2d(zscore(img.float()), p["patch_embed.proj.weight"], p["patch_embed.proj.bias"], stride=PATCH).flatten(2).transpose(1, 2)
        x = assemble(p, conv.float(), R, torch.float32)
        B, L, _ = x.shape
        for i in range(depth_of(sd)):
            g = lambda n: p[f"blocks.{i}.{n}"]
            h = F.layer_norm(x, (D,), g("norm1.weight"), g("norm1.bias"), 1e-6)
            q, k, v = F.linear(h, g("attn.qkv.weight"), g("attn.qkv.bias")).view(B, L, 3, H, 64).permute(2, 0, 3, 1, 4)
            a = F.scaled_dot_product_attention(q, k, v).permute(0, 2, 1, 3).reshape(B, L, D)
            x = x + g("ls1.gamma") * F.linear(a, g("attn.proj.weight"), g("attn.proj.bias")).float()
            h = F.layer_norm(x, (D,), g("norm2.weight"), g("norm2.bias"), 1e-6)
            x = x + g("ls2.gamma") * F.linear(F.gelu(F.linear(h, g("mlp.fc1.weight"), g("mlp.fc1.bias"))), g("mlp.fc2.weight"), g("mlp.fc2.bias")).float()
    return readouts(p, x.float())


def rel_l2(a, b):
    a, b = a.double(), b.double()
    return float((a - b).norm() / b.norm().clamp_min(1e-300))


# ---- bounds of the new kernels (derived from their arithmetic; see csrc/vit.hip, csrc/gemm.hip) ---------------------------------------------
def patch_embed_model(img, sd, dt):
    """(ref, bound) float64 (B, n, D) of the patch rows of gvf_vit_patch_embed: the fp64 product of the 16-bit-rounded operands + bias + pos,
    and gemm_ref.accumulation_error at K = 608 (19 k-steps, the bias add) plus one fp32 rounding for the position add.  The A operand is
    the correctly rounded fp32 z-score: subtract and divide are IEEE operations on both sides, so it carries no error term of its own."""
    B = img.shape[0]
    A = patch_rows(patch_operand(img, dt))
    W = sd["patch_embed.proj.weight"].float().to(dt).double().reshape(-1, PATCH_K)
    b = sd["patch_embed.proj.bias"].double()
    pos = sd["pos_embed"][0, 1:].double()
    acc = (A @ W.T).view(B, -1, W.shape[0])
    S = (A.abs() @ W.abs().T).view(B, -1, W.shape[0])
    pre = acc + b
    ref = pre + pos
    e = gemm_ref.accumulation_error(PATCH_KPAD, S, b.abs()) + U32 * (pre.abs() + pos.abs())
    return ref, gemm_ref._round_bound(ref, e, None)


def gelu_erf_model(a16, w16, bias, a_err=None):
    """(ref, bound) of GVF_EPI_GELU_ERF_16: r16(gelu_erf(acc + bias)).  gemm_ref.model's accumulator and its error e (fp32 store epilogue), then
    the epilogue's fp32 arithmetic: 0.5 x (1 + erff(x / sqrt 2)) -- erff to a few ulp OF ITS VALUE NEAR 1, i.e. absolute 4 2^-24, so the product
    with 0.5 x carries 2 |x| 2^-24, the scaling of the argument and the two multiplications three roundings of the result; counted as
    8 2^-24 (|x| + |gelu(x)|), the budget gemm_ref gives erff inside GEGLU -- and the one rounding to 16 bits (gemm_ref._round_bound)."""
    pre, e = gemm_ref.model(a16, w16, bias, gemm_ref.EPI_STORE_F32, a_err=a_err)
    g = gemm_ref.gelu_erf(pre)
    E = gemm_ref.GELU_LIP * e + 8.0 * U32 * (pre.abs() + g.abs())
    return g, gemm_ref._round_bound(g, E, a16.dtype)


def layernorm_model(x, eps, w=None, b=None, out_dt=None):
    """(ref, bound) float64 of gvf_vit_tokens_out's LayerNorm over the last axis of the fp32 rows x, all in fp32 on the device:
    s = sum x (<= 4 values per lane: 3 in-lane adds, then a depth-6 tree: 9 roundings), mean = s / D (1), c = x - mean (1), q = sum c^2
    (1 + 9), var = q / D (1), rstd = rsqrtf(var + eps) (1 + ~2 ulp), y = c * rstd (1), z = y * w + b (2).  First order, rounding counts as factors."""
    xd = x.double()
    D = xd.shape[-1]
    mean = xd.mean(-1, keepdim=True)
    c = xd - mean
    var = (c * c).mean(-1, keepdim=True)
    rstd = 1.0 / torch.sqrt(var + eps)
    y = c * rstd
    e_mean = 10.0 * U32 * xd.abs().sum(-1, keepdim=True) / D
    e_c = e_mean + U32 * (xd.abs() + mean.abs())
    e_var = 12.0 * U32 * var + 2.0 * (c.abs() * e_c).sum(-1, keepdim=True) / D
    d_r = 0.5 * e_var / (var + eps) + 4.0 * U32
    e_y = e_c * rstd + y.abs() * (d_r + U32)
    ref = y
    if w is not None:
        ref = y * w.double() + b.double()
        e_y = e_y * w.double().abs() + 2.0 * U32 * ((y * w.double()).abs() + b.double().abs())
    return ref, gemm_ref._round_bound(ref, e_y, out_dt)
