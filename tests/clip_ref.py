"""Plain torch restatement of CLIP's ViT image tower as the HIP encoder implements it (gvfdiffusion_amd/model/clip.py, csrc/clip.hip), the key
map to the Hugging Face implementation it is checked against (tests/test_clip_ref.py), and the error bounds of the new kernels.

forward() is the whole tower in one dtype (float64 for the reference) from NORMALISED pixels: the 32 x 32 stride-32 convolution without bias,
token assembly [class_embedding + pos[0] | patches + pos[1:]], ln_pre, the blocks x += out_proj(attn(ln_1 x)); x += c_proj(quick_gelu(c_fc(ln_2
x))) (LayerNorm eps 1e-5, heads of 64, softmax scale 1/8, quick_gelu(v) = v sigmoid(1.702 v)), and the read-out ln_post(x[:, 0]) @ proj.
`mutant` switches ONE of the model's decisions to a plausible wrong one; the comparison of tests/test_clip_ref.py must reject each.

Everything here runs on torch CPU tensors."""
import numpy as np
import torch
import torch.nn.functional as F

import gemm_ref
import vit_ref

CLIP_MEAN, CLIP_STD = (0.48145466, 0.4578275, 0.40821073), (0.26862954, 0.26130258, 0.27577711)
PATCH, PATCH_K = 32, 3072
EPS = 1e-5
U32 = gemm_ref.U32
EPI_QUICK_GELU_16 = 6
QUICK_GELU_LIP = 1.13                # max |d/dv v sigmoid(1.702 v)| = 1.0998 (at v = 1.41); gemm_ref.GELU_LIP covers it
MUTANTS = ("gelu_erf", "no_ln_pre", "pos_after_ln_pre", "eps_1e-6", "ln_post_patch", "mean_pool", "proj_transposed", "conv_bias", "flatten_dydxc")
rel_l2 = vit_ref.rel_l2


# ---- weights ----------------------------------------------------------------------------------------------------------------------------
def state_dict_keys(depth: int):
    """OpenAI's `model.visual` parameter names (from memory of the public checkpoint: unpinned), in nn.Module.state_dict() order."""
    keys = ["class_embedding", "positional_embedding", "proj", "conv1.weight", "ln_pre.weight", "ln_pre.bias"]
    for i in range(depth):
        keys += [f"transformer.resblocks.{i}.{n}" for n in ("attn.in_proj_weight", "attn.in_proj_bias", "attn.out_proj.weight", "attn.out_proj.bias",
                                                            "ln_1.weight", "ln_1.bias", "mlp.c_fc.weight", "mlp.c_fc.bias", "mlp.c_proj.weight",
                                                            "mlp.c_proj.bias", "ln_2.weight", "ln_2.bias")]
    return keys + ["ln_post.weight", "ln_post.bias"]


def random_state_dict(D: int, depth: int, grid: int, E: int, seed: int = 0):
    """Deterministic fp32 weights of a (width D, depth, grid x grid patches, E features) tower: Linear / conv weights ~ N(0, 1 / fan_in) so that
    activations keep unit scale, LayerNorm gains around 1."""
    g = torch.Generator().manual_seed(seed)
    rn = lambda *s, std=1.0: torch.randn(*s, generator=g) * std
    sd = {"class_embedding": rn(D), "positional_embedding": rn(1 + grid * grid, D, std=0.5), "proj": rn(D, E, std=D ** -0.5),
          "conv1.weight": rn(D, 3, PATCH, PATCH, std=PATCH_K ** -0.5)}
    for n in ("ln_pre", "ln_post"):
        sd[n + ".weight"] = 1.0 + rn(D, std=0.1)
        sd[n + ".bias"] = rn(D, std=0.1)
    for i in range(depth):
        p = f"transformer.resblocks.{i}."
        for n, (o, k) in (("attn.in_proj_", (3 * D, D)), ("attn.out_proj.", (D, D)), ("mlp.c_fc.", (4 * D, D)), ("mlp.c_proj.", (D, 4 * D))):
            sd[p + n + "weight"] = rn(o, k, std=k ** -0.5)
            sd[p + n + "bias"] = rn(o, std=0.1)
        for n in ("ln_1", "ln_2"):
            sd[p + n + ".weight"] = 1.0 + rn(D, std=0.1)
            sd[p + n + ".bias"] = rn(D, std=0.1)
    return {k: sd[k] for k in state_dict_keys(depth)}


def depth_of(sd) -> int:
    i = 0
    while f"transformer.resblocks.{i}.ln_1.weight" in sd:
        i += 1
    return i


def to_hf(sd: dict) -> dict:
    """The same weights under the names of transformers' CLIPVisionModelWithProjection (in_proj split into q / k / v, proj transposed)."""
    p = "vision_model."
    out = {p + "embeddings.class_embedding": sd["class_embedding"], p + "embeddings.position_embedding.weight": sd["positional_embedding"],
           p + "embeddings.patch_embedding.weight": sd["conv1.weight"], "visual_projection.weight": sd["proj"].t().contiguous()}
    for a, b in (("ln_pre", "pre_layrnorm"), ("ln_post", "post_layernorm")):
        for n in ("weight", "bias"):
            out[f"{p}{b}.{n}"] = sd[f"{a}.{n}"]
    names = {"ln_1": "layer_norm1", "ln_2": "layer_norm2", "attn.out_proj": "self_attn.out_proj", "mlp.c_fc": "mlp.fc1", "mlp.c_proj": "mlp.fc2"}
    for i in range(depth_of(sd)):
        src, dst = f"transformer.resblocks.{i}.", f"{p}encoder.layers.{i}."
        for a, b in names.items():
            for n in ("weight", "bias"):
                out[f"{dst}{b}.{n}"] = sd[f"{src}{a}.{n}"]
        D = sd[src + "attn.in_proj_weight"].shape[1]
        for j, q in enumerate(("q", "k", "v")):
            out[f"{dst}self_attn.{q}_proj.weight"] = sd[src + "attn.in_proj_weight"][j * D:(j + 1) * D]
            out[f"{dst}self_attn.{q}_proj.bias"] = sd[src + "attn.in_proj_bias"][j * D:(j + 1) * D]
    return out


# ---- pixels -------------------------------------------------------------------------------------------------------------------------------
def operand_table(dt) -> torch.Tensor:
    """(3, 256): ToTensor -> Normalize in fp32 ((u8 / 255 - mean) / std: divide, subtract, divide), then one rounding to `dt`."""
    u = torch.arange(256, dtype=torch.float32)[None].repeat(3, 1) / 255
    return ((u - torch.tensor(CLIP_MEAN).view(3, 1)) / torch.tensor(CLIP_STD).view(3, 1)).to(dt)


def normalise_u8(img_u8: torch.Tensor, dtype=torch.float32) -> torch.Tensor:
    """uint8 (B, 3, S, S) -> (u8 / 255 - mean) / std in `dtype`."""
    m = torch.tensor(CLIP_MEAN, dtype=dtype).view(1, 3, 1, 1)
    s = torch.tensor(CLIP_STD, dtype=dtype).view(1, 3, 1, 1)
    return (img_u8.to(dtype) / 255 - m) / s


def preprocess_u8(images01: torch.Tensor, size: int = 224, rounding: bool = False) -> torch.Tensor:
    """fp32 (F, 3, S, S) in [0, 1] -> uint8 (F, 3, size, size) on the host: numpy truncation of x * 255 (torchvision's ToPILImage:
    pic.mul(255).byte()) + PIL.Image.resize((size, size), BICUBIC).  rounding=True: the mutant that rounds x * 255 instead."""
    from PIL import Image
    v = images01.float().mul(255)
    u8 = (v.round() if rounding else v).numpy().astype(np.uint8)
    out = [np.asarray(Image.fromarray(np.ascontiguousarray(f.transpose(1, 2, 0))).resize((size, size), Image.BICUBIC)) for f in u8]
    return torch.from_numpy(np.stack(out)).permute(0, 3, 1, 2).contiguous()


def patch_rows(a: torch.Tensor, order: str = "cdydx") -> torch.Tensor:
    """(B, 3, S, S) -> (B * n, 3072): row = patch in raster order, column k = c * 1024 + dy * 32 + dx (the conv weight's own flattening);
    order 'dydxc': the (dy, dx, c) flattening of the mutant."""
    B, C, H, W = a.shape
    u = a.unfold(2, PATCH, PATCH).unfold(3, PATCH, PATCH)                 # (B, 3, gh, gw, 32, 32)
    if order == "dydxc":
        return u.permute(0, 2, 3, 4, 5, 1).reshape(B * (H // PATCH) * (W // PATCH), C * PATCH * PATCH)
    return u.permute(0, 2, 3, 1, 4, 5).reshape(B * (H // PATCH) * (W // PATCH), C * PATCH * PATCH)


# ---- the model ---------------------------------------------------------------------------------------------------------------------------
def quick_gelu(x):
    return x * torch.sigmoid(1.702 * x)


def front(sd, pix, dtype, operand_dtype=None, mutant=None):
    """Normalised pixels (B, 3, S, S) -> the stream that enters block 0 (B, 1 + n, D)."""
    w = sd["conv1.weight"]
    a = pix
    if operand_dtype is not None:
        w, a = w.float().to(operand_dtype), pix.float().to(operand_dtype)
    a, w = a.to(dtype), w.to(dtype)
    B, D = a.shape[0], w.shape[0]
    conv = (patch_rows(a, "dydxc" if mutant == "flatten_dydxc" else "cdydx") @ w.reshape(D, -1).T).view(B, -1, D)
    if mutant == "conv_bias":
        conv = conv + torch.randn(D, generator=torch.Generator().manual_seed(77)).to(dtype) * 0.1
    pos = sd["positional_embedding"].to(dtype)
    cls = sd["class_embedding"].to(dtype).expand(B, 1, D)
    x = torch.cat([cls, conv], 1)
    if mutant != "pos_after_ln_pre":
        x = x + pos
    if mutant != "no_ln_pre":
        x = F.layer_norm(x, (D,), sd["ln_pre.weight"].to(dtype), sd["ln_pre.bias"].to(dtype), 1e-6 if mutant == "eps_1e-6" else EPS)
    if mutant == "pos_after_ln_pre":
        x = x + pos
    return x


def blocks(sd, x, mutant=None):
    dtype = x.dtype
    B, L, D = x.shape
    H = D // 64
    eps = 1e-6 if mutant == "eps_1e-6" else EPS
    act = gemm_ref.gelu_erf if mutant == "gelu_erf" else quick_gelu
    for i in range(depth_of(sd)):
        p = lambda n: sd[f"transformer.resblocks.{i}.{n}"].to(dtype)
        h = F.layer_norm(x, (D,), p("ln_1.weight"), p("ln_1.bias"), eps)
        q, k, v = (h @ p("attn.in_proj_weight").T + p("attn.in_proj_bias")).view(B, L, 3, H, 64).permute(2, 0, 3, 1, 4)
        a = torch.softmax(q @ k.transpose(-1, -2) * 0.125, -1) @ v
        x = x + (a.permute(0, 2, 1, 3).reshape(B, L, D) @ p("attn.out_proj.weight").T + p("attn.out_proj.bias"))
        h = F.layer_norm(x, (D,), p("ln_2.weight"), p("ln_2.bias"), eps)
        x = x + (act(h @ p("mlp.c_fc.weight").T + p("mlp.c_fc.bias")) @ p("mlp.c_proj.weight").T + p("mlp.c_proj.bias"))
    return x


def readout(sd, x, mutant=None):
    D = x.shape[-1]
    tok = x[:, 1] if mutant == "ln_post_patch" else (x.mean(1) if mutant == "mean_pool" else x[:, 0])
    h = F.layer_norm(tok, (D,), sd["ln_post.weight"].to(x.dtype), sd["ln_post.bias"].to(x.dtype), 1e-6 if mutant == "eps_1e-6" else EPS)
    proj = sd["proj"].to(x.dtype)
    if mutant == "proj_transposed":                      # the stored (D, E) buffer read as (E, D)
        proj = proj.reshape(proj.shape[1], proj.shape[0]).T
    return h @ proj


def forward(sd, pix, dtype=torch.float64, operand_dtype=None, mutant=None):
    """Normalised pixels (B, 3, S, S) -> {"stream": (B, 1 + n, D) behind the last block, "feat": (B, E)} in `dtype`."""
    x = blocks(sd, front(sd, pix, dtype, operand_dtype, mutant), mutant)
    return {"stream": x, "feat": readout(sd, x, mutant)}


def cosine(f, g):
    """rows of f against the vector g, in f's dtype"""
    return (f / f.norm(dim=-1, keepdim=True)) @ (g / g.norm())


def forward_autocast(sd, pix, dt):
    """The torch composition a user of the reference runs -- F.conv2d, F.layer_norm, F.linear, F.scaled_dot_product_attention on fp32 parameters
    under torch.autocast('cpu', dt), fp32 residual stream: the yardstick of the whole-model test.  -> features (B, E) fp32."""
    p = {k: v.float() for k, v in sd.items()}
    D = p["class_embedding"].shape[0]
    H = D // 64
    with torch.no_grad(), torch.autocast("cpu", dtype=dt):
        conv = F.conv2d(pix.float(), p["conv1.weight"], None, stride=PATCH).flatten(2).transpose(1, 2).float()
        B = conv.shape[0]
        x = torch.cat([p["class_embedding"].expand(B, 1, D), conv], 1) + p["positional_embedding"]
        x = F.layer_norm(x, (D,), p["ln_pre.weight"], p["ln_pre.bias"], EPS).float()
        L = x.shape[1]
        for i in range(depth_of(sd)):
            g = lambda n: p[f"transformer.resblocks.{i}.{n}"]
            h = F.layer_norm(x, (D,), g("ln_1.weight"), g("ln_1.bias"), EPS)
            q, k, v = F.linear(h, g("attn.in_proj_weight"), g("attn.in_proj_bias")).view(B, L, 3, H, 64).permute(2, 0, 3, 1, 4)
            a = F.scaled_dot_product_attention(q, k, v).permute(0, 2, 1, 3).reshape(B, L, D)
            x = x + F.linear(a, g("attn.out_proj.weight"), g("attn.out_proj.bias")).float()
            h = F.layer_norm(x, (D,), g("ln_2.weight"), g("ln_2.bias"), EPS)
            u = F.linear(h, g("mlp.c_fc.weight"), g("mlp.c_fc.bias"))
            x = x + F.linear(u * torch.sigmoid(1.702 * u), g("mlp.c_proj.weight"), g("mlp.c_proj.bias")).float()
        h = F.layer_norm(x[:, 0], (D,), p["ln_post.weight"], p["ln_post.bias"], EPS)
        f = F.linear(h, p["proj"].t().contiguous())
    return f.float()


# ---- bounds of the new kernels (derived from their arithmetic; see csrc/clip.hip, csrc/gemm.hip) ---------------------------------------------
def patch_embed_model(a16, sd, dt):
    """(ref, bound) float64 (B, n, D) of the patch rows of gvf_clip_patch_embed (before ln_pre) for the 16-bit operand image a16 (B, 3, S, S),
    given as float64: the fp64 product of the 16-bit operands + pos, and gemm_ref.accumulation_error at K = 3072 -- (96 k-steps + 2) 2^-24
    sum |a w| -- plus one fp32 rounding for the position add."""
    B = a16.shape[0]
    A = patch_rows(a16)
    W = sd["conv1.weight"].float().to(dt).double().reshape(-1, PATCH_K)
    pos = sd["positional_embedding"][1:].double()
    acc = (A @ W.T).view(B, -1, W.shape[0])
    S = (A.abs() @ W.abs().T).view(B, -1, W.shape[0])
    ref = acc + pos
    e = gemm_ref.accumulation_error(PATCH_K, S, torch.zeros(())) + U32 * (acc.abs() + pos.abs())
    return ref, e


def quick_gelu_model(a16, w16, bias, a_err=None):
    """(ref, bound) of GVF_EPI_QUICK_GELU_16: r16(v / (1 + expf(-1.702 v))), v = acc + bias.  gemm_ref.model's accumulator and its error e (fp32
    store epilogue) carried through |d/dv| <= 1.13, then the epilogue's fp32 arithmetic: t = -1.702 v (one rounding: |t| 2^-24 absolute),
    E = expf(t) (relative (|t| + 2) 2^-24 with expf's ~1 ulp), 1 + E and the division one rounding each.  d g / d E = -g / (1 + E), so E's
    error reaches g as |g| sigmoid(t) (|t| + 2) 2^-24.  Absolute floor 1e-36: expf overflows to inf once t > 88.72 (v < -52.1), where the
    exact |g| < 53 e^-88.7 = 1.6e-37 and the kernel returns -0; below that lie fp32 subnormals.  Then one rounding to 16 bits."""
    pre, e = gemm_ref.model(a16, w16, bias, gemm_ref.EPI_STORE_F32, a_err=a_err)
    g = pre * torch.sigmoid(1.702 * pre)
    t = (1.702 * pre).abs()
    E = QUICK_GELU_LIP * e + g.abs() * (torch.sigmoid(-1.702 * pre) * (t + 2.0) + 2.0) * U32 + 1e-36
    return g, gemm_ref._round_bound(g, E, a16.dtype)


def head_model(x0, sd, dt, eps=EPS):
    """(ref, bound) float64 (B, E) of gvf_clip_head's features for the fp32 cls rows x0 (B, D): h = r16(LN(x0)) -- vit_ref.layernorm_model's
    fp32 error decides which 16-bit values the kernel may hold (amb, as gemm_ref.ln_operand) --, then one fp32 fma per term in ascending d
    (D roundings of a partial sum of at most S = sum |h p|), then one rounding to 16 bits."""
    ln_ref, ln_e = vit_ref.layernorm_model(x0, eps, sd["ln_post.weight"], sd["ln_post.bias"], None)
    h16 = gemm_ref.r16(ln_ref, dt)
    amb = gemm_ref.r16(ln_ref + ln_e, dt) - gemm_ref.r16(ln_ref - ln_e, dt)
    P = sd["proj"].float().to(dt).double()
    pre = h16 @ P
    S = h16.abs() @ P.abs()
    e = x0.shape[-1] * U32 * S + amb.abs() @ P.abs()
    return pre, gemm_ref._round_bound(pre, e, dt)


def unit_model(f):
    """(unit, bound, ss) float64 of gvf_clip_head's unit vector for ITS OWN features f (B, E) fp32: sum of squares -- at most 4 products and 4
    adds in a thread, a depth-6 tree, 3 adds over the waves: 17 roundings, relative 17 2^-24 --, sqrtf (1), so |f| to 10 2^-24; the division one
    more: 12 2^-24 |unit| covers it."""
    fd = f.double()
    n = fd.norm(dim=-1, keepdim=True)
    u = fd / n
    return u, 12.0 * U32 * u.abs()


def sim_model(unit, g):
    """(sim, bound) float64 of <unit, g> for the kernel's own unit vectors (B, E) fp32: a product and an add per term in the same 17-rounding
    tree: 18 2^-24 sum |u g|."""
    ud, gd = unit.double(), g.double()
    return ud @ gd, 18.0 * U32 * (ud.abs() @ gd.abs())
