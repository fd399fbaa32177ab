"""CLIP's image tower (ViT-B/32) for inference on the MI355X: pixels -> image features -> cosine similarity, the CLIP term of the alignment
score (utils/inference_utils.py:37-178 of the reference: `l1 + 0.2 * (1 - cos(CLIP(render), CLIP(canonical)))`).

The reference takes the model from `clip.load("ViT-B/32")`; its source is not part of the reference, so this is a restatement of the public
architecture (OpenAI's clip/model.py VisionTransformer):
    x = ln_pre([class_embedding + pos[0] | conv32(pixels) + pos[1:]])               (conv1 has no bias)
    per block:  x += out_proj(attn(ln_1 x));  x += c_proj(quick_gelu(c_fc(ln_2 x)))  (LayerNorm eps 1e-5, heads of 64, x * sigmoid(1.702 x))
    features = ln_post(x[:, 0]) @ proj
The parameters carry the names of OpenAI's `model.visual` state dict (written from memory of the public checkpoint: unpinned, see
DESIGN.md), so a released state dict loads with strict=True; load_clip_state_dict also takes a full CLIP state dict and a transformers
CLIPVisionModelWithProjection one.  No weights are fetched here: clip_vit_b32() builds the architecture with its initial values.

Every operation between the pixels and the similarity is a launch of the HIP library: ops.clip.patch_embed and ops.clip.ln_rows (ln_pre, which
also writes the LayerNorm statistics of block 0's ln_1), then five launches per block -- gvf_gemm_ln (in_proj), gvf_attn_fwd,
gvf_gemm_resid_stats (out_proj), gvf_gemm_ln (c_fc with the QuickGELU epilogue), gvf_gemm_resid_stats (c_proj) -- and ops.clip.head.  The
residual stream is fp32 (the reference's is fp16), the matrix operands fp16 or bf16 (`dtype`).  There is no torch fall-back."""
import torch
import torch.nn as nn

from .. import _lib
from ..ops import clip as clip_ops, dit_ops
from ..rasterizer import frames_to_uint8
from ..utils.image_ops import resize_pad_crop_u8

__all__ = ["CLIPVisionTransformer", "clip_vit_b32", "load_clip_state_dict", "clip_preprocess_u8"]

HEAD_DIM = 64
LN_EPS = 1e-5


class _Attention(nn.Module):
    """The parameters of nn.MultiheadAttention under its names (in_proj_weight (3D, D), in_proj_bias, out_proj)."""
    def __init__(self, dim):
        super().__init__()
        self.in_proj_weight = nn.Parameter(torch.empty(3 * dim, dim))
        self.in_proj_bias = nn.Parameter(torch.zeros(3 * dim))
        self.out_proj = nn.Linear(dim, dim)
        nn.init.xavier_uniform_(self.in_proj_weight)


class _Mlp(nn.Module):
    def __init__(self, dim):
        super().__init__()
        self.c_fc = nn.Linear(dim, 4 * dim)
        self.c_proj = nn.Linear(4 * dim, dim)


class _ResidualAttentionBlock(nn.Module):
    def __init__(self, dim):
        super().__init__()
        self.attn = _Attention(dim)
        self.ln_1 = nn.LayerNorm(dim, eps=LN_EPS)
        self.mlp = _Mlp(dim)
        self.ln_2 = nn.LayerNorm(dim, eps=LN_EPS)


class _Transformer(nn.Module):
    def __init__(self, dim, layers):
        super().__init__()
        self.resblocks = nn.ModuleList([_ResidualAttentionBlock(dim) for _ in range(layers)])


class CLIPVisionTransformer(nn.Module):
    def __init__(self, input_resolution: int = 224, patch_size: int = 32, width: int = 768, layers: int = 12, heads: int = 12,
                 output_dim: int = 512, dtype=torch.float16):
        super().__init__()
        if patch_size != clip_ops.PATCH:
            raise NotImplementedError(f"patch_size={patch_size} is not built: the patch-embedding kernel is the 32 x 32 one")
        if input_resolution <= 0 or input_resolution % patch_size != 0:
            raise NotImplementedError(f"input_resolution={input_resolution} is not built: the image side must be a multiple of the patch size 32")
        if width % 128 != 0 or width > 1024 or width != heads * HEAD_DIM:
            raise NotImplementedError(f"width={width}, heads={heads} is not built: heads of 64, width a multiple of 128 up to 1024 "
                                      "(the LayerNorm-folded GEMM stages K <= 1024)")
        if output_dim % 64 != 0 or output_dim > 1024 or output_dim <= 0:
            raise NotImplementedError(f"output_dim={output_dim} is not built: the read-out takes a multiple of 64 up to 1024")
        if dtype not in dit_ops.LP_DTYPES:
            raise ValueError("dtype must be torch.float16 or torch.bfloat16")
        self.input_resolution, self.patch_size, self.width, self.heads, self.output_dim = input_resolution, patch_size, width, heads, output_dim
        self.num_patches = (input_resolution // patch_size) ** 2
        self.lp = dtype
        self.image_mean, self.image_std = clip_ops.CLIP_MEAN, clip_ops.CLIP_STD
        scale = width ** -0.5
        self.class_embedding = nn.Parameter(scale * torch.randn(width))
        self.positional_embedding = nn.Parameter(scale * torch.randn(1 + self.num_patches, width))
        self.proj = nn.Parameter(scale * torch.randn(width, output_dim))
        self.conv1 = nn.Conv2d(3, width, kernel_size=patch_size, stride=patch_size, bias=False)
        self.ln_pre = nn.LayerNorm(width, eps=LN_EPS)
        self.transformer = _Transformer(width, layers)
        self.ln_post = nn.LayerNorm(width, eps=LN_EPS)
        self._images = None                            # the 16-bit weight images, built once per load (key: device, dtype)
        self.register_load_state_dict_post_hook(lambda module, incompatible: module.drop_weight_images())
        self.requires_grad_(False)
        self.eval()

    # ---- the 16-bit weight images ------------------------------------------------------------------------------------------------------
    def drop_weight_images(self):
        self._images = None

    def _apply(self, fn, *args, **kwargs):             # .to() / .cuda() move the parameters: the images follow on the next call
        self._images = None
        return super()._apply(fn, *args, **kwargs)

    def train(self, mode: bool = True):
        if mode:
            raise NotImplementedError("training is not built: the CLIP image tower is inference only")
        return super().train(False)

    def weight_images(self):
        dev = self.class_embedding.device
        key = (dev, self.lp)
        if self._images is not None and self._images["key"] == key:
            return self._images
        f32 = lambda p: p.detach().float().contiguous()
        lp = lambda p: p.detach().to(self.lp).contiguous()
        ln = lambda m: (f32(m.weight), f32(m.bias))
        im = {"key": key, "patch_w": clip_ops.pack_patch_weight(f32(self.conv1.weight), self.lp),
              "lut": clip_ops.operand_table(self.lp, self.image_mean, self.image_std).to(dev),
              "cls": f32(self.class_embedding), "pos": f32(self.positional_embedding), "ln_pre": ln(self.ln_pre), "ln_post": ln(self.ln_post),
              "proj": lp(self.proj), "blocks": []}
        for b in self.transformer.resblocks:
            im["blocks"].append({"ln_1": ln(b.ln_1), "in_proj": (lp(b.attn.in_proj_weight), f32(b.attn.in_proj_bias)),
                                 "out_proj": (lp(b.attn.out_proj.weight), f32(b.attn.out_proj.bias)), "ln_2": ln(b.ln_2),
                                 "c_fc": (lp(b.mlp.c_fc.weight), f32(b.mlp.c_fc.bias)), "c_proj": (lp(b.mlp.c_proj.weight), f32(b.mlp.c_proj.bias))})
        self._images = im
        return im

    # ---- forward -----------------------------------------------------------------------------------------------------------------------
    def _check_pixels(self, x):
        _lib.require_cuda(x)
        if x.dim() != 4 or x.shape[1] != 3 or x.dtype not in (torch.uint8, torch.float32):
            raise _lib.GvfError(f"the encoder takes a uint8 or an fp32 (normalised) (B, 3, S, S) image, got {x.dtype} {tuple(x.shape)}")
        if x.device != self.class_embedding.device:
            raise _lib.GvfError("image and model are on different devices")
        if x.shape[2] != x.shape[3]:
            raise _lib.GvfError(f"non-square images are not built: got {x.shape[2]} x {x.shape[3]}")
        if x.shape[2] % self.patch_size != 0 or x.shape[2] != self.input_resolution:
            raise _lib.GvfError(f"the image side must be {self.input_resolution} (a multiple of 32, the grid positional_embedding holds), got {x.shape[2]}")

    @torch.no_grad()
    def forward_stream(self, x: torch.Tensor) -> torch.Tensor:
        """x uint8 (B, 3, S, S) (the z-score is the patch kernel's operand table) or fp32 (B, 3, S, S), normalised already -> the fp32
        token stream (B, 1 + n, D) behind the last block (ln_post not applied)."""
        self._check_pixels(x)
        im = self.weight_images()
        D, H = self.width, self.heads
        x3 = clip_ops.patch_embed(x, im["patch_w"], im["cls"], im["pos"], im["lut"])
        B, L, _ = x3.shape
        M = B * L
        xs = x3.view(M, D)
        n_part = dit_ops.gemm_stats_parts(D)
        dev = xs.device
        stats = torch.empty((M, n_part, 2), dtype=torch.float32, device=dev)
        clip_ops.ln_rows(xs, im["ln_pre"][0], im["ln_pre"][1], LN_EPS, stats)
        qkv = torch.empty((M, 3 * D), dtype=self.lp, device=dev)
        ab = torch.empty((M, D), dtype=self.lp, device=dev)
        hidden = torch.empty((M, 4 * D), dtype=self.lp, device=dev)
        s_qkv, s_o = (L * 3 * D, 0, 3 * D), (L * D, 0, D)
        for b in im["blocks"]:
            dit_ops.gemm_ln_bf16(xs, stats, n_part, b["in_proj"][0], b["in_proj"][1], qkv, dit_ops.EPI_STORE_16, eps=LN_EPS, ln_w=b["ln_1"][0],
                                 ln_b=b["ln_1"][1])
            dit_ops.attention(qkv, qkv[:, D:], qkv[:, 2 * D:], ab, B, 1, L, L, H, s_qkv, s_qkv, s_qkv, s_o, head_dim=HEAD_DIM)
            dit_ops.gemm_resid_stats(ab, b["out_proj"][0], b["out_proj"][1], xs, stats)
            dit_ops.gemm_ln_bf16(xs, stats, n_part, b["c_fc"][0], b["c_fc"][1], hidden, dit_ops.EPI_QUICK_GELU_16, eps=LN_EPS, ln_w=b["ln_2"][0],
                                 ln_b=b["ln_2"][1])
            dit_ops.gemm_resid_stats(hidden, b["c_proj"][0], b["c_proj"][1], xs, stats)
        return x3

    @torch.no_grad()
    def encode(self, x: torch.Tensor, ref_unit: torch.Tensor = None):
        """x as forward_stream takes it -> (features (B, E), features / |features| (B, E), <unit, ref_unit> (B,) or None), fp32."""
        xs = self.forward_stream(x)
        im = self.weight_images()
        return clip_ops.head(xs, im["ln_post"][0], im["ln_post"][1], im["proj"], ref_unit, LN_EPS)

    def encode_image(self, x: torch.Tensor) -> torch.Tensor:
        """The image features (B, output_dim), fp32, of uint8 pixels or of an fp32 image normalised already (`encode_image(preprocess(pil))`)."""
        return self.encode(x)[0]

    forward = encode_image

    @torch.no_grad()
    def similarity(self, images: torch.Tensor, canonical: torch.Tensor) -> torch.Tensor:
        """images fp32 (F, 3, S, S) in [0, 1], S square -> (F,) cosine similarity of each image's features with the canonical image's.
        canonical: an image (3, S, S) / (1, 3, S, S) in [0, 1], encoded once here, or the unit feature vector (E,) of one encoded earlier
        (`unit_feature`).  One batched pass of the encoder; nothing is read back to the host."""
        ref = canonical if canonical.dim() == 1 else self.unit_feature(canonical)
        return self.encode(clip_preprocess_u8(images, self.input_resolution), ref)[2]

    @torch.no_grad()
    def unit_feature(self, image: torch.Tensor) -> torch.Tensor:
        """image fp32 (3, S, S) or (1, 3, S, S) in [0, 1] -> its unit feature vector (E,), fp32."""
        if image.dim() == 3:
            image = image[None]
        if image.shape[0] != 1:
            raise _lib.GvfError("unit_feature takes one image")
        return self.encode(clip_preprocess_u8(image, self.input_resolution))[1][0].contiguous()


def clip_preprocess_u8(images: torch.Tensor, size: int = 224) -> torch.Tensor:
    """fp32 (F, 3, S, S) in [0, 1] on the device -> uint8 (F, 3, size, size): the reference's `preprocess(ToPILImage()(image))` up to the
    z-score (which the patch kernel's operand table applies).
      1. x * 255 truncated to uint8: torchvision's ToPILImage on a float tensor is `pic.mul(255).byte()` (restated from torchvision's public
         source: the package is not a dependency here); values are clamped to [0, 1] first, which is the identity on the stated domain;
      2. Pillow's bicubic resize to size x size (csrc/resize.hip, bit-identical): for a square image `Resize(size, BICUBIC)` + `CenterCrop(size)`.
    Only square inputs are built."""
    _lib.require_cuda(images)
    if images.dim() != 4 or images.shape[1] != 3 or images.dtype != torch.float32:
        raise _lib.GvfError(f"clip_preprocess_u8 takes an fp32 (F, 3, S, S) image in [0, 1], got {images.dtype} {tuple(images.shape)}")
    if images.shape[2] != images.shape[3]:
        raise _lib.GvfError(f"non-square images are not built: got {images.shape[2]} x {images.shape[3]}")
    return resize_pad_crop_u8(frames_to_uint8(images), size, out_size=size, filt="bicubic")


def clip_vit_b32(dtype=torch.float16, **kwargs) -> CLIPVisionTransformer:
    """ViT-B/32 at 224 x 224 (7 x 7 patches, 50 tokens), 512 output features: the architecture only -- load a state dict to give it weights."""
    return CLIPVisionTransformer(input_resolution=224, patch_size=32, width=768, layers=12, heads=12, output_dim=512, dtype=dtype, **kwargs)


def _from_transformers(sd: dict) -> dict:
    """transformers' CLIPVisionModelWithProjection names -> OpenAI's `visual` names (q / k / v concatenated, visual_projection transposed)."""
    p = "vision_model."
    out = {"class_embedding": sd[p + "embeddings.class_embedding"], "positional_embedding": sd[p + "embeddings.position_embedding.weight"],
           "conv1.weight": sd[p + "embeddings.patch_embedding.weight"], "proj": sd["visual_projection.weight"].t().contiguous()}
    for a, b in (("pre_layrnorm", "ln_pre"), ("post_layernorm", "ln_post")):
        for n in ("weight", "bias"):
            out[f"{b}.{n}"] = sd[f"{p}{a}.{n}"]
    names = {"layer_norm1": "ln_1", "layer_norm2": "ln_2", "self_attn.out_proj": "attn.out_proj", "mlp.fc1": "mlp.c_fc", "mlp.fc2": "mlp.c_proj"}
    i = 0
    while f"{p}encoder.layers.{i}.layer_norm1.weight" in sd:
        src, dst = f"{p}encoder.layers.{i}.", f"transformer.resblocks.{i}."
        for a, b in names.items():
            for n in ("weight", "bias"):
                out[f"{dst}{b}.{n}"] = sd[f"{src}{a}.{n}"]
        for n, o in (("weight", "in_proj_weight"), ("bias", "in_proj_bias")):
            out[dst + "attn." + o] = torch.cat([sd[f"{src}self_attn.{q}_proj.{n}"] for q in ("q", "k", "v")], 0)
        i += 1
    known = set(p + k for k in ("embeddings.class_embedding", "embeddings.position_embedding.weight", "embeddings.patch_embedding.weight",
                                "embeddings.position_ids", "pre_layrnorm.weight", "pre_layrnorm.bias", "post_layernorm.weight",
                                "post_layernorm.bias")) | {"visual_projection.weight"}
    extra = [k for k in sd if k not in known and not k.startswith(p + "encoder.layers.")]
    for k in extra:                                    # strict: a key this map does not know surfaces in load_state_dict
        out[k] = sd[k]
    return out


def load_clip_state_dict(model: CLIPVisionTransformer, sd: dict) -> CLIPVisionTransformer:
    """Load (strictly, after mapping) one of: OpenAI's `model.visual` state dict; a full CLIP state dict (the `visual.*` keys are taken, the
    text tower ignored); a transformers CLIPVisionModelWithProjection state dict."""
    if "visual_projection.weight" in sd:
        sd = _from_transformers(sd)
    elif any(k.startswith("visual.") for k in sd):
        sd = {k[len("visual."):]: v for k, v in sd.items() if k.startswith("visual.")}
    model.load_state_dict({k: v.float() if v.is_floating_point() else v for k, v in sd.items()}, strict=True)
    return model
