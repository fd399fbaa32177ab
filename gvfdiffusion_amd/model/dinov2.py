"""DINOv2 ViT (with or without register tokens) for inference on the MI355X: pixels -> the token dict the reference reads.

The reference takes the model from torch.hub (`dinov2_vitl14_reg`, trellis/pipelines/trellis_image_to_3d.py:73-83;
scripts/encode_img_cond_dinov2_feature.py:36-64); its source is not part of the reference, so this is a restatement of the public architecture:
    x = [cls + pos[0] | registers | conv14(z-score(img)) + pos[1:]]
    per block:  x += ls1 * proj(attn(norm1 x));  x += ls2 * fc2(gelu_erf(fc1(norm2 x)))        (LayerNorm eps 1e-6, heads of 64)
    x_prenorm = x;  x_norm = norm(x)
The parameters carry the hub checkpoint's state-dict names (written from memory of the public checkpoint: unpinned), so a
released state dict loads with strict=True.  No weights are fetched here: the factories build the architecture with its initial values.

Every operation between the pixels and the tokens is a launch of the HIP library: ops.vit.patch_embed (which also writes the LayerNorm
statistics of block 0's norm1), then five launches per block -- gvf_gemm_ln (qkv), gvf_attn_fwd, gvf_gemm_resid_stats (proj, gate = ls1.gamma),
gvf_gemm_ln (fc1 with the exact-erf GELU epilogue), gvf_gemm_resid_stats (fc2, gate = ls2.gamma) -- and ops.vit.tokens_out.  The residual
stream is fp32, the matrix operands fp16 or bf16 (`dtype`).  There is no torch fall-back."""
import torch
import torch.nn as nn

from .. import _lib
from ..ops import dit_ops, vit as vit_ops

__all__ = ["DinoVisionTransformer", "dinov2_vitl14_reg", "dinov2_vitl14"]

HEAD_DIM = 64


class _LayerScale(nn.Module):
    def __init__(self, dim, init_values):
        super().__init__()
        self.gamma = nn.Parameter(init_values * torch.ones(dim))


class _Attention(nn.Module):
    def __init__(self, dim):
        super().__init__()
        self.qkv = nn.Linear(dim, 3 * dim)
        self.proj = nn.Linear(dim, dim)


class _Mlp(nn.Module):
    def __init__(self, dim, hidden):
        super().__init__()
        self.fc1 = nn.Linear(dim, hidden)
        self.fc2 = nn.Linear(hidden, dim)


class _Block(nn.Module):
    def __init__(self, dim, hidden, init_values):
        super().__init__()
        self.norm1 = nn.LayerNorm(dim, eps=1e-6)
        self.attn = _Attention(dim)
        self.ls1 = _LayerScale(dim, init_values)
        self.norm2 = nn.LayerNorm(dim, eps=1e-6)
        self.mlp = _Mlp(dim, hidden)
        self.ls2 = _LayerScale(dim, init_values)


class _PatchEmbed(nn.Module):
    def __init__(self, patch_size, dim):
        super().__init__()
        self.proj = nn.Conv2d(3, dim, kernel_size=patch_size, stride=patch_size)


class DinoVisionTransformer(nn.Module):
    def __init__(self, img_size: int = 518, patch_size: int = 14, embed_dim: int = 1024, depth: int = 24, num_heads: int = 16,
                 mlp_ratio: float = 4.0, num_register_tokens: int = 0, init_values: float = 1.0, ffn_layer: str = "mlp",
                 drop_path_rate: float = 0.0, dtype=torch.float16):
        super().__init__()
        if ffn_layer != "mlp":
            raise NotImplementedError(f"ffn_layer={ffn_layer!r} is not built: the SwiGLU feed-forward of the giant model has no kernel here")
        if drop_path_rate != 0.0:
            raise NotImplementedError("drop_path is not built: the encoder is inference only")
        if init_values is None:
            raise NotImplementedError("a model without LayerScale is not built: the released checkpoints all carry ls1 / ls2")
        if patch_size != vit_ops.PATCH:
            raise NotImplementedError(f"patch_size={patch_size} is not built: the patch-embedding kernel is the 14 x 14 one")
        if img_size % patch_size != 0:
            raise ValueError("img_size must be a multiple of the patch size")
        if embed_dim % 128 != 0 or embed_dim > 1024 or embed_dim != num_heads * HEAD_DIM:
            raise NotImplementedError(f"embed_dim={embed_dim}, num_heads={num_heads} is not built: heads of 64, width a multiple of 128 up to 1024 "
                                      "(the LayerNorm-folded GEMM stages K <= 1024)")
        if dtype not in dit_ops.LP_DTYPES:
            raise ValueError("dtype must be torch.float16 or torch.bfloat16")
        hidden = int(embed_dim * mlp_ratio)
        if hidden % 32 != 0:
            raise NotImplementedError(f"mlp_ratio={mlp_ratio} is not built: the hidden width must be a multiple of 32")
        self.img_size, self.patch_size, self.embed_dim, self.num_heads = img_size, patch_size, embed_dim, num_heads
        self.num_register_tokens = num_register_tokens
        self.num_patches = (img_size // patch_size) ** 2
        self.lp = dtype
        # the z-score in front of the model (the reference's transforms.Normalize) runs inside the patch kernel; a caller whose pixels are
        # normalised already sets mean (0, 0, 0) and std (1, 1, 1), which the kernel's (x - 0) / 1 passes through exactly
        self.image_mean, self.image_std = vit_ops.IMAGENET_MEAN, vit_ops.IMAGENET_STD
        self.cls_token = nn.Parameter(torch.zeros(1, 1, embed_dim))
        self.pos_embed = nn.Parameter(torch.zeros(1, 1 + self.num_patches, embed_dim))
        if num_register_tokens:                       # (the checkpoints without registers have no such key)
            self.register_tokens = nn.Parameter(torch.zeros(1, num_register_tokens, embed_dim))
        else:
            self.register_tokens = None
        self.mask_token = nn.Parameter(torch.zeros(1, embed_dim))
        self.patch_embed = _PatchEmbed(patch_size, embed_dim)
        self.blocks = nn.ModuleList([_Block(embed_dim, hidden, init_values) for _ in range(depth)])
        self.norm = nn.LayerNorm(embed_dim, eps=1e-6)
        nn.init.trunc_normal_(self.pos_embed, std=0.02)
        nn.init.normal_(self.cls_token, std=1e-6)
        if num_register_tokens:
            nn.init.normal_(self.register_tokens, std=1e-6)
        self._images = None                            # the 16-bit weight images, built once per load (key: device, dtype, parameter versions)
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
            raise NotImplementedError("training is not built: the DINOv2 encoder is inference only")
        return super().train(False)

    def weight_images(self):
        dev = self.cls_token.device
        key = (dev, self.lp)
        if self._images is not None and self._images["key"] == key:
            return self._images
        f32 = lambda p: p.detach().float().contiguous()
        lp = lambda p: p.detach().to(self.lp).contiguous()
        D = self.embed_dim
        im = {"key": key,
              "patch_w": vit_ops.pack_patch_weight(f32(self.patch_embed.proj.weight), self.lp), "patch_b": f32(self.patch_embed.proj.bias),
              "cls": f32(self.cls_token).reshape(D), "pos": f32(self.pos_embed).reshape(-1, D),
              "reg": None if self.register_tokens is None else f32(self.register_tokens).reshape(-1, D),
              "norm": (f32(self.norm.weight), f32(self.norm.bias)), "blocks": []}
        for b in self.blocks:
            im["blocks"].append({
                "n1": (f32(b.norm1.weight), f32(b.norm1.bias)), "qkv": (lp(b.attn.qkv.weight), f32(b.attn.qkv.bias)),
                "proj": (lp(b.attn.proj.weight), f32(b.attn.proj.bias)), "ls1": f32(b.ls1.gamma),
                "n2": (f32(b.norm2.weight), f32(b.norm2.bias)), "fc1": (lp(b.mlp.fc1.weight), f32(b.mlp.fc1.bias)),
                "fc2": (lp(b.mlp.fc2.weight), f32(b.mlp.fc2.bias)), "ls2": f32(b.ls2.gamma)})
        self._images = im
        return im

    # ---- forward -----------------------------------------------------------------------------------------------------------------------
    @torch.no_grad()
    def forward_stream(self, image01: torch.Tensor) -> torch.Tensor:
        """image01 fp32 (B, 3, S, S) in [0, 1] (the z-score is inside the patch kernel) -> x_prenorm fp32 (B, 1 + R + n, D)."""
        _lib.require_cuda(image01)
        if image01.dim() != 4 or image01.shape[1] != 3 or image01.dtype != torch.float32:
            raise _lib.GvfError(f"the encoder takes an fp32 (B, 3, H, W) image, got {image01.dtype} {tuple(image01.shape)}")
        if image01.device != self.cls_token.device:
            raise _lib.GvfError("image and model are on different devices")
        im = self.weight_images()
        D, H = self.embed_dim, self.num_heads
        x3, stats = vit_ops.patch_embed(image01, im["patch_w"], im["patch_b"], im["cls"], im["reg"], im["pos"], self.image_mean, self.image_std)
        B, L, _ = x3.shape
        M = B * L
        x = x3.view(M, D)
        n_part = dit_ops.gemm_stats_parts(D)
        dev = x.device
        qkv = torch.empty((M, 3 * D), dtype=self.lp, device=dev)
        ab = torch.empty((M, D), dtype=self.lp, device=dev)
        hidden = torch.empty((M, self.blocks[0].mlp.fc1.out_features), dtype=self.lp, device=dev) if len(self.blocks) else None
        s_qkv, s_o = (L * 3 * D, 0, 3 * D), (L * D, 0, D)
        for b in im["blocks"]:
            dit_ops.gemm_ln_bf16(x, stats, n_part, b["qkv"][0], b["qkv"][1], qkv, dit_ops.EPI_STORE_16, eps=1e-6, ln_w=b["n1"][0], ln_b=b["n1"][1])
            dit_ops.attention(qkv, qkv[:, D:], qkv[:, 2 * D:], ab, B, 1, L, L, H, s_qkv, s_qkv, s_qkv, s_o, head_dim=HEAD_DIM)
            # LayerScale = the gate of the residual epilogue, one row group over all M rows
            dit_ops.gemm_resid_stats(ab, b["proj"][0], b["proj"][1], x, stats, gate=b["ls1"], gate_ld=D, rows_per_group=M)
            dit_ops.gemm_ln_bf16(x, stats, n_part, b["fc1"][0], b["fc1"][1], hidden, dit_ops.EPI_GELU_ERF_16, eps=1e-6, ln_w=b["n2"][0], ln_b=b["n2"][1])
            dit_ops.gemm_resid_stats(hidden, b["fc2"][0], b["fc2"][1], x, stats, gate=b["ls2"], gate_ld=D, rows_per_group=M)
        return x3

    @torch.no_grad()
    def forward(self, x: torch.Tensor, masks=None, is_training: bool = True):
        """x: fp32 (B, 3, S, S) in [0, 1].  The ImageNet z-score the reference applies in front of the model (transforms.Normalize) is folded
        into the patch kernel (image_mean / image_std), so the caller passes the un-normalised image.  is_training=True returns the dict the reference reads
        (x_norm_clstoken, x_norm_regtokens, x_norm_patchtokens, x_prenorm, masks); otherwise the cls feature, as the hub model's head-less
        forward does."""
        if masks is not None:
            raise NotImplementedError("masked patches are not built (mask_token is carried for the checkpoint's sake only)")
        xp = self.forward_stream(x)
        R = self.num_register_tokens
        im = self.weight_images()
        xn = vit_ops.tokens_out(xp, R, vit_ops.OUT_LN_AFFINE, vit_ops.ORDER_STORED, torch.float32, im["norm"][0], im["norm"][1], eps=1e-6)
        if not is_training:
            return xn[:, 0]
        return {"x_norm_clstoken": xn[:, 0], "x_norm_regtokens": xn[:, 1:R + 1], "x_norm_patchtokens": xn[:, R + 1:], "x_prenorm": xp, "masks": None}


def dinov2_vitl14_reg(dtype=torch.float16, **kwargs) -> DinoVisionTransformer:
    """ViT-L/14 with 4 register tokens at 518 x 518 (37 x 37 patches): the architecture only -- load a state dict to give it weights."""
    return DinoVisionTransformer(img_size=518, patch_size=14, embed_dim=1024, depth=24, num_heads=16, mlp_ratio=4, num_register_tokens=4,
                                 init_values=1.0, dtype=dtype, **kwargs)


def dinov2_vitl14(dtype=torch.float16, **kwargs) -> DinoVisionTransformer:
    """ViT-L/14 without register tokens at 518 x 518."""
    return DinoVisionTransformer(img_size=518, patch_size=14, embed_dim=1024, depth=24, num_heads=16, mlp_ratio=4, num_register_tokens=0,
                                 init_values=1.0, dtype=dtype, **kwargs)
