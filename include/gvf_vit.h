/*
 * gvf_vit.h -- C ABI of the MI355X (gfx950) kernels in front of and behind the DINOv2 ViT blocks (csrc/vit.hip): the patch embedding with
 * the token assembly, and the read-out of the token stream.  The blocks themselves run on the entry points of gvf_dit.h (gvf_gemm_ln,
 * gvf_attn_fwd, gvf_gemm_resid_stats; GVF_EPI_GELU_ERF_16 is the MLP's exact-erf GELU).
 *
 * Reference seams (the model comes through torch.hub there; this restates the public architecture):
 *   trellis/pipelines/trellis_image_to_3d.py:73-83, 121-146   transforms.Normalize + dinov2_vitl14_reg(..., is_training=True)['x_prenorm'] + F.layer_norm
 *   scripts/encode_img_cond_dinov2_feature.py:36-64           x_prenorm[:, R+1:] with the cls token appended last (or x_norm_* with --normalize), fp16
 * Conventions as in gvf_dit.h: device pointers, caller-owned buffers, explicit stream, int status, `dtype` = GVF_DT_BF16 / GVF_DT_F16.
 */
#ifndef GVF_VIT_H
#define GVF_VIT_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GVF_VIT_PATCH 14              /* patch side */
#define GVF_VIT_PATCH_K 588           /* 3 * 14 * 14 contraction depth of the patch convolution ... */
#define GVF_VIT_PATCH_KPAD 608        /* ... zero-padded to 19 MFMA k-steps of 32 */

/* packed [D][608] 16-bit <- w fp32 [D][3][14][14] (the Conv2d weight as stored: k = c * 196 + dy * 14 + dx), rounded to nearest even once,
 * columns 588 .. 607 zero. */
int gvf_vit_pack_patch_weight(int dtype, const float* w, int D, void* packed, void* stream);

/* The 14 x 14 stride-14 convolution 3 -> D as an implicit GEMM on v_mfma_f32_16x16x32, with the token assembly in its epilogue.
 *   img:   fp32 [B][3][H][W], values in [0, 1]; the operand is r16((img - mean[c]) / std[c]) -- fp32 subtract, fp32 divide, ONE rounding to
 *          16 bits; mean / std: HOST arrays of 3 floats.  H, W multiples of 14 with (H / 14) * (W / 14) == n_patches, the grid `pos` was
 *          stored for; img 8-byte aligned.
 *   x:     the fp32 token stream [B][1 + R + n_patches][D] in the model's order:
 *            row 0            = cls[d] + pos[0][d]                              (one fp32 add)
 *            rows 1 .. R      = reg[r][d]                                       (no position term)
 *            row 1 + R + i    = (acc_i[d] + bias[d]) + pos[1 + i][d]            (fp32 accumulation over ascending k-steps, two fp32 adds)
 *   stats: per row of x, D / 64 partial (sum, sum of squares) pairs, one per 64-column slice -- gvf_gemm_stats_parts(D) of them, the layout
 *          gvf_gemm_resid_stats writes -- so that the first block's norm1 goes through gvf_gemm_ln.  May be NULL.
 * pos fp32 [1 + n_patches][D], cls fp32 [D], reg fp32 [R][D] (NULL when R == 0), bias fp32 [D] or NULL.  D a multiple of 128, R >= 0.
 * A token's bits do not depend on its position in the batch.  Anything else is GVF_EINVAL with nothing launched. */
int gvf_vit_patch_embed(int dtype, const float* img, int B, int H, int W, const float* mean, const float* std, const void* w_packed,
                        const float* bias, const float* cls, const float* reg, int R, const float* pos, int n_patches, int D, float* x,
                        float* stats, void* stream);

/* The read-out of the stream x fp32 [B][1 + R + n][D] (x_prenorm) in one launch, a wave per output row.
 *   mode:  GVF_VIT_OUT_COPY; GVF_VIT_OUT_LN_AFFINE = LayerNorm(x) * ln_w + ln_b (norm.weight / bias, eps 1e-6: x_norm);
 *          GVF_VIT_OUT_LN = LayerNorm without affine terms (eps 1e-5: F.layer_norm(x, x.shape[-1:]), the TRELLIS condition).
 *   order: GVF_VIT_ORDER_STORED = the 1 + R + n rows as stored; GVF_VIT_ORDER_PATCHES_CLS = the n patch rows, then the cls row (n + 1 rows,
 *          registers dropped: the 1370-token layout of the DiT's cond_images).
 *   out:   [B][rows][D] fp32 (out_f16 == 0) or IEEE fp16 (out_f16 != 0), contiguous.
 * LayerNorm in fp32: mean = sum / D, variance from the centred values (two passes over registers), sums by gvf_wave_sum_dpp's fixed
 * order: the same bits every run and at every batch position.  D a multiple of 4, <= 1024; x and out 16-byte aligned. */
#define GVF_VIT_OUT_COPY 0
#define GVF_VIT_OUT_LN_AFFINE 1
#define GVF_VIT_OUT_LN 2
#define GVF_VIT_ORDER_STORED 0
#define GVF_VIT_ORDER_PATCHES_CLS 1
int gvf_vit_tokens_out(const float* x, int B, int R, int n_patches, int D, int mode, float eps, const float* ln_w, const float* ln_b,
                       int order, int out_f16, void* out, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* GVF_VIT_H */
