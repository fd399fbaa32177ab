/*
 * gvf_clip.h -- C ABI of the MI355X (gfx950) kernels in front of and behind the blocks of CLIP's ViT-B/32 image tower (csrc/clip.hip): the
 * 32 x 32 patch convolution with the token assembly, ln_pre, and the read-out ln_post(cls) @ proj -> unit vector -> cosine.  The blocks run
 * on the entry points of gvf_dit.h (gvf_gemm_ln, gvf_attn_fwd, gvf_gemm_resid_stats; GVF_EPI_QUICK_GELU_16 is the MLP's activation).
 *
 * Reference seam: utils/inference_utils.py:37-178 (align_gaussian_to_canonical) scores a view with 0.2 * (1 - cos(encode_image(a),
 * encode_image(b))) of clip.load("ViT-B/32"); the model's source is not part of the reference, so this restates the public architecture.
 * Conventions as in gvf_dit.h: device pointers, caller-owned buffers, explicit stream, int status, `dtype` = GVF_DT_BF16 / GVF_DT_F16.
 * No atomics anywhere: the same bits every run, and an image's bits do not depend on its position in the batch.
 */
#ifndef GVF_CLIP_H
#define GVF_CLIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GVF_CLIP_PATCH 32             /* patch side */
#define GVF_CLIP_PATCH_K 3072         /* 3 * 32 * 32 contraction depth of the patch convolution: 96 MFMA k-steps of 32 */

#define GVF_CLIP_IN_U8 0              /* img uint8 [B][3][S][S]; the operand is lut[c][img] */
#define GVF_CLIP_IN_F32 1             /* img fp32  [B][3][S][S], normalised already; the operand is r16(img) */

/* packed [D][3072] 16-bit <- w fp32 [D][3][32][32] (conv1.weight as stored: k = c * 1024 + dy * 32 + dx), rounded to nearest even once.
 * packed 16-byte aligned. */
int gvf_clip_pack_patch_weight(int dtype, const float* w, int D, void* packed, void* stream);

/* The 32 x 32 stride-32 convolution 3 -> D (no bias) as an implicit GEMM on v_mfma_f32_16x16x32, with the token assembly in its epilogue.
 *   img:   in_kind GVF_CLIP_IN_U8: uint8 pixels, and lut 16-bit [3][256] (device) holds the operand of every (channel, pixel value) -- the host
 *          computes (u8 / 255 - mean[c]) / std[c] in fp32 and rounds once, which for fp16 is what ToTensor -> Normalize -> .half() feeds conv1;
 *          in_kind GVF_CLIP_IN_F32: fp32 pixels, normalised by the caller, rounded once to the operand type; lut is ignored.
 *          S a multiple of 32 with (S / 32)^2 == n_patches, the grid `pos` was stored for; img 16-byte aligned.
 *   x:     the fp32 token stream [B][1 + n_patches][D]:
 *            row 0       = cls[d] + pos[0][d]                    (one fp32 add)
 *            row 1 + i   = acc_i[d] + pos[1 + i][d]              (fp32 accumulation over the 96 k-steps in ascending k, one fp32 add)
 * cls fp32 [D], pos fp32 [1 + n_patches][D].  D a multiple of 128.  Anything else is GVF_EINVAL with nothing launched. */
int gvf_clip_patch_embed(int dtype, int in_kind, const void* img, const void* lut, int B, int S, const void* w_packed, const float* cls,
                         const float* pos, int n_patches, int D, float* x, void* stream);

/* In-place LayerNorm of `rows` fp32 rows of D (ln_pre; also usable on any fp32 stream): x = LN(x) * ln_w + ln_b, a wave per row, all in fp32:
 * mean = sum / D, variance from the centred values, sums in gvf_wave_sum_dpp's fixed order.  stats (may be NULL): per row, D / 64 partial
 * (sum, sum of squares) pairs of the row AS WRITTEN, one per 64-column slice -- gvf_gemm_stats_parts(D) of them, the layout
 * gvf_gemm_resid_stats writes -- so that block 0's ln_1 goes through gvf_gemm_ln.  D a multiple of 128, <= 1024; x, ln_w, ln_b 16-byte
 * aligned, stats 8-byte aligned. */
int gvf_clip_ln_rows(float* x, long long rows, int D, float eps, const float* ln_w, const float* ln_b, float* stats, void* stream);

/* The read-out, a workgroup per image.  x fp32 [B][L][D]: row 0 of every image is read.
 *   h = r16(LN(x0) * ln_w + ln_b)                (fp32 LayerNorm as in gvf_clip_ln_rows, one rounding)
 *   f = r16(sum_d h[d] * proj[d][e])             (proj 16-bit [D][E]; one fp32 fma chain per column, ascending d)
 *   feat [B][E] fp32 = f;  unit [B][E] fp32 = f / sqrt(sum_e f^2)     (fp32; the sum in a fixed order)
 *   sim  [B]    fp32 = sum_e unit[e] * g[e]      (only with g fp32 [E], a reference unit vector; sim may be NULL when g is)
 * A zero f makes unit and sim NaN (0 / 0), as IEEE and the reference do.  E a multiple of 64, <= 1024; D a multiple of 128, <= 1024. */
int gvf_clip_head(int dtype, const float* x, int B, int L, int D, float eps, const float* ln_w, const float* ln_b, const void* proj, int E,
                  const float* g, float* feat, float* unit, float* sim, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* GVF_CLIP_H */
