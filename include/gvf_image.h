/*
 * gvf_image.h -- C ABI of the frame post-process of the path's caller side: 8-bit separable resampling with placement
 * into a fixed canvas.
 *
 * Replaces, per rendered frame, the host round trip of utils/inference_utils.py:276-297 (render_and_save_images):
 *     rgb.cpu() -> uint8 -> PIL Image.resize((target, target), LANCZOS) -> paste into a white 512x512 canvas or
 *     centre-crop to 512x512 -> PNG
 * with device-side passes over the uint8 frames the rasteriser driver already produces (gvf_rgb_to_u8, gvf_rast.h), so that
 * only finished 512x512 frames cross PCIe.  The arithmetic is Pillow's 8-bit-per-channel resampler (third-party, not under
 * /root/reference; src/libImaging/Resample.c: precompute_coeffs, normalize_coeffs_8bpc, ImagingResampleHorizontal_8bpc /
 * Vertical_8bpc): per output sample an int32 accumulation  (1 << 21) + sum_k in[first + k] * coef[k]  followed by
 * >> 22 and a clamp to 0..255; horizontal pass first, its uint8 result feeding the vertical pass.  The coefficient tables
 * (22-bit fixed point, any filter) are computed by the host in double precision and handed over; restated in
 * oracle/resize_ref.py and checked bit-exactly against Pillow itself in the tests.
 * Conventions as in gvf_rast.h (device pointers, explicit stream, int status, caller-owned buffers).
 */
#ifndef GVF_IMAGE_H
#define GVF_IMAGE_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GVF_RESAMPLE_PRECISION_BITS 22   /* 32 - 8 - 2, Pillow's PRECISION_BITS */
#define GVF_RESAMPLE_MAX_TAPS       256
#define GVF_RESAMPLE_MAX_WIDTH      16384

/* One separable pass table for `n_out` output samples: first[n_out] = index of the first input sample, count[n_out] = taps
 * used (<= ksize), coef[ksize][n_out] int32 fixed point (tap-major, so that neighbouring outputs read neighbouring words);
 * taps beyond count are zero. */
typedef struct GvfResampleTable {
    const int32_t* first;
    const int32_t* count;
    const int32_t* coef;
    int32_t ksize;
    int32_t n_out;
} GvfResampleTable;

/* src: planes x in_h x in_w uint8 (planes = frames x channels).  Horizontal pass with `tab_h` (n_out = mid_w) into
 * tmp (planes x in_h rows of pitch (mid_w + 3) & ~3 bytes; may be null when tab_h is null = no horizontal resampling,
 * mid_w = in_w), vertical pass with
 * `tab_v` (n_out = mid_h; null = none, mid_h = in_h), written into dst (planes x dst_h x dst_w) with the resampled image's
 * top-left corner at (off_y, off_x) -- negative offsets crop, uncovered canvas pixels take pad_value. */
int gvf_resample_place_u8(const uint8_t* src, int64_t planes, int in_h, int in_w, const GvfResampleTable* tab_h,
                          const GvfResampleTable* tab_v, uint8_t* tmp, uint8_t* dst, int dst_h, int dst_w, int off_y, int off_x,
                          int pad_value, void* stream);

/*
 * RGBA condition preprocessing: what the reference does per frame on the host, in front of the image encoder, with Pillow and
 * numpy -- trellis/pipelines/trellis_image_to_3d.py:85-119 (preprocess_image), scripts/encode_in_the_wild_img_cond_dinov2_feature.py
 * :27-66, 86-110 (remove_background and the later frames) and scripts/encode_img_cond_dinov2_feature.py:40-44.
 * `img.crop(box).resize((W, H), LANCZOS)` on an RGBA image is not four plane resizes.  Pillow (third-party, restated here, not
 * transcribed) converts to premultiplied RGBa, resamples all four bands with the 8-bit resampler above, and converts back:
 *     premultiply     t = c * a + 128;  p = ((t >> 8) + t) >> 8          (alpha unchanged)
 *     un-premultiply  a == 0 or a == 255: p;  otherwise min(255, (255 * p) / a), the division truncating
 * Crop pixels outside the image read (0, 0, 0, 0).  When the crop already has the output size Pillow returns a copy and neither
 * conversion runs (the round trip is lossy); when one axis has it, that pass alone is skipped.
 */
#define GVF_RGBA_OUT_RGBA  0   /* dst uint8 [n][dst_h][dst_w][4]: the resized RGBA image itself */
#define GVF_RGBA_OUT_BLACK 1   /* dst uint8 [n][dst_h][dst_w][3]: uint8(((c / 255f) * (a / 255f)) * 255f), fp32 throughout */
#define GVF_RGBA_OUT_WHITE 2   /* dst uint8 [n][dst_h][dst_w][3]: w = (c / 255f) * (a / 255f) + (1f - a / 255f) * 1f in fp32 without
                                  contraction, uint8((double)w * 255.0); mask (may be null) uint8 [n][dst_h][dst_w]:
                                  uint8((double)(a / 255f) * 255.0), 0 where the canvas is uncovered */
#define GVF_RGBA_OUT_F32   3   /* dst float [n][3][dst_h][dst_w]: (c / 255f) * (a / 255f), not rounded to 8 bit; pad_value / 255f */

/* rgba: n x h x w x 4 interleaved, 4-byte aligned.  out: n x int32[5] = xmin, ymin, xmax, ymax over the pixels with
 * alpha > threshold -- (w, h, -1, -1) when there is none -- and the smallest alpha of the image.  n <= 65535. */
int gvf_alpha_bbox_u8(const uint8_t* rgba, int64_t n, int h, int w, int threshold, int32_t* out, void* stream);

/* src: n x in_h x in_w x 4 interleaved RGBA, 4-byte aligned.  The crop window crop_w x crop_h has its top-left corner at
 * (crop_x, crop_y) of the image and may stick out on any side.  tab_h (crop_w -> n_out = out_w) and tab_v (crop_h -> out_h) as for
 * gvf_resample_place_u8; a null table skips that pass, both null is Pillow's copy without conversions.  tmp: n * crop_h * out_w * 4
 * bytes, 4-byte aligned (may be null when both tables are).  The result is written in `mode` into a dst_h x dst_w canvas with its
 * top-left corner at (off_y, off_x); negative offsets crop, uncovered canvas pixels take pad_value in every channel.  One window
 * for all n images; n <= 65535; every extent within GVF_RESAMPLE_MAX_WIDTH, every table within GVF_RESAMPLE_MAX_TAPS. */
int gvf_rgba_resample_u8(const uint8_t* src, int64_t n, int in_h, int in_w, int crop_x, int crop_y, int crop_w, int crop_h,
                         const GvfResampleTable* tab_h, const GvfResampleTable* tab_v, uint8_t* tmp, int mode, void* dst, uint8_t* mask,
                         int dst_h, int dst_w, int off_y, int off_x, int pad_value, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* GVF_IMAGE_H */
