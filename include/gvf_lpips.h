/*
 * gvf_lpips.h -- C ABI of the LPIPS (VGG16) term of the render loss (train_vae.py:328-334; utils/lpips/lpips.py, networks.py):
 * one entry point per layer, so that the operator (ops/lpips.py) composes them and every kernel can be tested alone.
 *
 *     x, y (N,3,H,W) fp32 in [-1,1]  ->  z-score  ->  VGG16 features[0:30]  ->  five taps (after the ReLU of convs 2, 4, 7, 10, 13)
 *     per tap: u = a / (sqrt(sum_c a^2) + 1e-10) for both images, sum_c lin_c (u_x - u_y)^2, mean over pixels
 *     loss = sum over taps and images / N;  the gradient flows to x only (frozen weights: no weight gradient anywhere).
 *
 * Layouts.  Activations are NHWC, 16-bit (`dtype`: GVF_DT_BF16 / GVF_DT_F16 of gvf_dit.h), dense: one tap's Cin is contiguous, so the
 * convolution stages a halo patch in LDS once and reads it nine times with shifted addresses.  The image and its gradient are fp32 NCHW.
 * Convolution weights are read from a packed 16-bit image (gvf_conv3x3_pack) in the operand order of v_mfma_f32_16x16x32.
 *
 * One kernel, two directions.  The gradient of a stride-1, pad-1 3x3 convolution with respect to its input is the same convolution with
 * the taps flipped and the channel roles swapped: gvf_conv3x3_pack(GVF_CONV_PACK_DGRAD) writes that image and gvf_conv3x3 runs it with
 * cin = the forward's Cout and cout = the forward's Cin.
 *
 * Operand types.  Forward activations and weights use `dtype`.  EVERY gradient tensor (g_pooled, tap_grad, z, the output of the tap
 * backward) and the DGRAD weight image are bf16 whatever the forward type: the gradients are ~1e-4 spread over thousands of pixels and
 * underflow in fp16, while bf16 has fp32's range.  There is no loss scale.
 *
 * Determinism: the tap forward reduces per workgroup in double and one workgroup adds the partials in a fixed order; no float atomics.
 *
 * Conventions as in gvf_loss.h: device pointers, an explicit stream (null = the default stream), an int status (GVF_OK or a negative
 * GVF_E*), caller-owned buffers.  Arguments are checked on the host before any launch.  Sizes: N, H, W >= 1 and N*H*W <= 2^31;
 * channel counts of the MFMA convolution are 64, 128, 256 or 512.
 */
#ifndef GVF_LPIPS_H
#define GVF_LPIPS_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GVF_CONV_PACK_FWD   0   /* image for out[co] = sum w[co][ci][ky][kx] in[y+ky-1][x+kx-1][ci]; cin = 3 allowed (the first layer, K = 27 padded to 32) */
#define GVF_CONV_PACK_DGRAD 1   /* image for the input gradient: rows = the forward's Cin, contraction over the forward's Cout, taps flipped */

#define GVF_CONV_RELU 1         /* flags of gvf_conv3x3: out = max(out, 0) after bias and addend, before the mask */

/* Bytes of the packed image of an fp32 [cout][cin][3][3] weight.  cout in {64,128,256,512}; cin in {64,128,256,512}, or 3 with
 * GVF_CONV_PACK_FWD (then cout must be 64). */
int gvf_conv3x3_packed_bytes(int cout, int cin, int mode, size_t* out);

/* w (device, fp32 [cout][cin][3][3], the FORWARD weight in both modes) -> out (device, >= packed_bytes, else GVF_ENOSPC), rounded to
 * `dtype`.  Weights are frozen: pack once per (module, dtype), never per step. */
int gvf_conv3x3_pack(const float* w, int cout, int cin, int mode, int dtype, void* out, size_t out_bytes, void* stream);

/* out (N,H,W,cout) = epilogue(conv3x3(in (N,H,W,cin), wimg)), stride 1, zero padding 1, fp32 accumulation, 9 cin / 32 MFMA k-steps:
 *     v = acc (+ bias[co], fp32, optional) (+ addend[n,y,x,co], 16-bit of `dtype`, optional);  GVF_CONV_RELU: v = max(v, 0);
 *     mask_src (optional, a stored 16-bit activation of the output's shape, either 16-bit type): v = mask_src > 0 ? v : 0.
 * cin, cout: the channel counts of THIS call (for a DGRAD image, the forward's Cout and Cin).  in, out, addend have type `dtype`. */
int gvf_conv3x3(const void* in, const void* wimg, const float* bias, const void* addend, const void* mask_src, void* out,
                int N, int H, int W, int cin, int cout, int flags, int dtype, void* stream);

/* First layer: x (N,3,H,W) fp32 -> out (N,H,W,64) 16-bit = relu(conv3x3(r16((x - mean[c]) / std[c])) + bias).  wimg: the
 * GVF_CONV_PACK_FWD image of the [64][3][3][3] weight; mean, std: device, 3 fp32 each. */
int gvf_lpips_first_forward(const float* x, const void* wimg, const float* bias, const float* mean, const float* std_, void* out,
                            int N, int H, int W, int dtype, void* stream);

/* First layer, input gradient: z (N,H,W,64) bf16 (the gradient at the first convolution's output, ReLU mask applied), w (device, fp32
 * [64][3][3][3], unpacked) -> dx (N,3,H,W) fp32 = (1 / std[c]) sum_{co,ky,kx} z[y+1-ky][x+1-kx][co] w[co][c][ky][kx]. */
int gvf_lpips_first_backward(const void* z, const float* w, const float* std_, float* dx, int N, int H, int W, void* stream);

/* 2x2 / stride 2 max pool (floor): in (N,H,W,C) -> out (N,H/2,W/2,C), 16-bit `dtype`.  H, W >= 2; C a multiple of 8. */
int gvf_maxpool2x2_forward(const void* in, void* out, int N, int H, int W, int C, int dtype, void* stream);

/* Pool backward fused with what surrounds it at a tap:
 *     z[i] = ([i is the argmax of its window] * g_pooled[window] + tap_grad[i]) * [a[i] > 0]
 * a (N,H,W,C) 16-bit `dtype` (the pooled activation, which is also the tap); g_pooled (N,H/2,W/2,C), tap_grad and z (N,H,W,C) bf16.
 * On a tie the first maximum in row-major window order wins; rows and columns the floor drops receive tap_grad only.  The sum is
 * one fp32 add, rounded to bf16. */
int gvf_maxpool2x2_backward(const void* a, const void* g_pooled, const void* tap_grad, void* z, int N, int H, int W, int C, int dtype,
                            void* stream);

/* Scratch of one tap forward (the per-workgroup double partials). */
int gvf_lpips_tap_scratch_bytes(int N, int H, int W, size_t* out);

/* terms_out[n] (device, N fp32) = (1 / (H W)) sum_pixels sum_c lin[c] (ax / (|ax| + 1e-10) - ay / (|ay| + 1e-10))^2 over the stored
 * activations ax, ay (N,H,W,C) 16-bit `dtype`; lin: device, C fp32.  C in {64,128,256,512}. */
int gvf_lpips_tap_forward(const void* ax, const void* ay, const float* lin, int N, int H, int W, int C, int dtype, float* terms_out,
                          void* scratch, size_t scratch_bytes, void* stream);

#define GVF_TAP_RELU_MASK 1     /* flags of gvf_lpips_tap_backward: grad = ax > 0 ? grad : 0 (the last tap, which no pool backward follows) */

/* grad_out (N,H,W,C) bf16 = upstream[n] * d terms[n] / d ax; upstream: device, N fp32 (the incoming gradient of every image's term), read
 * on the device (no host synchronisation).  With u = ax / D, D = |ax| + 1e-10, w_c = 2 upstream[n] lin_c (u_c - v_c) / (H W):  grad_k = (w_k - (ax_k / |ax|) sum_c w_c u_c) / D, where
 * ax_k / |ax| is 0 on a pixel whose activations are all zero (finite there; the ReLU mask downstream zeroes it). */
int gvf_lpips_tap_backward(const void* ax, const void* ay, const float* lin, const float* upstream, int N, int H, int W, int C, int dtype,
                           int flags, void* grad_out, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* GVF_LPIPS_H */
