/*
 * gvf_loss.h -- C ABI of the fused image loss of the render-loss training step:
 *
 *     loss = w_l1 * mean|pred - gt| + w_ssim * (1 - mean SSIM(pred, gt))
 *
 * the reference's motion-VAE render loss without its LPIPS term (train_vae.py:328-334; SSIM as utils/loss_util.py:ssim).
 *
 * Layout: pred, gt are fp32, dense, planes x H x W (planes = N * C); every plane is independent (the reference's
 * groups = channel convolution).  n = planes * H * W.
 *
 * SSIM (utils/loss_util.py:_ssim): per plane, G = the 11 x 11 Gaussian window with sigma 1.5 (the fp32-normalised 1-D taps,
 * applied separably: a horizontal 11-tap pass, then a vertical one), zero padding 5 (as conv2d(padding=5); border means
 * are not renormalised):
 *     mu1 = G*p, mu2 = G*g, s1 = G*(p p) - mu1^2, s2 = G*(g g) - mu2^2, s12 = G*(p g) - mu1 mu2
 *     S   = (2 mu1 mu2 + C1)(2 s12 + C2) / ((mu1^2 + mu2^2 + C1)(s1 + s2 + C2)),   C1 = 0.01^2, C2 = 0.03^2
 *     mean SSIM = sum S / n.
 *
 * Gradient (design: the forward saves three per-pixel partial-derivative maps, the backward applies the window to them):
 *     d(mean SSIM)/dp = (G*a + 2 p G*b + g G*c) / n,
 *     a = dS/dmu1 - 2 mu1 b - mu2 c (the total derivative in G*p),  b = dS/ds1,  c = dS/ds12,
 * and d(mean L1)/dp = sign(p - g) / n with sign(0) = 0.
 *
 * Determinism: the loss is reduced per workgroup in double and the partials are summed in a fixed order by one workgroup;
 * no float atomics, so the result is bit-identical run to run and independent of the stream.
 *
 * Conventions as in gvf_rast.h: device pointers, an explicit stream (null = the default stream), an int status (GVF_OK or a
 * negative GVF_E*), caller-owned buffers.  Arguments are checked on the host before any launch.
 */
#ifndef GVF_LOSS_H
#define GVF_LOSS_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GVF_SSIM_WINDOW 11

/* flags: the forward keeps the SSIM partial maps in the scratch for gvf_image_loss_backward (3 x n fp32).  Without it the
 * forward writes no per-pixel output and the backward computes the L1 part of the gradient only. */
#define GVF_IMAGE_LOSS_SSIM_GRAD 1

/* The 11 fp32 taps of the 1-D window the kernels apply (utils/loss_util.py:gaussian(11, 1.5)) into taps[11] (host memory). */
int gvf_ssim_window(float* taps);

/* Scratch size for one forward (+ backward) over planes x H x W with `flags`.  GVF_EINVAL for planes, H or W <= 0, a null
 * `out`, unknown flags or a size that does not fit. */
int gvf_image_loss_scratch_bytes(int64_t planes, int H, int W, int flags, size_t* out);

/* terms_out (device, 3 fp32): [loss, mean L1, mean SSIM], loss = w_l1 * mean L1 + w_ssim * (1 - mean SSIM).
 * scratch: >= gvf_image_loss_scratch_bytes(planes, H, W, flags) bytes (GVF_ENOSPC otherwise); with
 * GVF_IMAGE_LOSS_SSIM_GRAD it holds the partial maps for the backward afterwards. */
int gvf_image_loss_forward(const float* pred, const float* gt, int64_t planes, int H, int W, float w_l1, float w_ssim,
                           float* terms_out, void* scratch, size_t scratch_bytes, int flags, void* stream);

/* grad_pred (device, planes x H x W) = d(t . terms)/d pred for the device vector t = grad_terms[3] (the incoming gradients
 * of loss, mean L1 and mean SSIM; read on the device, so no host synchronisation):
 *     grad = ((t0 w_l1 + t1) / n) sign(p - g) + ((t2 - t0 w_ssim) / n) (G*a + 2 p G*b + g G*c)
 * The SSIM part needs GVF_IMAGE_LOSS_SSIM_GRAD and the scratch of the forward on the same pred, gt; without the flag it is
 * left out (the caller states that its coefficient is zero). */
int gvf_image_loss_backward(const float* pred, const float* gt, int64_t planes, int H, int W, float w_l1, float w_ssim,
                            const float* grad_terms, float* grad_pred, const void* scratch, size_t scratch_bytes, int flags,
                            void* stream);

#ifdef __cplusplus
}
#endif
#endif /* GVF_LOSS_H */
