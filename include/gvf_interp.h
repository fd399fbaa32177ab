/*
 * gvf_interp.h -- C ABI of the KNN interpolation ("deformation xyz") loss of the motion-VAE training step
 * (train_vae.py:486-586, compute_interpolation_loss_delta_interp) and of its core, the KNN-interpolated motion of a set of
 * query points (model/autoencoder.py compute_delta_interp).
 *
 * Inputs, all fp32 and dense: queries q (B, P, 3), anchors a (B, N, 3), moving anchors m (B, T, N, 3) (absolute positions),
 * len (B) int32 valid queries per sample (null: every sample has P; a value above P counts as P, a negative one as 0).
 *
 *  1. d_j = ((qx-ax)^2 + (qy-ay)^2) + (qz-az)^2, every operation rounded on its own (no fma contraction).
 *  2. The K smallest d_j, ascending; equal distances: the lower anchor index first.   1 <= K <= 16, K <= N.
 *  3. r = sqrt(mean_k d_k) + 1e-6, r2 = r r.  adaptive: w_k = exp(-beta d_k / r2) if d_k <= r2, else 0; otherwise
 *     w_k = exp(-beta d_k).  Then w_k /= (sum_k w_k + 1e-8).  Queries p >= len[b]: all weights 0 (idx 0, dist 0).
 *  4. est[b, t, p, :] = sum_k w_k (m[b, t, idx_k, :] - a[b, idx_k, :]), summed in neighbour order (the kernels form the differences,
 *     products and the sum in double and round the fp32 estimate once; the loss is taken against the unrounded sum).
 *  5. loss = sum_{b, t, p < len[b], c < 3} |pred - est| / (3 T sum_b len[b]);
 *     d loss / d pred = sign(pred - est) / (3 T sum_b len[b]), sign(0) = 0, zero for padded queries.
 *     With sum_b len[b] = 0 the loss and the gradient are 0 / 0 = NaN, as in the reference.
 *
 * pred and grad_pred are read / written through a row stride (in floats, >= 3): row (b, t, p) starts at
 * ((b T + t) P + p) * stride and its channels 0..2 are used, so a (B, T, P, 14) delta tensor is consumed in place.
 *
 * Design: the search keeps each query's running top K in registers (no (P, N)-sized intermediate); the loss forward fuses the
 * gather of rule 4 with the reduction and, on request, leaves one byte per (b, t, p) row with the three signs of pred - est,
 * from which the backward writes the gradient without touching pred, the anchors or the neighbour lists again.
 *
 * Determinism: the loss is reduced per workgroup in double and the partials are summed in a fixed order by one workgroup;
 * no float atomics, so the result is bit-identical run to run.  sum_b len[b] is formed on the device.
 *
 * Conventions as in gvf_loss.h: device pointers, an explicit stream (null = the default stream), an int status (GVF_OK or a
 * negative GVF_E*), caller-owned buffers.  Every argument is checked on the host before any launch: GVF_EINVAL for a null
 * required pointer, K < 1, K > 16, K > N, a non-positive size, a row stride < 3; GVF_ENOSPC for a short scratch.
 * Neighbour indices read from a caller's buffer are clamped to [0, N) before they address memory.
 */
#ifndef GVF_INTERP_H
#define GVF_INTERP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GVF_INTERP_MAX_K 16

/* Rules 1-3: idx (B, P, K) int32, w (B, P, K) fp32 and, if `dist` is not null, dist (B, P, K) fp32 (the squared distances). */
int gvf_knn_interp_weights(const float* q, const int32_t* len, const float* a, int B, int P, int N, int K, float beta, int adaptive,
                           int32_t* idx, float* w, float* dist, void* stream);

/* Rule 4: est (B, T, P, 3), dense. */
int gvf_knn_interp_apply(const int32_t* idx, const float* w, const float* a, const float* m, int B, int T, int P, int N, int K,
                         float* est, void* stream);

/* Scratch of one gvf_interp_loss_forward (the per-workgroup partials; independent of N and K). */
int gvf_interp_loss_scratch_bytes(int B, int T, int P, size_t* out);

/* Rules 4-5: loss_out (device, 1 fp32).  est (B, T, P, 3) and sign (B, T, P) bytes are written if not null; a sign byte holds
 * (s_x + 1) | (s_y + 1) << 2 | (s_z + 1) << 4 with s = sign(pred - est) in {-1, 0, 1}, and 0x15 (all zero) for padded queries. */
int gvf_interp_loss_forward(const float* pred, int64_t pred_stride, const int32_t* idx, const float* w, const float* a, const float* m,
                            const int32_t* len, int B, int T, int P, int N, int K, float* loss_out, float* est, uint8_t* sign,
                            void* scratch, size_t scratch_bytes, void* stream);

/* grad_pred row (b, t, p), channels 0..2 = grad_loss[0] * sign / (3 T sum_b len[b]) (grad_loss: device, 1 fp32, read on the
 * device); channels 3..grad_channels-1 are set to zero (3 <= grad_channels <= grad_stride), anything beyond is left untouched. */
int gvf_interp_loss_backward(const uint8_t* sign, const float* grad_loss, const int32_t* len, int B, int T, int P, float* grad_pred,
                             int64_t grad_stride, int grad_channels, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* GVF_INTERP_H */
