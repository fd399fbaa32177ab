/*
 * gvf_sparse_train.h -- C ABI of the training kernels of the static VAE that are not matrix products (csrc/sparse_train.hip):
 *   a. the tanh-GELU between mlp.0 and mlp.2, forward and backward,
 *   b. the row gather  out[i, :] = src[index[i], :]  (window-order gather, scatter back, and both gradients),
 *   c. the posterior sample  z = mean + exp(0.5 logvar) eps  with its KL term, forward and backward,
 *   d. the volume and opacity regularisers of the Gaussians, forward and backward,
 *   e. the column sums of fp32 rows (a closing projection's bias gradient from the unrounded stream gradient).
 *
 * fp32 arithmetic inside; `dtype` (GVF_DT_BF16 / GVF_DT_F16 of gvf_dit.h) is the 16-bit storage type where an operator has one, rounded once at
 * the store.  16-byte accesses wherever the addresses allow (stated per operator); otherwise a scalar path, never an error.
 *
 * Scalars (kl, vol, opa) are means over rows: every workgroup writes ONE double-precision partial per scalar into its own slot of the caller's
 * workspace, and one small launch adds the slots in ascending order and scales.  No atomics, no host read, no wait between workgroups: two calls
 * on the same inputs give the same bits, on any stream.  Incoming scalar gradients (dkl, dvol, dopa) are DEVICE pointers to one fp32 each.
 *
 * Conventions as in gvf_dit_train.h: device pointers, an explicit stream (null = the default stream), no host synchronisation, no allocation,
 * an int status.  Everything is checked on the host before any launch: GVF_EINVAL for a null pointer, a non-positive extent where one is
 * required, a leading dimension smaller than the row, a workspace smaller than the *_workspace_bytes query reports (or not 8-byte aligned), a
 * dtype that is not a 16-bit type.  An empty call (n == 0, rows == 0) returns GVF_OK without a launch; the scalars have no value for T == 0 /
 * N == 0 (a mean over nothing), which is GVF_EINVAL.
 */
#ifndef GVF_SPARSE_TRAIN_H
#define GVF_SPARSE_TRAIN_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* a. u, a, da, du 16-bit, flat, n elements (any n).
 *   a  = 0.5 u (1 + t),   t = tanh(k (u + 0.044715 u^3)),   k = sqrt(2 / pi)
 *   du = da (0.5 (1 + t) + 0.5 u (1 - t^2) k (1 + 3 * 0.044715 u^2)),  the second term exactly 0 once |k (u + 0.044715 u^3)| >= 10 (t = +-1 in
 *        fp32 there), so that |u| up to the type's largest finite value gives finite a and du.
 * Evaluated as 0.5 (1 + t) = 1 / (1 + exp(-2 y)) on the hardware exponential: no cancellation for negative y, 1e-6 relative at the worst.
 * The first n / 8 * 8 elements move as 16-byte vectors when every pointer is 16-byte aligned, the rest (or everything) element by element. */
int gvf_gelu_tanh_fwd(int dtype, const void* u, void* a, int64_t n, void* stream);
int gvf_gelu_tanh_bwd(int dtype, const void* u, const void* da, void* du, int64_t n, void* stream);

/* b. out[i, 0:width_bytes] = src[index[i], 0:width_bytes],  i < rows.  The payload is opaque bytes (16-bit or fp32 rows alike): width_bytes a
 * positive multiple of 16, src_stride_bytes >= width_bytes and a multiple of 16 (a column slice of a wider matrix is read in place), out
 * contiguous [rows, width_bytes]; src and out 16-byte aligned, index int64 [rows] on the device.
 * PRECONDITION, not checked (checking would need a host read): 0 <= index[i] < the row count of src. */
int gvf_gather_rows(const void* src, int64_t src_stride_bytes, const int64_t* index, void* out, int64_t rows, int64_t width_bytes, void* stream);

/* c. h fp32 [T, >= 2L] with row stride ldh (elements) holding mean | logvar in its first 2L columns, eps fp32 [T, L] contiguous.
 *   z  = mean + exp(0.5 logvar) eps                      fp32 [T, L] contiguous
 *   kl = 0.5 mean_{T L} (mean^2 + exp(logvar) - logvar - 1)   one fp32 on the device
 * Backward: dz fp32 [T, L] contiguous or null (z unused), dkl one fp32 on the device or null (kl unused); dh fp32 [T, 2L] with row stride lddh,
 * written in one pass:
 *   dmean = dz + dkl mean / (T L),   dlogvar = dz 0.5 exp(0.5 logvar) eps + dkl 0.5 (exp(logvar) - 1) / (T L)
 * eps may be null when dz is.  L any positive count; float4 accesses when L % 4 == 0, the leading dimensions are multiples of 4 and the
 * pointers 16-byte aligned.  The exponential is expf (documented to 1 ulp). */
int gvf_posterior_workspace_bytes(int64_t T, int L, size_t* out);
int gvf_posterior_fwd(const float* h, int64_t ldh, const float* eps, float* z, float* kl, int64_t T, int L, void* workspace, size_t workspace_bytes,
                      void* stream);
int gvf_posterior_bwd(const float* h, int64_t ldh, const float* eps, const float* dz, const float* dkl, float* dh, int64_t lddh, int64_t T, int L,
                      void* stream);

/* d. scaling fp32 [N, 3] and opacity fp32 [N] contiguous: the RAW tensors of a GaussianModel (already lr-scaled).  activation 0 = exp,
 * 1 = softplus (torch's: x for x > 20, log1p(exp(x)) otherwise).
 *   vol = mean_i prod_k q_ik,   q_ik = sqrt(act(s_ik + scale_bias)^2 + min_kernel_size^2)
 *   opa = mean_i (sigmoid(o_i + opacity_bias) - 1)^2
 * Backward (dvol, dopa: one fp32 each on the device, either may be null = that term unused, its output then optional):
 *   ds_ik = dvol / N * prod_{j != k} q_ij * (a_ik / q_ik) * act'(s_ik + scale_bias)     (a / q taken as 0 where q = 0)
 *   do_i  = dopa / N * 2 (sg - 1) sg (1 - sg)
 * Four Gaussians per thread on 16-byte loads when the pointers are 16-byte aligned. */
int gvf_gaussian_reg_workspace_bytes(int64_t N, size_t* out);
int gvf_gaussian_reg_fwd(const float* scaling, const float* opacity, int64_t N, float scale_bias, float opacity_bias, float min_kernel_size,
                         int activation, float* vol, float* opa, void* workspace, size_t workspace_bytes, void* stream);
int gvf_gaussian_reg_bwd(const float* scaling, const float* opacity, int64_t N, float scale_bias, float opacity_bias, float min_kernel_size,
                         int activation, const float* dvol, const float* dopa, float* dscaling, float* dopacity, void* stream);

/* e. out[c] = sum_r x[r, c] for fp32 x [rows, C] contiguous, rows >= 1 (at most 65535 * 64), accumulated in double per chunk of 64 rows and
 * over the chunks in order: the bias gradient of a projection that closes a sub-layer, taken from the fp32 stream gradient BEFORE it is rounded
 * to the 16-bit operand of the weight-gradient product.  out fp32 [C]. */
int gvf_colsum_f32_workspace_bytes(int64_t rows, int C, size_t* out);
int gvf_colsum_f32(const float* x, int64_t rows, int C, float* out, void* workspace, size_t workspace_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* GVF_SPARSE_TRAIN_H */
