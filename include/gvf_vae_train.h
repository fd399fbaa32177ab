/*
 * gvf_vae_train.h -- C ABI of the training kernels of the motion VAE that are not matrix products or attention (csrc/vae_train.hip):
 *   a. GEGLU  a = x * gelu_erf(g)  on the 16-bit rows u = [x | g], forward and backward,
 *   b. the point / Gaussian embedding  e = LN(r W^T + b) + LN(PointEmbed(r[:, 0:3]))  as an fp32 tensor, forward and backward,
 *   c. the posterior sample with the reference's clamp on logvar and ONE KL term per group of rows, forward and backward.
 *
 * fp32 arithmetic inside; `dtype` (GVF_DT_BF16 / GVF_DT_F16 of gvf_dit.h) is the 16-bit storage type of (a), rounded once at the store; (b) and
 * (c) are fp32 at every interface.  The inference kernels gvf_geglu / gvf_vae_embed of gvf_vae.h are separate entry points and unchanged.
 *
 * Reductions (dW, db of the embedding; kl of a group): every workgroup writes ONE partial per result into its own slot of the caller's
 * workspace, and a second launch adds the slots in ascending order (in double) and rounds once.  No atomics, no host read, no wait between
 * workgroups: two calls on the same inputs give the same bits, on any stream.  The workspace needs no initialisation.
 *
 * Conventions as in gvf_sparse_train.h: device pointers, an explicit stream (null = the default stream), no host synchronisation, no
 * allocation, an int status.  Everything is checked on the host before any launch: GVF_EINVAL for a null pointer, a negative extent, an extent
 * of 0 where the result is a mean, a leading dimension smaller than the row, a pointer or stride that misses the stated alignment, a workspace
 * smaller than the *_workspace_bytes query reports (or not 8-byte aligned), a dtype that is not a 16-bit type.  An empty call (rows == 0,
 * P == 0, G == 0) returns GVF_OK without a launch.
 */
#ifndef GVF_VAE_TRAIN_H
#define GVF_VAE_TRAIN_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* a. u 16-bit [rows, 2F] with row stride ldu: x = u[:, 0:F], g = u[:, F:2F].  F a positive multiple of 8, every leading dimension a multiple
 * of 8 elements and every pointer 16-byte aligned: all accesses are 16-byte vectors.
 *   a  = x * gelu(g),  gelu(g) = g Phi(g),  Phi(g) = 0.5 (1 + erf(g / sqrt 2))                  16-bit [rows, F], row stride lda
 *   dx = da * gelu(g),  dg = da * (x * (Phi(g) + g phi(g))),  phi(g) = exp(-g^2 / 2) / sqrt(2 pi)   16-bit du = [dx | dg], row stride lddu
 * Each output is rounded once.  The term g phi(g) is exactly 0 from |g| = 14 on (there it is below 2e-42: nothing a stored value can show),
 * and x (Phi + g phi) is clamped to the largest finite fp32 before it meets da: no inf * 0 and no NaN for ANY finite u and da, and a finite
 * result wherever the exact one fits the type. */
int gvf_geglu_fwd(int dtype, const void* u, int64_t ldu, void* a, int64_t lda, int64_t rows, int F, void* stream);
int gvf_geglu_bwd(int dtype, const void* u, int64_t ldu, const void* da, int64_t ldda, void* du, int64_t lddu, int64_t rows, int F, void* stream);

/* b. r fp32 [P, qdim] contiguous (3 <= qdim <= 16; columns 0..2 are xyz), W fp32 [C, qdim], bias fp32 [C], omega fp32 [C / 6]; C a positive
 * multiple of 6, at most 768.  With u = r W^T + bias and v = PointEmbed(r[:, 0:3]) (per axis: sin(p omega_j), j < C / 6, then cos(p omega_j)):
 *   e = LN(u) + LN(v),  LN(t) = (t - mean t) / sqrt(var t + eps), no affine                       fp32 [P, C] contiguous
 * Backward from de fp32 [P, C] contiguous; u, v and both rows' statistics are recomputed, nothing is saved by the forward:
 *   du = LN'(u)[de],  dv = LN'(v)[de],  LN'(t)[d] = rstd (d - mean d - th mean(d th)),  th = LN(t)
 *   dW [C, qdim] = du^T r,   db [C] = column sums of du                                           (partials + finaliser)
 *   dr [P, qdim] = du W  +  on columns 0..2  sum_j omega_j (dv_sin cos(p omega_j) - dv_cos sin(p omega_j))      or null: not computed
 * sin / cos are the library's accurate routines (the result is an fp32 interface, not a 16-bit operand).  4-byte aligned pointers. */
int gvf_vae_embed_train_fwd(const float* r, int qdim, const float* W, const float* bias, const float* omega, float* e, int64_t P, int C, float eps,
                            void* stream);
int gvf_vae_embed_bwd_workspace_bytes(int64_t P, int qdim, int C, size_t* out);
int gvf_vae_embed_bwd(const float* r, int qdim, const float* W, const float* bias, const float* omega, const float* de, float* dW, float* db,
                      float* dr, int64_t P, int C, float eps, void* workspace, size_t workspace_bytes, void* stream);

/* c. mean, logvar fp32 [G * L, Dl] with row strides ld_mean / ld_logvar (two column slices of one [G * L, 2 Dl] matrix are read in place):
 * G groups of L consecutive rows.  eps, z, dz fp32 [G * L, Dl] contiguous.
 *   lv = min(max(logvar, -30), 20),   z = mean + exp(0.5 lv) eps
 *   kl[g] = 0.5 / (L Dl) * sum over the group of (mean^2 + exp(lv) - 1 - lv)      fp32 terms, double sums                 fp32 [G]
 * Backward: dz or null (z unused; eps may then be null too), dkl fp32 [G] or null (kl unused):
 *   dmean   = dz + (dkl[g] mean) / (L Dl)
 *   dlogvar = inside * (dz 0.5 exp(0.5 lv) eps + (0.5 dkl[g] (exp(lv) - 1)) / (L Dl)),  inside = 1 for -30 <= logvar <= 20, else 0
 * (the clamp's gradient is 1 ON the bounds: torch's rule).  dmean / dlogvar with row strides ld_dmean / ld_dlogvar.  float4 accesses when
 * Dl % 4 == 0, every leading dimension is a multiple of 4 and every pointer 16-byte aligned; element-wise otherwise.  expf (1 ulp). */
int gvf_posterior_groups_workspace_bytes(int64_t G, int64_t L, int Dl, size_t* out);
int gvf_posterior_groups_fwd(const float* mean, int64_t ld_mean, const float* logvar, int64_t ld_logvar, const float* eps, float* z, float* kl,
                             int64_t G, int64_t L, int Dl, void* workspace, size_t workspace_bytes, void* stream);
int gvf_posterior_groups_bwd(const float* mean, int64_t ld_mean, const float* logvar, int64_t ld_logvar, const float* eps, const float* dz,
                             const float* dkl, float* dmean, int64_t ld_dmean, float* dlogvar, int64_t ld_dlogvar, int64_t G, int64_t L, int Dl,
                             void* stream);

#ifdef __cplusplus
}
#endif
#endif /* GVF_VAE_TRAIN_H */
