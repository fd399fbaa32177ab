/*
 * gvf_dit_train.h -- C ABI of the element-wise training kernels of the DiT block (csrc/dit_train.hip):
 *   a. the backward of gvf_layernorm_modulate (gvf_dit.h), whose forward stays the inference kernel,
 *   b. the gated residual  out = x + gate_g * h,  forward and backward,
 *   c. the multi-head RMSNorm of q / k,  y = x / max(|x|, 1e-12) * gamma[h, :] * sqrt(d),  forward and backward.
 *
 * fp32 arithmetic inside; `dtype` (GVF_DT_BF16 / GVF_DT_F16 of gvf_dit.h) is the 16-bit storage type of the rows named "16-bit" below, rounded
 * once at the store.  One wave per row; rows are [rows, C] row-major and contiguous unless a leading dimension is given.  A "group" g of a
 * row is row / rows_per_group; per-group vectors (scale, gate) are rows of a [G, ld] fp32 table read in place, G = ceil(rows / rows_per_group).
 *
 * Sums over rows: every workgroup owns GVF_TRAIN_ROWS_PER_WG consecutive rows and writes its fp32 partial column sums into the
 * caller's workspace: workgroup wg writes one slot per group g it touches, at index wg + g (rows_per_group need not divide anything), so
 * group g owns the consecutive slots first_row(g) / 16 + g .. last_row(g) / 16 + g.  That is one slot written per workgroup and one more per
 * group boundary strictly inside a workgroup's rows; a boundary that falls between two workgroups leaves the index in between unused (never
 * written, never read), and the *_workspace_bytes queries reserve W + G slots per per-group output (W workgroups, G groups), W per output
 * that is not per group.  ONE further small launch adds the slots of each output in ascending order.  No float atomics: two calls on the
 * same inputs give the same bits, on any stream.
 *
 * Two code paths, as gvf_layernorm_modulate: C % 256 == 0 && C <= 1024 keeps the row in registers and moves it with 8- / 16-byte accesses (then
 * fp32 rows, ln_w, ln_b, the table rows (ld % 4 == 0) must be 16-byte aligned and 16-bit rows 8-byte aligned); any other C takes a generic path
 * without alignment demands.  The RMSNorm moves 16 bytes per lane on every shape: bases 16-byte aligned, leading dimensions multiples of 8.
 *
 * Conventions as in gvf_attn_bwd.h: device pointers, an explicit stream (null = the default stream), no host synchronisation, no allocation,
 * an int status.  Everything is checked on the host before any launch: GVF_EINVAL for a null pointer, a mismatched optional pair, a
 * misaligned pointer where the vector path would load it, a workspace smaller than the *_workspace_bytes query reports (or not 16-byte
 * aligned), a dtype that is not a 16-bit type.  rows == 0 returns GVF_OK without a launch.
 */
#ifndef GVF_DIT_TRAIN_H
#define GVF_DIT_TRAIN_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GVF_TRAIN_ROWS_PER_WG 16

/* a. Backward of  y = (xh * w + b) * (1 + scale_g) + shift_g,  xh = (x - mean) * rstd  (mean, rstd recomputed from x, the mean as a two-term sum:
 * rows with a large common offset keep fp32-accurate centred values).  x fp32, dy 16-bit, dres optional fp32 (the residual stream's incoming gradient, added into dx).
 *   dx        = dres + rstd * (g - mean(g) - xh * mean(g * xh)),   g = dy * (1 + scale) * w                    fp32 [rows, C]
 *   dshift[g] = sum dy,   dscale[g] = sum dy * (xh * w + b)            fp32 [G, C] contiguous; both required iff scale is given
 *   dw        = sum dy * (1 + scale) * xh,   db = sum dy * (1 + scale)   fp32 [C];          both required iff ln_w (and ln_b) is given
 * (shift itself does not enter any gradient and is not an argument.) */
int gvf_ln_mod_bwd_workspace_bytes(int rows, int C, int rows_per_group, size_t* out);
int gvf_ln_mod_bwd(int dtype, const float* x, const void* dy, const float* dres, float* dx, int rows, int C, float eps,
                   const float* ln_w, const float* ln_b, const float* scale, int mod_ld, int rows_per_group,
                   float* dshift, float* dscale, float* dw, float* db, void* workspace, size_t workspace_bytes, void* stream);

/* b. out = x + gate_g * h  (x, out fp32; h 16-bit; gate optional: null = plain x + h, and then rows_per_group / gate_ld are ignored). */
int gvf_gate_residual_fwd(int dtype, const float* x, const void* h, const float* gate, int gate_ld, int rows_per_group, float* out,
                          int rows, int C, void* stream);
/* dh = gate_g * dout (16-bit), dgate[g] = sum dout * h (fp32 [G, C] contiguous; required iff gate is given; without a gate h may be null
 * and no workspace is needed).  The gradient of x is dout itself. */
int gvf_gate_residual_bwd_workspace_bytes(int rows, int C, int rows_per_group, size_t* out);
int gvf_gate_residual_bwd(int dtype, const float* dout, const void* h, const float* gate, int gate_ld, int rows_per_group, void* dh,
                          float* dgate, int rows, int C, void* workspace, size_t workspace_bytes, void* stream);

/* c. x, y, dy, dx 16-bit [rows, H, d] with a row stride in elements (ld >= H * d; the q / k slice of a packed projection is read in
 * place), heads packed, d = 32 or 64, H * d <= 2048; gamma, dgamma fp32 [H, d].
 *   y  = x / max(|x|, 1e-12) * gamma * sqrt(d)
 *   dx = (u - xt * sum_d(u * xt)) / max(|x|, 1e-12),   u = dy * gamma * sqrt(d),   xt = x / max(|x|, 1e-12)
 *   dgamma = sqrt(d) * sum_rows dy * xt */
int gvf_rmsnorm_heads_fwd(int dtype, const void* x, int64_t ldx, const float* gamma, void* y, int64_t ldy, int rows, int H, int d,
                          void* stream);
int gvf_rmsnorm_heads_bwd_workspace_bytes(int rows, int H, int d, size_t* out);
int gvf_rmsnorm_heads_bwd(int dtype, const void* x, int64_t ldx, const void* dy, int64_t lddy, const float* gamma, void* dx, int64_t lddx,
                          float* dgamma, int rows, int H, int d, void* workspace, size_t workspace_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* GVF_DIT_TRAIN_H */
