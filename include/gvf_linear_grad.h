/*
 * gvf_linear_grad.h -- C ABI of a projection's backward (csrc/linear_grad.hip): what a training step needs around y = x W^T + b beside
 * gvf_gemm (gvf_dit.h), which already serves the forward (W = the 16-bit image [N][K]) and the input gradient dX = dY W (the same entry
 * point with A = dY and W = the transposed image [K][N], no bias).
 *
 *   gvf_cast_transpose   ONE pass over an fp32 master weight [N][K] writes both 16-bit images: W16 [N][ld_k] and its transpose W16T [K][ld_n].
 *   gvf_gemm_wgrad       dW[n][k] = sum_m dY[m][n] X[m][k]  and  db[n] = sum_m dY[m][n]:  16-bit operands, fp32 accumulation (MFMA 16x16x32),
 *                        fp32 results straight onto the master gradients.
 *
 * The contraction index m is the SLOW axis of both operands of the weight gradient.  A workgroup (4 waves, one 128 x 128 tile of dW) stages 64
 * rows of each operand row-major into LDS (16-byte coalesced loads, rows of 288 bytes: 256 of data + 32 of padding) and reads the MFMA fragments
 * column-wise with gfx950's transposed LDS read (ds_read_b64_tr_b16; a 32-lane half reads 8 consecutive rows x 16 columns, whose 288-byte stride
 * puts them on 64 distinct banks).  Rows past M (and columns past N / K) enter as zeros and are never loaded.
 *
 * Split over m: the k-steps (32 rows each) of M are dealt to `splits` groups of ceil(ceil(M / 32) / splits) consecutive k-steps; group s writes
 * its fp32 partial tile (and, from the workgroups of the first column tile, the column sums of the dY rows it already holds: one more MFMA
 * against a fragment of ones) into slot s of the workspace, a group without rows writes zeros, and a second launch adds the slots in ascending
 * order.  No atomics, no waiting between workgroups: two calls on the same inputs give the same bits.  Rounding points of one output element: one fp32
 * rounding per k-step its group accumulates, one per slot the reducer adds.
 * splits = 0 takes gvf_gemm_wgrad_splits(M, N, K) = max(1, min(512 / tiles, 16, ceil(M / 32) / 8)), tiles = ceil(N / 128) ceil(K / 128): two
 * workgroups per CU of the MI355X (256 CUs) over the output tiles, at most 16 slots for the reducer to add, a group never shorter than 8 k-steps
 * -- a pure function of its arguments (integer divisions).
 *
 * Conventions as in gvf_dit_train.h: device pointers, an explicit stream (null = the default stream), no host synchronisation, no allocation, an
 * int status; `dtype` is GVF_DT_BF16 / GVF_DT_F16 of gvf_dit.h.  Everything is checked on the host before any launch and answered with GVF_EINVAL:
 * a null pointer, a dtype that is not a 16-bit type, N or K not positive (gvf_gemm_wgrad: not a positive multiple of 8), M < 0, a leading
 * dimension below its extent or not a multiple of 8 (ldw of the fp32 master: only below its extent), splits < 0 or > 65535, a workspace smaller than
 * gvf_gemm_wgrad_workspace_bytes reports, a pointer of gvf_gemm_wgrad that is not 16-byte aligned (4-byte alignment suffices for gvf_cast_transpose).
 */
#ifndef GVF_LINEAR_GRAD_H
#define GVF_LINEAR_GRAD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* W fp32 [N][K] (row stride ldw) -> W16 16-bit [N][ld_k] and W16T 16-bit [K][ld_n], rounded to nearest even (gvf_cast_pad's rounding); the padding
 * columns K .. ld_k - 1 of W16 and N .. ld_n - 1 of W16T are written as zeros, nothing else is written.  Any N, K > 0. */
int gvf_cast_transpose(int dtype, const float* W, int ldw, void* W16, int ld_k, void* W16T, int ld_n, int N, int K, void* stream);

/* The split count splits = 0 selects (>= 1), or GVF_EINVAL for M < 0, N <= 0, K <= 0. */
int gvf_gemm_wgrad_splits(int M, int N, int K);
/* *out = splits * (N * K + N) * 4 bytes, rounded up to a multiple of 256; splits = 0: for the count gvf_gemm_wgrad_splits picks. */
int gvf_gemm_wgrad_workspace_bytes(int M, int N, int K, int splits, size_t* out);
/* dY 16-bit [M][N] (row stride ldy), X 16-bit [M][K] (ldx), dW fp32 [N][K] (lddw), db fp32 [N] or null.  M >= 0 (M = 0: zeros), N % 8 == 0,
 * K % 8 == 0.  Reads nothing outside [M][N] / [M][K], writes nothing outside [N][K] / [N]; the workspace's contents before the call do not matter. */
int gvf_gemm_wgrad(int dtype, const void* dY, int ldy, const void* X, int ldx, int M, int N, int K, float* dW, int lddw, float* db,
                   void* workspace, size_t workspace_bytes, int splits, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* GVF_LINEAR_GRAD_H */
