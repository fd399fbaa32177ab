/*
 * gvf_spconv.h -- C ABI of the submanifold sparse 3x3x3 convolution (the reference's sp.SparseConv3d -> spconv.SubMConv3d of the
 * structured-latent flow model, trellis/models/structured_latent_flow.py; csrc/spconv.hip) and of the LayerNorm + activation link in
 * front of it.
 *
 * Definition.  For active voxels p_i = (b, x, y, z), i < T, with unique coordinates:
 *
 *     out[i, co] = bias[co] + sum_{kx,ky,kz in {0,1,2}} sum_ci W[co, kx, ky, kz, ci] * in[j, ci]
 *
 * where j is the row whose coordinates are (b, x + kx - 1, y + ky - 1, z + kz - 1); the term is absent if no such row exists.  This
 * equals F.conv3d(dense, W.permute(0, 4, 1, 2, 3), bias, padding = 1) read back at the active sites: a cross-correlation (no flipped
 * taps), kernel axes in coordinate-column order, weights [Cout][3][3][3][Cin] -- the shape under which spconv 2 stores
 * SubMConv3d.weight.  The set of active sites does not change (submanifold): outputs exist at the input's rows only.
 *
 * Layouts.
 *   coords  int32 [T][4] = (b, x, y, z); x, y, z in [0, 1024) (as csrc/vox2seq.hip), b >= 0.
 *   nbr     int32 [T][27], tap index k = kx * 9 + ky * 3 + kz; the row index of the neighbour, or -1 where absent.  A neighbour
 *           coordinate of -1 or 1024 is absent (it never aliases another cell through the key packing); two samples with equal
 *           (x, y, z) are not neighbours.  A row whose own coordinates are out of range is in nobody's neighbourhood and has none.
 *   in      16-bit [T][ld_in], ld_in >= Cin: columns beyond Cin and rows beyond T are never read.
 *   wimg    the packed 16-bit image of the weight in the operand order of v_mfma_f32_16x16x32 (gvf_spconv_pack):
 *           element ((((cb * 27 + k) * (Cin / 32) + ch) * 64 + lane) * 8 + e) = W[16 cb + lane % 16][k][32 ch + 8 (lane / 16) + e].
 *   out     fp32 or 16-bit [T][Cout], dense; rows beyond T are never written.
 *
 * The convolution is an output-stationary implicit GEMM: a workgroup owns 64 output rows, walks the 27 taps in ascending order and
 * the Cin / 32 k-steps inside each, and gathers whole input rows by `nbr` into LDS.  Absent neighbours are written as zeros in LDS --
 * never loaded -- so a NaN in row j reaches only the outputs that list j as a neighbour.  A tap without a neighbour in the whole tile
 * is skipped.  There are no atomics in it and the accumulation order per output row is fixed: results are bit-identical from run to
 * run and across streams.  (The neighbour map's hash table uses integer atomics; the map does not depend on insertion order.)
 *
 * Conventions as in gvf_lpips.h: device pointers, an explicit stream (null = the default stream), an int status (GVF_OK or a negative
 * GVF_E*), caller-owned buffers with workspace-size queries.  Every argument is checked on the host before a launch: GVF_EINVAL for
 * null / misaligned pointers, bad channel counts or a bad dtype (GVF_DT_BF16 / GVF_DT_F16 of gvf_dit.h).  Sizes: T >= 1 and
 * 27 T < 2^31; Cin and Cout multiples of 64 up to 2048.  No gradient of any of these operators exists.
 */
#ifndef GVF_SPCONV_H
#define GVF_SPCONV_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* Bytes of the hash table gvf_spconv_neighbor_map needs for T rows. */
int gvf_spconv_map_workspace_bytes(int T, size_t* out);

/* coords (device, int32 [T][4]) -> nbr (device, int32 [T][27]).  Runs on the device alone (no host read-back): an open-addressing
 * table keyed on the 64-bit packing (b << 30 | x << 20 | y << 10 | z), filled by one launch and searched by the next.  workspace: device,
 * 256-byte aligned, >= the queried size (else GVF_ENOSPC); its contents need not be initialised. */
int gvf_spconv_neighbor_map(const int32_t* coords, int T, int32_t* nbr, void* workspace, size_t workspace_bytes, void* stream);

/* Bytes of the packed image of an fp32 [cout][3][3][3][cin] weight. */
int gvf_spconv_packed_bytes(int cout, int cin, size_t* out);

/* w (device, fp32 [cout][3][3][3][cin]) -> out (device, 16-byte aligned, >= packed_bytes, else GVF_ENOSPC), rounded to `dtype`.  Pack
 * once per (module, dtype), never per step. */
int gvf_spconv_pack(const float* w, int cout, int cin, int dtype, void* out, size_t out_bytes, void* stream);

/* out [T][cout] = conv(in, nbr, wimg) (+ bias[co], fp32, optional) (+ addend[i][co], fp32 [T][cout], optional: a block's skip path),
 * fp32 accumulation; the bias is added first, then the addend, one fp32 rounding each.  out_f32 != 0: out is fp32; else out has the
 * operand's 16-bit type (round to nearest even).  in, wimg, addend and out are 16-byte aligned; ld_in is a multiple of 8. */
int gvf_spconv3(const void* in, int ld_in, const int32_t* nbr, const void* wimg, const float* bias, const float* addend, void* out,
                int out_f32, int T, int cin, int cout, int dtype, void* stream);

#define GVF_ACT_NONE 0
#define GVF_ACT_SILU 1          /* v / (1 + exp(-v)) */

/* out16 [rows][C] (16-bit `dtype`) = act(LN_eps(x) [* ln_w + ln_b] [* (1 + scale) + shift]) of fp32 rows x [rows][C]: LayerNorm over C
 * (biased variance, two passes), the affine pair and the modulation pair each optional (both of a pair or neither).  ONE shift / scale
 * row (C fp32 each) per call: ragged batches call it per sample slice.  C a multiple of 4 up to 2048; x, ln_w, ln_b, shift, scale
 * 16-byte aligned, out16 8-byte aligned. */
int gvf_ln_act_rows(int dtype, const float* x, void* out16, int rows, int C, float eps, const float* ln_w, const float* ln_b,
                    const float* shift, const float* scale, int act, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* GVF_SPCONV_H */
