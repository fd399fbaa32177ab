/*
 * gvf_conv3d.h -- C ABI of the dense 3x3x3 convolution (nn.Conv3d(cin, cout, 3, padding = 1) of the reference's sparse-structure decoder,
 * trellis/models/sparse_structure_vae.py; csrc/conv3d.hip) with the decoder's pixel-shuffle folded into its store, and of the occupancy
 * read-out that turns the decoder's logits into sparse-structure coordinates.
 *
 * Layout.  A dense volume is a row matrix [B * X * Y * Z][C] with row = ((b * X + x) * Y + y) * Z + z: the rows of a SparseTensor whose
 * coordinates are the full grid in grid order.
 *
 * Definition.  out = F.conv3d(in, W, bias, padding = 1) in row layout:
 *
 *     out[(b, x, y, z), co] = bias[co] + sum_{kx,ky,kz in {0,1,2}} sum_ci W[co, ci, kx, ky, kz] * in[(b, x + kx - 1, y + ky - 1, z + kz - 1), ci]
 *
 * a cross-correlation (no flipped taps) with zero padding at all six faces; a term whose neighbour is outside the grid is absent; samples
 * do not see each other.
 *
 *   in      16-bit [rows][ld_in], ld_in a multiple of 8 and >= roundup32(cin).  Columns cin .. roundup32(cin) - 1 ARE read (they meet zero
 *           weights, so the caller passes zeros there: a NaN or an infinity in them poisons the row's neighbourhood); columns from
 *           roundup32(cin) on and rows beyond B X Y Z are never read.
 *   wimg    the packed 16-bit image of the weight in the operand order of v_mfma_f32_16x16x32 (gvf_conv3d3_pack), cin zero-padded to a
 *           multiple of 32 and cout to a multiple of 16: with nch = roundup32(cin) / 32 and tap k = kx * 9 + ky * 3 + kz, element
 *           ((((cb * nch + ch) * 27 + k) * 64 + lane) * 8 + e) = W[16 cb + lane % 16][32 ch + 8 (lane / 16) + e][k].
 *   out     store GVF_CONV3D_STORE_ROWS: fp32 or 16-bit [rows][cout], dense.
 *           store GVF_CONV3D_STORE_SHUFFLE2 (the reference's pixel_shuffle_3d(., 2), trellis/modules/spatial.py): cout a multiple of 8;
 *           output channel c = ((c' * 2 + i) * 2 + j) * 2 + k of voxel (b, x, y, z) is written to channel c' of voxel (b, 2x + i, 2y + j,
 *           2z + k) of a [B * 2X * 2Y * 2Z][cout / 8] volume, which is written once and in no other form.
 *   addend  fp32, optional, in the layout and shape of `out` (the shuffled one under SHUFFLE2).
 *
 * The convolution is an output-stationary implicit GEMM: a workgroup owns a 4 x 4 x 4 brick of output voxels and a tile of output channels,
 * stages the brick's 6 x 6 x 6 halo of one 32-channel chunk in LDS once and reads it 27 times with shifted addresses.  Halo cells outside
 * the grid are written to LDS as zeros -- never loaded -- so a NaN in one voxel reaches exactly the outputs of its up to 27 neighbours, and
 * no address outside [in, in + rows * ld_in) is formed.  The chunks go in ascending order and the 27 taps in ascending order inside each:
 * 27 ceil(cin / 32) MFMA k-steps per output.  No atomics, a fixed accumulation order: bit-identical from run to run and across streams.
 *
 * Conventions as in gvf_spconv.h: device pointers, an explicit stream (null = the default stream), an int status (GVF_OK or a negative
 * GVF_E*), caller-owned buffers with size queries.  Every argument is checked on the host before a launch: GVF_EINVAL for null /
 * misaligned pointers, bad sizes, a bad dtype (GVF_DT_BF16 / GVF_DT_F16 of gvf_dit.h) or store mode; GVF_ENOSPC for a short buffer.
 * Sizes: 1 <= cin, cout <= 2048; B, X, Y, Z >= 1 with 27 B X Y Z < 2^31 (and 27 * 8 B X Y Z < 2^31 under SHUFFLE2).  No gradients.
 */
#ifndef GVF_CONV3D_H
#define GVF_CONV3D_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GVF_CONV3D_STORE_ROWS 0
#define GVF_CONV3D_STORE_SHUFFLE2 1

/* Bytes of the packed image of an fp32 [cout][cin][3][3][3] weight: roundup16(cout) * roundup32(cin) * 27 * 2. */
int gvf_conv3d3_packed_bytes(int cout, int cin, size_t* out);

/* w (device, fp32 [cout][cin][3][3][3]: nn.Conv3d's own layout) -> out (device, 16-byte aligned, >= packed_bytes, else GVF_ENOSPC),
 * rounded to `dtype`, the padding written as zeros.  Pack once per (module, dtype), never per call. */
int gvf_conv3d3_pack(const float* w, int cout, int cin, int dtype, void* out, size_t out_bytes, void* stream);

/* out = conv(in, wimg) (+ bias[co], fp32 [cout], optional) (+ addend, fp32, optional: a block's skip path); fp32 accumulation; the bias
 * is added first, then the addend, one fp32 rounding each.  out_f32 != 0: out is fp32; else out has the operand's 16-bit type (round to
 * nearest even).  in and wimg are 16-byte aligned; bias, addend 4-byte; out 4-byte (fp32) or 2-byte. */
int gvf_conv3d3(const void* in, int ld_in, const void* wimg, const float* bias, const float* addend, void* out, int out_f32, int store,
                int B, int X, int Y, int Z, int cin, int cout, int dtype, void* stream);

/* Bytes of the workspace gvf_occupancy_coords needs for `cells` = B X Y Z logits. */
int gvf_occupancy_workspace_bytes(int64_t cells, size_t* out);

/* logits (device, fp32 [B][X * Y * Z]) -> coords (device, int32 [n][4] = (b, x, y, z)) of the cells with logit > 0 in ascending row
 * order -- torch.argwhere(dense > 0)[:, [0, 2, 3, 4]] -- and n to *count (device int32).  +0, -0 and NaN are not occupied.  Per-block
 * counts, one scan, ordered writes: no atomic append, so the order is part of the contract and the result is deterministic.
 * capacity: the rows `coords` can hold; it must cover the worst case (capacity >= B X Y Z, else GVF_ENOSPC).  workspace: device, 256-byte
 * aligned, >= the queried size (else GVF_ENOSPC); its contents need not be initialised.  coords is 16-byte aligned. */
int gvf_occupancy_coords(const float* logits, int B, int X, int Y, int Z, int32_t* coords, int64_t capacity, int32_t* count,
                         void* workspace, size_t workspace_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* GVF_CONV3D_H */
