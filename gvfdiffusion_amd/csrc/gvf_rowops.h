// gvf_rowops.h -- the small helpers of the row and loss kernels that decide the bits of a result (internal): the wave and workgroup
// sums, each named after the order in which it adds; the 8 x 16-bit <-> fp32 packing; the erf GELU; the argument checks of the C entry
// points.  One definition each: two kernels that must agree (a backward that recomputes its forward's row statistics, a training forward
// that stores what the inference kernel stores, a GEMM epilogue and the stand-alone GEGLU) agree because they call the same function.
#pragma once
#include "gvf_common.h"
#include "gvf_lp.h"
#include "../../include/gvf_dit.h"

// ---- sums over a wave: every lane gets the total ------------------------------------------------------------------------------------------
// One DPP step on an fp32 value: what the lane's partner under `ctrl_` holds (all rows and banks enabled).
#define GVF_ROWOPS_DPP_F32(x_, ctrl_) \
    __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, x_), ctrl_, 0xF, 0xF, false))

// On the DPP / permlane data paths only (quad_perm, row mirrors, v_permlane16_swap, v_permlane32_swap), nothing through the LDS unit.
// Order: lane ^ 1, lane ^ 2, the other quad of the half row, the other half of the row, rows 0+1 | 2+3, the two halves of the wave.
// The LayerNorm kernels of elem.hip, dit_train.hip and spconv.hip share it: a backward recomputes the forward's mean and rstd to the bit.
__device__ __forceinline__ float gvf_wave_sum_dpp(float v) {
    v += GVF_ROWOPS_DPP_F32(v, 0xB1);      // quad_perm [1,0,3,2]: lane ^ 1
    v += GVF_ROWOPS_DPP_F32(v, 0x4E);      // quad_perm [2,3,0,1]: lane ^ 2
    v += GVF_ROWOPS_DPP_F32(v, 0x141);     // row_half_mirror: lane i of 8 <-> 7 - i (the other quad of the half row)
    v += GVF_ROWOPS_DPP_F32(v, 0x140);     // row_mirror: lane i of 16 <-> 15 - i (the other half of the row)
    const unsigned u = __builtin_bit_cast(unsigned, v);
    const auto r16 = __builtin_amdgcn_permlane16_swap(u, u, false, false);      // {rows 0,0,2,2 | rows 1,1,3,3}: their sum = rows 0+1 | 2+3
    const unsigned a0 = r16[0], a1 = r16[1];
    const float w = __uint_as_float(a0) + __uint_as_float(a1);
    const unsigned uw = __builtin_bit_cast(unsigned, w);
    const auto r32 = __builtin_amdgcn_permlane32_swap(uw, uw, false, false);
    const unsigned b0 = r32[0], b1 = r32[1];
    return __uint_as_float(b0) + __uint_as_float(b1);
}

// The xor butterfly, lane ^ 32 first and lane ^ 1 last.  The motion VAE's embedding LayerNorms (vae.hip, vae_train.hip): the training
// forward stores the same values as the inference kernel.
__device__ __forceinline__ float gvf_wave_sum_xor(float v) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d, 64);
    return v;
}

// The 16 lanes of a DPP row (lane ^ 1, ^ 2, ^ 4, ^ 8): a 64-column slice of a row held as one float4 per lane (the partial LayerNorm
// statistics gvf_gemm_ln reads, written by the row kernels of clip.hip).
__device__ __forceinline__ float gvf_row16_sum_xor(float v) {
#pragma unroll
    for (int d = 1; d < 16; d <<= 1) v += __shfl_xor(v, d, 64);
    return v;
}

// ---- sums over a workgroup of THREADS threads; red: LDS scratch ---------------------------------------------------------------------------
// A fixed tree over the threads (red: THREADS doubles), so a workgroup's partial does not depend on anything but its terms.  Every thread
// gets the total.
template <int THREADS>
__device__ __forceinline__ double gvf_block_sum_tree(double v, double* red) {
    red[threadIdx.x] = v;
    __syncthreads();
    for (int s = THREADS / 2; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) red[threadIdx.x] += red[threadIdx.x + s];
        __syncthreads();
    }
    const double r = red[0];
    __syncthreads();
    return r;
}

// Each wave by a fixed shuffle tree, then thread 0 adds waves 0 .. THREADS / 64 - 1 in that order (red: one double per wave): the loss
// and gradient-norm scalars come out the same bits every run.
template <int THREADS>
__device__ __forceinline__ double gvf_block_sum_waves(double v, double* red) {
#pragma unroll
    for (int off = GVF_WAVE / 2; off > 0; off >>= 1) v += __shfl_down(v, off, GVF_WAVE);
    const int wave = threadIdx.x / GVF_WAVE;
    if ((threadIdx.x & (GVF_WAVE - 1)) == 0) red[wave] = v;
    __syncthreads();
    double s = 0.0;
    if (threadIdx.x == 0)
        for (int w = 0; w < THREADS / GVF_WAVE; ++w) s += red[w];
    __syncthreads();
    return s;   // valid in thread 0
}

// ---- 16 bytes of eight 16-bit elements <-> eight floats ---------------------------------------------------------------------------------
template <int DT>
__device__ __forceinline__ void gvf_unpack8(uint4 q, float (&f)[8]) {
    f[0] = GvfLp<DT>::lo(q.x); f[1] = GvfLp<DT>::hi(q.x); f[2] = GvfLp<DT>::lo(q.y); f[3] = GvfLp<DT>::hi(q.y);
    f[4] = GvfLp<DT>::lo(q.z); f[5] = GvfLp<DT>::hi(q.z); f[6] = GvfLp<DT>::lo(q.w); f[7] = GvfLp<DT>::hi(q.w);
}
template <int DT>
__device__ __forceinline__ uint4 gvf_pack8(const float (&f)[8]) {
    uint4 q;
    q.x = GvfLp<DT>::pack(f[0], f[1]); q.y = GvfLp<DT>::pack(f[2], f[3]); q.z = GvfLp<DT>::pack(f[4], f[5]); q.w = GvfLp<DT>::pack(f[6], f[7]);
    return q;
}

// ---- GELU, the exact erf form (model/autoencoder.py:90-93) ---------------------------------------------------------------------------------
// The GEGLU kernels (vae.hip, vae_train.hip) and the GEGLU epilogues of the GEMMs (gemm.hip, gemm8.hip) must agree bit for bit.
__device__ __forceinline__ float gvf_gelu_erf(float x) { return 0.5f * x * (1.0f + erff(x * 0.70710678118654752440f)); }

// ---- QuickGELU x * sigmoid(1.702 x) (CLIP's MLP) ---------------------------------------------------------------------------------------------
// expf, not __expf: the argument reaches +-1e5 for a 16-bit pre-activation.  exp(+large) = inf gives x / inf = -0 (x < 0 there), exp(-large) = 0
// gives x: finite for every finite x.
__device__ __forceinline__ float gvf_quick_gelu(float x) { return x / (1.0f + expf(-1.702f * x)); }

// ---- host: argument checks of the C entry points ------------------------------------------------------------------------------------------
static inline bool gvf_lp_ok(int dtype) { return dtype == GVF_DT_BF16 || dtype == GVF_DT_F16; }
static inline bool gvf_mis(const void* p, uintptr_t mask) { return (((uintptr_t)p) & mask) != 0; }      // misaligned: mask = alignment - 1
static inline long long gvf_cdiv(long long a, long long b) { return (a + b - 1) / b; }
