// dit_train.hip -- the element-wise training kernels of the DiT block for gfx950 (include/gvf_dit_train.h): the backward of the fused
// LayerNorm + (affine | adaLN modulate) of elem.hip, the gated residual and the multi-head RMSNorm of q / k, forward and backward.
//
// Reference: model/dit.py:246-277 (norm -> h * (1 + scale) + shift -> sub-layer -> h * gate -> x + h), model/attention/modules.py:8-15
// (MultiHeadRMSNorm).  Under autocast the reference runs each of these as 8-10 bandwidth-bound launches forward and as many backward, plus the
// broadcast-gradient reductions over the rows of a sample; here a sub-layer boundary is one launch each way and one small finaliser.
// One wave per row, the row in registers (C <= 1024), fp32 inside, 16-bit only at the stores.  Sums over rows are per-workgroup partials in
// a fixed slot of the workspace, added in slot order by colsum_finalize_kernel: no atomics, same bits every run.
#include <cmath>
#include "gvf_common.h"
#include "gvf_lp.h"
#include "gvf_rowops.h"
#include "../../include/gvf_rast.h"
#include "../../include/gvf_dit.h"
#include "../../include/gvf_dit_train.h"

namespace {

constexpr int RPW = GVF_TRAIN_ROWS_PER_WG;        // rows per workgroup (4 waves, rows r0 + wave + 4 i)

// Sum over aligned groups of NL = 4 or 8 lanes (one head of the RMSNorm: 8 channels per lane): the first steps of gvf_wave_sum_dpp
template <int NL>
__device__ __forceinline__ float group_sum(float v) {
    v += GVF_ROWOPS_DPP_F32(v, 0xB1);
    v += GVF_ROWOPS_DPP_F32(v, 0x4E);
    if (NL == 8) v += GVF_ROWOPS_DPP_F32(v, 0x141);
    return v;
}

// The slot of workgroup wg's partial for group g: wg + g.  A workgroup's rows cover groups g_lo..g_hi and the next workgroup starts at a
// group >= g_hi, so the pairs (wg, g) in row order get strictly increasing slots, and the slots of one group are consecutive:
// (first workgroup touching g) + g .. (last workgroup touching g) + g.  At most n_wg + G - 1 slots.  Outputs that are not per group use
// slot wg (G = 1 in the finaliser).
__device__ __forceinline__ long long seg_lo(long long r0, long long g, long long rpg) { const long long a = g * rpg; return a > r0 ? a : r0; }
__device__ __forceinline__ long long seg_hi(long long r1, long long g, long long rpg) { const long long a = (g + 1) * rpg; return a < r1 ? a : r1; }

// the four waves' register partials of n_cols columns -> one slot, waves added in order 0..3.  lds: 4 * n_cols floats.
template <int N4>
__device__ __forceinline__ void flush_cols(const float (&acc)[N4][4], float* lds, float* dst, int n_cols, int lane, int wave, int tid) {
#pragma unroll
    for (int i = 0; i < N4; ++i)
        *reinterpret_cast<float4*>(lds + (size_t)wave * n_cols + (lane + 64 * i) * 4) = make_float4(acc[i][0], acc[i][1], acc[i][2], acc[i][3]);
    __syncthreads();
    for (int c = tid; c < n_cols; c += 256) dst[c] = ((lds[c] + lds[n_cols + c]) + lds[2 * n_cols + c]) + lds[3 * n_cols + c];
    __syncthreads();
}

template <int DT>
__device__ __forceinline__ void unpack4(uint2 q, float (&f)[4]) {
    f[0] = GvfLp<DT>::lo(q.x); f[1] = GvfLp<DT>::hi(q.x); f[2] = GvfLp<DT>::lo(q.y); f[3] = GvfLp<DT>::hi(q.y);
}

// ---- a. LayerNorm + adaLN backward ----------------------------------------------------------------------------------------------------
// VPL = float4 per lane: C = 256 VPL.  rpg = rows when there is no scale (one group).
template <int VPL, int DT>
__global__ __launch_bounds__(256) void ln_bwd_kernel(const float* __restrict__ x, const unsigned short* __restrict__ dy, const float* __restrict__ dres,
                                                     float* __restrict__ dx, int rows, float eps, const float* __restrict__ ln_w,
                                                     const float* __restrict__ ln_b, const float* __restrict__ scale, int mod_ld, long long rpg,
                                                     float* __restrict__ p_shift, float* __restrict__ p_scale, float* __restrict__ p_w,
                                                     float* __restrict__ p_b) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    constexpr int C = 256 * VPL;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const long long r0 = (long long)blockIdx.x * RPW, r1 = r0 + RPW < rows ? r0 + RPW : rows;
    const long long g_lo = r0 / rpg, g_hi = (r1 - 1) / rpg;
    float w[VPL][4], b[VPL][4], aw[VPL][4], ab[VPL][4];
#pragma unroll
    for (int i = 0; i < VPL; ++i) {
        const int c0 = (lane + 64 * i) * 4;
        float4 w4 = make_float4(1.f, 1.f, 1.f, 1.f), b4 = make_float4(0.f, 0.f, 0.f, 0.f);
        if (ln_w != nullptr) { w4 = *reinterpret_cast<const float4*>(ln_w + c0); b4 = *reinterpret_cast<const float4*>(ln_b + c0); }
        w[i][0] = w4.x; w[i][1] = w4.y; w[i][2] = w4.z; w[i][3] = w4.w;
        b[i][0] = b4.x; b[i][1] = b4.y; b[i][2] = b4.z; b[i][3] = b4.w;
#pragma unroll
        for (int e = 0; e < 4; ++e) aw[i][e] = ab[i][e] = 0.f;
    }
    for (long long g = g_lo; g <= g_hi; ++g) {
        const long long s0 = seg_lo(r0, g, rpg), s1 = seg_hi(r1, g, rpg);
        float m[VPL][4], as[VPL][4], ac[VPL][4];
#pragma unroll
        for (int i = 0; i < VPL; ++i) {
            float4 sc = make_float4(0.f, 0.f, 0.f, 0.f);
            if (scale != nullptr) sc = *reinterpret_cast<const float4*>(scale + (size_t)g * mod_ld + (lane + 64 * i) * 4);
            m[i][0] = 1.0f + sc.x; m[i][1] = 1.0f + sc.y; m[i][2] = 1.0f + sc.z; m[i][3] = 1.0f + sc.w;
#pragma unroll
            for (int e = 0; e < 4; ++e) as[i][e] = ac[i][e] = 0.f;
        }
        for (long long row = s0 + wave; row < s1; row += 4) {
            const float4* xr = reinterpret_cast<const float4*>(x + (size_t)row * C);
            const uint2* dr = reinterpret_cast<const uint2*>(dy + (size_t)row * C);
            float4 v[VPL];
            uint2 dq[VPL];
            float s = 0.f;
#pragma unroll
            for (int i = 0; i < VPL; ++i) {
                v[i] = xr[lane + 64 * i];
                dq[i] = dr[lane + 64 * i];
                s += (v[i].x + v[i].y) + (v[i].z + v[i].w);
            }
            // mean as a two-term sum mean + mean_lo: with one fp32 term a row whose mean is 100 x its spread (a residual stream with a common
            // offset) carries half an ulp of the MEAN into every centred value, 1e-5 of xh -- invisible in the 16-bit forward output, the
            // largest error of the fp32 gradients
            const float mean = gvf_wave_sum_dpp(s) / (float)C;
            float r = 0.f;
#pragma unroll
            for (int i = 0; i < VPL; ++i) r += ((v[i].x - mean) + (v[i].y - mean)) + ((v[i].z - mean) + (v[i].w - mean));
            const float mean_lo = gvf_wave_sum_dpp(r) / (float)C;
            float q = 0.f;
#pragma unroll
            for (int i = 0; i < VPL; ++i) {
                v[i].x = (v[i].x - mean) - mean_lo; v[i].y = (v[i].y - mean) - mean_lo; v[i].z = (v[i].z - mean) - mean_lo; v[i].w = (v[i].w - mean) - mean_lo;
                q += (v[i].x * v[i].x + v[i].y * v[i].y) + (v[i].z * v[i].z + v[i].w * v[i].w);
            }
            const float rstd = rsqrtf(gvf_wave_sum_dpp(q) / (float)C + eps);
            float xh[VPL][4], gg[VPL][4];
            float sg = 0.f, sgx = 0.f;
#pragma unroll
            for (int i = 0; i < VPL; ++i) {
                float d4[4];
                unpack4<DT>(dq[i], d4);
                xh[i][0] = v[i].x * rstd; xh[i][1] = v[i].y * rstd; xh[i][2] = v[i].z * rstd; xh[i][3] = v[i].w * rstd;
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const float a = xh[i][e] * w[i][e] + b[i][e];        // the affine output (w = 1, b = 0 without an affine pair)
                    const float gm = d4[e] * m[i][e];
                    as[i][e] += d4[e];
                    ac[i][e] += d4[e] * a;
                    aw[i][e] += gm * xh[i][e];
                    ab[i][e] += gm;
                    gg[i][e] = gm * w[i][e];
                    sg += gg[i][e];
                    sgx += gg[i][e] * xh[i][e];
                }
            }
            const float c1 = gvf_wave_sum_dpp(sg) / (float)C, c2 = gvf_wave_sum_dpp(sgx) / (float)C;
            float4* dxr = reinterpret_cast<float4*>(dx + (size_t)row * C);
            const float4* rr = reinterpret_cast<const float4*>(dres + (size_t)row * C);
#pragma unroll
            for (int i = 0; i < VPL; ++i) {
                float4 o = make_float4(0.f, 0.f, 0.f, 0.f);
                if (dres != nullptr) o = rr[lane + 64 * i];
                o.x += rstd * (gg[i][0] - c1 - xh[i][0] * c2);
                o.y += rstd * (gg[i][1] - c1 - xh[i][1] * c2);
                o.z += rstd * (gg[i][2] - c1 - xh[i][2] * c2);
                o.w += rstd * (gg[i][3] - c1 - xh[i][3] * c2);
                dxr[lane + 64 * i] = o;
            }
        }
        if (p_shift != nullptr) {
            flush_cols<VPL>(as, lds, p_shift + (size_t)(blockIdx.x + g) * C, C, lane, wave, tid);
            flush_cols<VPL>(ac, lds, p_scale + (size_t)(blockIdx.x + g) * C, C, lane, wave, tid);
        }
    }
    if (p_w != nullptr) {
        flush_cols<VPL>(aw, lds, p_w + (size_t)blockIdx.x * C, C, lane, wave, tid);
        flush_cols<VPL>(ab, lds, p_b + (size_t)blockIdx.x * C, C, lane, wave, tid);
    }
}

// any C: the waves write dx and leave the row statistics in LDS, then every thread owns columns tid, tid + 256, ... and walks the
// workgroup's rows in order (the rows come back from cache)
template <int DT>
__global__ __launch_bounds__(256) void ln_bwd_generic_kernel(const float* __restrict__ x, const unsigned short* __restrict__ dy, const float* __restrict__ dres,
                                                             float* __restrict__ dx, int rows, int C, float eps, const float* __restrict__ ln_w,
                                                             const float* __restrict__ ln_b, const float* __restrict__ scale, int mod_ld, long long rpg,
                                                             float* __restrict__ p_shift, float* __restrict__ p_scale, float* __restrict__ p_w,
                                                             float* __restrict__ p_b) {
    __shared__ float s_mean[RPW], s_lo[RPW], s_rstd[RPW];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const long long r0 = (long long)blockIdx.x * RPW, r1 = r0 + RPW < rows ? r0 + RPW : rows;
    const long long g_lo = r0 / rpg, g_hi = (r1 - 1) / rpg;
    for (long long row = r0 + wave; row < r1; row += 4) {
        const float* xr = x + (size_t)row * C;
        const unsigned short* dr = dy + (size_t)row * C;
        float s = 0.f;
        for (int c = lane; c < C; c += 64) s += xr[c];
        const float mean = gvf_wave_sum_dpp(s) / (float)C;
        float r = 0.f;
        for (int c = lane; c < C; c += 64) r += xr[c] - mean;
        const float mean_lo = gvf_wave_sum_dpp(r) / (float)C;           // (the two-term mean of ln_bwd_kernel)
        float q = 0.f;
        for (int c = lane; c < C; c += 64) { const float a = (xr[c] - mean) - mean_lo; q += a * a; }
        const float rstd = rsqrtf(gvf_wave_sum_dpp(q) / (float)C + eps);
        const float* sc = scale != nullptr ? scale + (size_t)(row / rpg) * mod_ld : nullptr;
        float sg = 0.f, sgx = 0.f;
        for (int c = lane; c < C; c += 64) {
            const float xh = ((xr[c] - mean) - mean_lo) * rstd;
            float g = GvfLp<DT>::from16(dr[c]);
            if (sc != nullptr) g *= 1.0f + sc[c];
            if (ln_w != nullptr) g *= ln_w[c];
            sg += g;
            sgx += g * xh;
        }
        const float c1 = gvf_wave_sum_dpp(sg) / (float)C, c2 = gvf_wave_sum_dpp(sgx) / (float)C;
        for (int c = lane; c < C; c += 64) {
            const float xh = ((xr[c] - mean) - mean_lo) * rstd;
            float g = GvfLp<DT>::from16(dr[c]);
            if (sc != nullptr) g *= 1.0f + sc[c];
            if (ln_w != nullptr) g *= ln_w[c];
            dx[(size_t)row * C + c] = (dres != nullptr ? dres[(size_t)row * C + c] : 0.f) + rstd * (g - c1 - xh * c2);
        }
        if (lane == 0) { s_mean[row - r0] = mean; s_lo[row - r0] = mean_lo; s_rstd[row - r0] = rstd; }
    }
    if (p_shift == nullptr && p_w == nullptr) return;
    __syncthreads();
    for (int c = tid; c < C; c += 256) {
        const float w = ln_w != nullptr ? ln_w[c] : 1.f, b = ln_w != nullptr ? ln_b[c] : 0.f;
        float aw = 0.f, ab = 0.f;
        for (long long g = g_lo; g <= g_hi; ++g) {
            const long long s0 = seg_lo(r0, g, rpg), s1 = seg_hi(r1, g, rpg);
            const float m = scale != nullptr ? 1.0f + scale[(size_t)g * mod_ld + c] : 1.f;
            float as = 0.f, ac = 0.f;
            for (long long row = s0; row < s1; ++row) {
                const float xh = ((x[(size_t)row * C + c] - s_mean[row - r0]) - s_lo[row - r0]) * s_rstd[row - r0];
                const float d = GvfLp<DT>::from16(dy[(size_t)row * C + c]);
                const float gm = d * m;
                as += d;
                ac += d * (xh * w + b);
                aw += gm * xh;
                ab += gm;
            }
            if (p_shift != nullptr) {
                p_shift[(size_t)(blockIdx.x + g) * C + c] = as;
                p_scale[(size_t)(blockIdx.x + g) * C + c] = ac;
            }
        }
        if (p_w != nullptr) {
            p_w[(size_t)blockIdx.x * C + c] = aw;
            p_b[(size_t)blockIdx.x * C + c] = ab;
        }
    }
}

// ---- b. gated residual ------------------------------------------------------------------------------------------------------------------
template <int VPL, int DT>
__global__ __launch_bounds__(256) void gate_fwd_kernel(const float* __restrict__ x, const unsigned short* __restrict__ h, const float* __restrict__ gate,
                                                       int gate_ld, long long rpg, float* __restrict__ out, int rows) {
    constexpr int C = 256 * VPL;
    const int lane = threadIdx.x & 63;
    const long long row = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= rows) return;
    const float4* xr = reinterpret_cast<const float4*>(x + (size_t)row * C);
    const uint2* hr = reinterpret_cast<const uint2*>(h + (size_t)row * C);
    float4* orow = reinterpret_cast<float4*>(out + (size_t)row * C);
    const float* gr = gate != nullptr ? gate + (size_t)(row / rpg) * gate_ld : nullptr;
#pragma unroll
    for (int i = 0; i < VPL; ++i) {
        const float4 v = xr[lane + 64 * i];
        float f[4];
        unpack4<DT>(hr[lane + 64 * i], f);
        float4 g4 = make_float4(1.f, 1.f, 1.f, 1.f);
        if (gr != nullptr) g4 = *reinterpret_cast<const float4*>(gr + (lane + 64 * i) * 4);
        orow[lane + 64 * i] = make_float4(v.x + g4.x * f[0], v.y + g4.y * f[1], v.z + g4.z * f[2], v.w + g4.w * f[3]);
    }
}

template <int DT>
__global__ __launch_bounds__(256) void gate_fwd_generic_kernel(const float* __restrict__ x, const unsigned short* __restrict__ h, const float* __restrict__ gate,
                                                               int gate_ld, long long rpg, float* __restrict__ out, int rows, int C) {
    const int lane = threadIdx.x & 63;
    const long long row = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= rows) return;
    const float* gr = gate != nullptr ? gate + (size_t)(row / rpg) * gate_ld : nullptr;
    for (int c = lane; c < C; c += 64) {
        const float f = GvfLp<DT>::from16(h[(size_t)row * C + c]);
        out[(size_t)row * C + c] = x[(size_t)row * C + c] + (gr != nullptr ? gr[c] * f : f);
    }
}

template <int VPL, int DT>
__global__ __launch_bounds__(256) void gate_bwd_kernel(const float* __restrict__ dout, const unsigned short* __restrict__ h, const float* __restrict__ gate,
                                                       int gate_ld, long long rpg, unsigned short* __restrict__ dh, int rows, float* __restrict__ p_gate) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    constexpr int C = 256 * VPL;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const long long r0 = (long long)blockIdx.x * RPW, r1 = r0 + RPW < rows ? r0 + RPW : rows;
    const long long g_lo = r0 / rpg, g_hi = (r1 - 1) / rpg;
    for (long long g = g_lo; g <= g_hi; ++g) {
        const long long s0 = seg_lo(r0, g, rpg), s1 = seg_hi(r1, g, rpg);
        float gt[VPL][4], acc[VPL][4];
#pragma unroll
        for (int i = 0; i < VPL; ++i) {
            float4 g4 = make_float4(1.f, 1.f, 1.f, 1.f);
            if (gate != nullptr) g4 = *reinterpret_cast<const float4*>(gate + (size_t)g * gate_ld + (lane + 64 * i) * 4);
            gt[i][0] = g4.x; gt[i][1] = g4.y; gt[i][2] = g4.z; gt[i][3] = g4.w;
#pragma unroll
            for (int e = 0; e < 4; ++e) acc[i][e] = 0.f;
        }
        for (long long row = s0 + wave; row < s1; row += 4) {
            const float4* dr = reinterpret_cast<const float4*>(dout + (size_t)row * C);
            const uint2* hr = reinterpret_cast<const uint2*>(h + (size_t)row * C);
            uint2* o = reinterpret_cast<uint2*>(dh + (size_t)row * C);
#pragma unroll
            for (int i = 0; i < VPL; ++i) {
                const float4 d = dr[lane + 64 * i];
                if (gate != nullptr) {
                    float f[4];
                    unpack4<DT>(hr[lane + 64 * i], f);
                    acc[i][0] += d.x * f[0]; acc[i][1] += d.y * f[1]; acc[i][2] += d.z * f[2]; acc[i][3] += d.w * f[3];
                }
                uint2 q;
                q.x = GvfLp<DT>::pack(gt[i][0] * d.x, gt[i][1] * d.y);
                q.y = GvfLp<DT>::pack(gt[i][2] * d.z, gt[i][3] * d.w);
                o[lane + 64 * i] = q;
            }
        }
        if (p_gate != nullptr) flush_cols<VPL>(acc, lds, p_gate + (size_t)(blockIdx.x + g) * C, C, lane, wave, tid);
    }
}

// any C: a thread owns columns tid, tid + 256, ... of the workgroup's rows
template <int DT>
__global__ __launch_bounds__(256) void gate_bwd_generic_kernel(const float* __restrict__ dout, const unsigned short* __restrict__ h, const float* __restrict__ gate,
                                                               int gate_ld, long long rpg, unsigned short* __restrict__ dh, int rows, int C,
                                                               float* __restrict__ p_gate) {
    const int tid = threadIdx.x;
    const long long r0 = (long long)blockIdx.x * RPW, r1 = r0 + RPW < rows ? r0 + RPW : rows;
    const long long g_lo = r0 / rpg, g_hi = (r1 - 1) / rpg;
    for (int c = tid; c < C; c += 256) {
        for (long long g = g_lo; g <= g_hi; ++g) {
            const long long s0 = seg_lo(r0, g, rpg), s1 = seg_hi(r1, g, rpg);
            const float gt = gate != nullptr ? gate[(size_t)g * gate_ld + c] : 1.f;
            float acc = 0.f;
            for (long long row = s0; row < s1; ++row) {
                const float d = dout[(size_t)row * C + c];
                if (gate != nullptr) acc += d * GvfLp<DT>::from16(h[(size_t)row * C + c]);
                dh[(size_t)row * C + c] = GvfLp<DT>::to16(gt * d);
            }
            if (p_gate != nullptr) p_gate[(size_t)(blockIdx.x + g) * C + c] = acc;
        }
    }
}

// ---- c. multi-head RMSNorm --------------------------------------------------------------------------------------------------------------
// A lane holds 8 consecutive channels (16 bytes), D / 8 lanes a head, a wave 512 channels per trip; HD = H * D is a multiple of 32, so a
// lane's 8 channels are all inside the row or all outside.
__device__ __forceinline__ void load8(const float* p, float (&f)[8]) {
    const float4 a = *reinterpret_cast<const float4*>(p), b = *reinterpret_cast<const float4*>(p + 4);
    f[0] = a.x; f[1] = a.y; f[2] = a.z; f[3] = a.w; f[4] = b.x; f[5] = b.y; f[6] = b.z; f[7] = b.w;
}

template <int D, int DT>
__global__ __launch_bounds__(256) void rms_fwd_kernel(const unsigned short* __restrict__ x, long long ldx, const float* __restrict__ gamma,
                                                      unsigned short* __restrict__ y, long long ldy, int rows, int HD) {
    const int lane = threadIdx.x & 63;
    const long long row = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= rows) return;
    const float sqrt_d = D == 32 ? 5.656854249492381f : 8.0f;
    for (int base = 0; base < HD; base += 512) {
        const int c0 = base + lane * 8;
        const bool on = c0 < HD;
        float f[8], gm[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) f[e] = gm[e] = 0.f;
        if (on) {
            gvf_unpack8<DT>(*reinterpret_cast<const uint4*>(x + (size_t)row * ldx + c0), f);
            load8(gamma + c0, gm);
        }
        float ss = 0.f;
#pragma unroll
        for (int e = 0; e < 8; ++e) ss += f[e] * f[e];
        const float den = fmaxf(sqrtf(group_sum<D / 8>(ss)), 1e-12f);
        float o[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) o[e] = ((f[e] / den) * gm[e]) * sqrt_d;
        if (on) *reinterpret_cast<uint4*>(y + (size_t)row * ldy + c0) = gvf_pack8<DT>(o);
    }
}

// NCH = trips of 512 channels: HD <= 512 NCH
template <int D, int NCH, int DT>
__global__ __launch_bounds__(256) void rms_bwd_kernel(const unsigned short* __restrict__ x, long long ldx, const unsigned short* __restrict__ dy, long long lddy,
                                                      const float* __restrict__ gamma, unsigned short* __restrict__ dx, long long lddx, int rows, int HD,
                                                      float* __restrict__ p_gamma) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const long long r0 = (long long)blockIdx.x * RPW, r1 = r0 + RPW < rows ? r0 + RPW : rows;
    const float sqrt_d = D == 32 ? 5.656854249492381f : 8.0f;
    float gm[NCH][8], acc[NCH][8];
#pragma unroll
    for (int j = 0; j < NCH; ++j) {
        const int c0 = j * 512 + lane * 8;
#pragma unroll
        for (int e = 0; e < 8; ++e) gm[j][e] = acc[j][e] = 0.f;
        if (c0 < HD) load8(gamma + c0, gm[j]);
    }
    for (long long row = r0 + wave; row < r1; row += 4) {
#pragma unroll
        for (int j = 0; j < NCH; ++j) {
            const int c0 = j * 512 + lane * 8;
            const bool on = c0 < HD;
            float f[8], d[8];
#pragma unroll
            for (int e = 0; e < 8; ++e) f[e] = d[e] = 0.f;
            if (on) {
                gvf_unpack8<DT>(*reinterpret_cast<const uint4*>(x + (size_t)row * ldx + c0), f);
                gvf_unpack8<DT>(*reinterpret_cast<const uint4*>(dy + (size_t)row * lddy + c0), d);
            }
            float ss = 0.f;
#pragma unroll
            for (int e = 0; e < 8; ++e) ss += f[e] * f[e];
            const float den = fmaxf(sqrtf(group_sum<D / 8>(ss)), 1e-12f);
            float xt[8], u[8], dot = 0.f;
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                xt[e] = f[e] / den;
                u[e] = (d[e] * gm[j][e]) * sqrt_d;
                dot += u[e] * xt[e];
                acc[j][e] += d[e] * xt[e];
            }
            dot = group_sum<D / 8>(dot);
            float o[8];
#pragma unroll
            for (int e = 0; e < 8; ++e) o[e] = (u[e] - xt[e] * dot) / den;
            if (on) *reinterpret_cast<uint4*>(dx + (size_t)row * lddx + c0) = gvf_pack8<DT>(o);
        }
    }
    // the four waves' partials -> slot blockIdx.x (waves in order); lds: 4 * HD floats
#pragma unroll
    for (int j = 0; j < NCH; ++j) {
        const int c0 = j * 512 + lane * 8;
        if (c0 < HD) {
            float* p = lds + (size_t)wave * HD + c0;
            *reinterpret_cast<float4*>(p) = make_float4(acc[j][0], acc[j][1], acc[j][2], acc[j][3]);
            *reinterpret_cast<float4*>(p + 4) = make_float4(acc[j][4], acc[j][5], acc[j][6], acc[j][7]);
        }
    }
    __syncthreads();
    float* dst = p_gamma + (size_t)blockIdx.x * HD;
    for (int c = tid; c < HD; c += 256) dst[c] = ((lds[c] + lds[HD + c]) + lds[2 * HD + c]) + lds[3 * HD + c];
}

// ---- the column-sum finaliser of all three families ----------------------------------------------------------------------------------
// out[g, c] = factor * sum over the slots of group g, in slot order: thread (cx, k) adds slots lo + k, lo + k + 4, ... and the four k are
// combined as (0 + 1) + (2 + 3).  Up to four outputs of one width per launch (blockIdx.z).
struct ColsumJob { const float* part; float* out; long long G; long long rpg; float factor; };
struct ColsumJobs { ColsumJob j[4]; };

__global__ __launch_bounds__(256) void colsum_finalize_kernel(ColsumJobs jobs, int n_cols, long long rows) {
    __shared__ float red[4][64];
    const ColsumJob J = jobs.j[blockIdx.z];
    const int cx = threadIdx.x & 63, k = threadIdx.x >> 6;
    const int c = blockIdx.x * 64 + cx;
    for (long long g = blockIdx.y; g < J.G; g += gridDim.y) {
        const long long last = ((g + 1) * J.rpg < rows ? (g + 1) * J.rpg : rows) - 1;
        const long long lo = (g * J.rpg) / RPW + g, hi = last / RPW + g;
        float s = 0.f;
        if (c < n_cols)
            for (long long w = lo + k; w <= hi; w += 4) s += J.part[(size_t)w * n_cols + c];
        red[k][cx] = s;
        __syncthreads();
        if (k == 0 && c < n_cols) J.out[(size_t)g * n_cols + c] = ((red[0][cx] + red[1][cx]) + (red[2][cx] + red[3][cx])) * J.factor;
        __syncthreads();
    }
}

inline long long n_wg(long long rows) { return (rows + RPW - 1) / RPW; }
inline long long n_groups(long long rows, long long rpg) { return (rows + rpg - 1) / rpg; }
inline bool vec_path(int C) { return (C % 256) == 0 && C <= 1024; }

int launch_finalize(const ColsumJobs& jobs, int n_jobs, long long max_G, int n_cols, long long rows, hipStream_t stream) {
    const dim3 grid((n_cols + 63) / 64, (unsigned)(max_G < 1024 ? max_G : 1024), n_jobs);
    hipLaunchKernelGGL(colsum_finalize_kernel, grid, dim3(256), 0, stream, jobs, n_cols, rows);
    GVF_CHECK_LAUNCH();
    return GVF_OK;
}

}  // namespace

extern "C" int gvf_ln_mod_bwd_workspace_bytes(int rows, int C, int rows_per_group, size_t* out) {
    if (!out || rows < 0 || C <= 0 || rows_per_group < 0) return GVF_EINVAL;
    const long long rpg = rows_per_group > 0 ? rows_per_group : (rows > 0 ? rows : 1);
    const long long W = n_wg(rows), G = rows > 0 ? n_groups(rows, rpg) : 0;
    *out = (size_t)(2 * (W + G) + 2 * W) * (size_t)C * sizeof(float);
    return GVF_OK;
}

extern "C" int gvf_ln_mod_bwd(int dtype, const float* x, const void* dy, const float* dres, float* dx, int rows, int C, float eps,
                              const float* ln_w, const float* ln_b, const float* scale, int mod_ld, int rows_per_group,
                              float* dshift, float* dscale, float* dw, float* db, void* workspace, size_t workspace_bytes, void* stream_) {
    if (!gvf_lp_ok(dtype)) return GVF_EINVAL;
    if (rows < 0 || C <= 0) return GVF_EINVAL;
    if (rows == 0) return GVF_OK;
    if (!x || !dy || !dx) return GVF_EINVAL;
    if ((ln_w == nullptr) != (ln_b == nullptr) || (dw == nullptr) != (ln_w == nullptr) || (db == nullptr) != (ln_w == nullptr)) return GVF_EINVAL;
    if ((dshift == nullptr) != (scale == nullptr) || (dscale == nullptr) != (scale == nullptr)) return GVF_EINVAL;
    if (scale != nullptr && (rows_per_group <= 0 || mod_ld < C)) return GVF_EINVAL;
    const bool vec = vec_path(C);
    if (vec && (gvf_mis(x, 15) || gvf_mis(dx, 15) || gvf_mis(dres, 15) || gvf_mis(dy, 7) || gvf_mis(ln_w, 15) || gvf_mis(ln_b, 15) || gvf_mis(scale, 15) ||
                (scale != nullptr && (mod_ld % 4) != 0)))
        return GVF_EINVAL;
    const bool sums = scale != nullptr || ln_w != nullptr;
    size_t need = 0;
    if (gvf_ln_mod_bwd_workspace_bytes(rows, C, scale != nullptr ? rows_per_group : 0, &need) != GVF_OK) return GVF_EINVAL;
    if (sums && (!workspace || workspace_bytes < need || gvf_mis(workspace, 15))) return GVF_EINVAL;
    hipStream_t stream = (hipStream_t)stream_;
    (void)hipGetLastError();
    const long long rpg = scale != nullptr ? rows_per_group : rows;
    const long long W = n_wg(rows), G = n_groups(rows, rpg);
    float* ws = (float*)workspace;
    float* p_shift = scale != nullptr ? ws : nullptr;
    float* p_scale = scale != nullptr ? ws + (size_t)(W + G) * C : nullptr;
    float* p_w = ln_w != nullptr ? ws + (size_t)2 * (W + G) * C : nullptr;
    float* p_b = ln_w != nullptr ? ws + (size_t)(2 * (W + G) + W) * C : nullptr;
    const dim3 grid((unsigned)W), block(256);
    const unsigned short* d16 = (const unsigned short*)dy;
    GVF_LP_DISPATCH(dtype,
        if (!vec) {
            hipLaunchKernelGGL(ln_bwd_generic_kernel<DT>, grid, block, 0, stream, x, d16, dres, dx, rows, C, eps, ln_w, ln_b, scale, mod_ld, rpg, p_shift, p_scale, p_w, p_b);
        } else {
            const size_t sh = (size_t)4 * C * sizeof(float);
            switch (C / 256) {
                case 1: hipLaunchKernelGGL((ln_bwd_kernel<1, DT>), grid, block, sh, stream, x, d16, dres, dx, rows, eps, ln_w, ln_b, scale, mod_ld, rpg, p_shift, p_scale, p_w, p_b); break;
                case 2: hipLaunchKernelGGL((ln_bwd_kernel<2, DT>), grid, block, sh, stream, x, d16, dres, dx, rows, eps, ln_w, ln_b, scale, mod_ld, rpg, p_shift, p_scale, p_w, p_b); break;
                case 3: hipLaunchKernelGGL((ln_bwd_kernel<3, DT>), grid, block, sh, stream, x, d16, dres, dx, rows, eps, ln_w, ln_b, scale, mod_ld, rpg, p_shift, p_scale, p_w, p_b); break;
                default: hipLaunchKernelGGL((ln_bwd_kernel<4, DT>), grid, block, sh, stream, x, d16, dres, dx, rows, eps, ln_w, ln_b, scale, mod_ld, rpg, p_shift, p_scale, p_w, p_b); break;
            }
        });
    GVF_CHECK_LAUNCH();
    if (!sums) return GVF_OK;
    ColsumJobs jobs = {};
    int n = 0;
    if (scale != nullptr) {
        jobs.j[n++] = ColsumJob{p_shift, dshift, G, rpg, 1.0f};
        jobs.j[n++] = ColsumJob{p_scale, dscale, G, rpg, 1.0f};
    }
    if (ln_w != nullptr) {
        jobs.j[n++] = ColsumJob{p_w, dw, 1, (long long)rows, 1.0f};
        jobs.j[n++] = ColsumJob{p_b, db, 1, (long long)rows, 1.0f};
    }
    return launch_finalize(jobs, n, scale != nullptr ? G : 1, C, rows, stream);
}

extern "C" int gvf_gate_residual_fwd(int dtype, const float* x, const void* h, const float* gate, int gate_ld, int rows_per_group, float* out,
                                     int rows, int C, void* stream_) {
    if (!gvf_lp_ok(dtype)) return GVF_EINVAL;
    if (rows < 0 || C <= 0) return GVF_EINVAL;
    if (rows == 0) return GVF_OK;
    if (!x || !h || !out) return GVF_EINVAL;
    if (gate != nullptr && (rows_per_group <= 0 || gate_ld < C)) return GVF_EINVAL;
    const bool vec = vec_path(C);
    if (vec && (gvf_mis(x, 15) || gvf_mis(out, 15) || gvf_mis(h, 7) || gvf_mis(gate, 15) || (gate != nullptr && (gate_ld % 4) != 0))) return GVF_EINVAL;
    hipStream_t stream = (hipStream_t)stream_;
    (void)hipGetLastError();
    const long long rpg = gate != nullptr ? rows_per_group : rows;
    const dim3 grid((unsigned)((rows + 3) / 4)), block(256);
    const unsigned short* h16 = (const unsigned short*)h;
    GVF_LP_DISPATCH(dtype,
        if (!vec) {
            hipLaunchKernelGGL(gate_fwd_generic_kernel<DT>, grid, block, 0, stream, x, h16, gate, gate_ld, rpg, out, rows, C);
        } else {
            switch (C / 256) {
                case 1: hipLaunchKernelGGL((gate_fwd_kernel<1, DT>), grid, block, 0, stream, x, h16, gate, gate_ld, rpg, out, rows); break;
                case 2: hipLaunchKernelGGL((gate_fwd_kernel<2, DT>), grid, block, 0, stream, x, h16, gate, gate_ld, rpg, out, rows); break;
                case 3: hipLaunchKernelGGL((gate_fwd_kernel<3, DT>), grid, block, 0, stream, x, h16, gate, gate_ld, rpg, out, rows); break;
                default: hipLaunchKernelGGL((gate_fwd_kernel<4, DT>), grid, block, 0, stream, x, h16, gate, gate_ld, rpg, out, rows); break;
            }
        });
    GVF_CHECK_LAUNCH();
    return GVF_OK;
}

extern "C" int gvf_gate_residual_bwd_workspace_bytes(int rows, int C, int rows_per_group, size_t* out) {
    if (!out || rows < 0 || C <= 0 || rows_per_group < 0) return GVF_EINVAL;
    const long long rpg = rows_per_group > 0 ? rows_per_group : (rows > 0 ? rows : 1);
    const long long W = n_wg(rows), G = rows > 0 ? n_groups(rows, rpg) : 0;
    *out = (size_t)(W + G) * (size_t)C * sizeof(float);
    return GVF_OK;
}

extern "C" int gvf_gate_residual_bwd(int dtype, const float* dout, const void* h, const float* gate, int gate_ld, int rows_per_group, void* dh,
                                     float* dgate, int rows, int C, void* workspace, size_t workspace_bytes, void* stream_) {
    if (!gvf_lp_ok(dtype)) return GVF_EINVAL;
    if (rows < 0 || C <= 0) return GVF_EINVAL;
    if (rows == 0) return GVF_OK;
    if (!dout || !dh) return GVF_EINVAL;
    if ((dgate == nullptr) != (gate == nullptr)) return GVF_EINVAL;
    if (gate != nullptr && (!h || rows_per_group <= 0 || gate_ld < C)) return GVF_EINVAL;
    const bool vec = vec_path(C);
    if (vec && (gvf_mis(dout, 15) || gvf_mis(dh, 7) || gvf_mis(h, 7) || gvf_mis(gate, 15) || (gate != nullptr && (gate_ld % 4) != 0))) return GVF_EINVAL;
    size_t need = 0;
    if (gvf_gate_residual_bwd_workspace_bytes(rows, C, gate != nullptr ? rows_per_group : 0, &need) != GVF_OK) return GVF_EINVAL;
    if (gate != nullptr && (!workspace || workspace_bytes < need || gvf_mis(workspace, 15))) return GVF_EINVAL;
    hipStream_t stream = (hipStream_t)stream_;
    (void)hipGetLastError();
    const long long rpg = gate != nullptr ? rows_per_group : rows;
    const long long W = n_wg(rows), G = n_groups(rows, rpg);
    float* p_gate = gate != nullptr ? (float*)workspace : nullptr;
    const dim3 grid((unsigned)W), block(256);
    const unsigned short* h16 = (const unsigned short*)h;
    unsigned short* o16 = (unsigned short*)dh;
    GVF_LP_DISPATCH(dtype,
        if (!vec) {
            hipLaunchKernelGGL(gate_bwd_generic_kernel<DT>, grid, block, 0, stream, dout, h16, gate, gate_ld, rpg, o16, rows, C, p_gate);
        } else {
            const size_t sh = (size_t)4 * C * sizeof(float);
            switch (C / 256) {
                case 1: hipLaunchKernelGGL((gate_bwd_kernel<1, DT>), grid, block, sh, stream, dout, h16, gate, gate_ld, rpg, o16, rows, p_gate); break;
                case 2: hipLaunchKernelGGL((gate_bwd_kernel<2, DT>), grid, block, sh, stream, dout, h16, gate, gate_ld, rpg, o16, rows, p_gate); break;
                case 3: hipLaunchKernelGGL((gate_bwd_kernel<3, DT>), grid, block, sh, stream, dout, h16, gate, gate_ld, rpg, o16, rows, p_gate); break;
                default: hipLaunchKernelGGL((gate_bwd_kernel<4, DT>), grid, block, sh, stream, dout, h16, gate, gate_ld, rpg, o16, rows, p_gate); break;
            }
        });
    GVF_CHECK_LAUNCH();
    if (gate == nullptr) return GVF_OK;
    ColsumJobs jobs = {};
    jobs.j[0] = ColsumJob{p_gate, dgate, G, rpg, 1.0f};
    return launch_finalize(jobs, 1, G, C, rows, stream);
}

static int rms_args_ok(int dtype, int rows, int H, int d) {
    if (!gvf_lp_ok(dtype)) return 0;
    if (rows < 0 || H <= 0 || (d != 32 && d != 64)) return 0;
    if ((long long)H * d > 2048) return 0;
    return 1;
}

extern "C" int gvf_rmsnorm_heads_fwd(int dtype, const void* x, int64_t ldx, const float* gamma, void* y, int64_t ldy, int rows, int H, int d,
                                     void* stream_) {
    if (!rms_args_ok(dtype, rows, H, d)) return GVF_EINVAL;
    if (rows == 0) return GVF_OK;
    const int HD = H * d;
    if (!x || !gamma || !y) return GVF_EINVAL;
    if (ldx < HD || ldy < HD || (ldx % 8) != 0 || (ldy % 8) != 0 || gvf_mis(x, 15) || gvf_mis(y, 15) || gvf_mis(gamma, 15)) return GVF_EINVAL;
    hipStream_t stream = (hipStream_t)stream_;
    (void)hipGetLastError();
    const dim3 grid((unsigned)((rows + 3) / 4)), block(256);
    const unsigned short* x16 = (const unsigned short*)x;
    unsigned short* y16 = (unsigned short*)y;
    GVF_LP_DISPATCH(dtype,
        if (d == 32) hipLaunchKernelGGL((rms_fwd_kernel<32, DT>), grid, block, 0, stream, x16, (long long)ldx, gamma, y16, (long long)ldy, rows, HD);
        else hipLaunchKernelGGL((rms_fwd_kernel<64, DT>), grid, block, 0, stream, x16, (long long)ldx, gamma, y16, (long long)ldy, rows, HD));
    GVF_CHECK_LAUNCH();
    return GVF_OK;
}

extern "C" int gvf_rmsnorm_heads_bwd_workspace_bytes(int rows, int H, int d, size_t* out) {
    if (!out || rows < 0 || H <= 0 || (d != 32 && d != 64) || (long long)H * d > 2048) return GVF_EINVAL;
    *out = (size_t)n_wg(rows) * (size_t)(H * d) * sizeof(float);
    return GVF_OK;
}

extern "C" int gvf_rmsnorm_heads_bwd(int dtype, const void* x, int64_t ldx, const void* dy, int64_t lddy, const float* gamma, void* dx, int64_t lddx,
                                     float* dgamma, int rows, int H, int d, void* workspace, size_t workspace_bytes, void* stream_) {
    if (!rms_args_ok(dtype, rows, H, d)) return GVF_EINVAL;
    if (rows == 0) return GVF_OK;
    const int HD = H * d;
    if (!x || !dy || !gamma || !dx || !dgamma || !workspace) return GVF_EINVAL;
    if (ldx < HD || lddy < HD || lddx < HD || (ldx % 8) != 0 || (lddy % 8) != 0 || (lddx % 8) != 0 || gvf_mis(x, 15) || gvf_mis(dy, 15) || gvf_mis(dx, 15) ||
        gvf_mis(gamma, 15) || gvf_mis(workspace, 15))
        return GVF_EINVAL;
    size_t need = 0;
    if (gvf_rmsnorm_heads_bwd_workspace_bytes(rows, H, d, &need) != GVF_OK || workspace_bytes < need) return GVF_EINVAL;
    hipStream_t stream = (hipStream_t)stream_;
    (void)hipGetLastError();
    const long long W = n_wg(rows);
    const dim3 grid((unsigned)W), block(256);
    const size_t sh = (size_t)4 * HD * sizeof(float);
    const unsigned short* x16 = (const unsigned short*)x;
    const unsigned short* d16 = (const unsigned short*)dy;
    unsigned short* o16 = (unsigned short*)dx;
    float* part = (float*)workspace;
    const int nch = (HD + 511) / 512;
#define GVF_RMS_BWD(D_, N_) hipLaunchKernelGGL((rms_bwd_kernel<D_, N_, DT>), grid, block, sh, stream, x16, (long long)ldx, d16, (long long)lddy, gamma, o16, \
                                               (long long)lddx, rows, HD, part)
    GVF_LP_DISPATCH(dtype,
        if (d == 32) { if (nch == 1) GVF_RMS_BWD(32, 1); else if (nch == 2) GVF_RMS_BWD(32, 2); else GVF_RMS_BWD(32, 4); }
        else { if (nch == 1) GVF_RMS_BWD(64, 1); else if (nch == 2) GVF_RMS_BWD(64, 2); else GVF_RMS_BWD(64, 4); });
#undef GVF_RMS_BWD
    GVF_CHECK_LAUNCH();
    ColsumJobs jobs = {};
    jobs.j[0] = ColsumJob{part, dgamma, 1, (long long)rows, d == 32 ? 5.656854249492381f : 8.0f};
    return launch_finalize(jobs, 1, 1, HD, rows, stream);
}
