// lpips.hip -- the non-convolution layers of the LPIPS trunk on NHWC 16-bit activations, gfx950: 2x2 max pool forward, its backward
// fused with the tap gradient and the ReLU mask, and the tap (normalise, squared difference, lin weight, pixel mean) forward and
// backward.  C ABI and formulas: include/gvf_lpips.h.
//
// Pool kernels: one thread per pixel and 8 channels (one 16-byte load per window element).
// Tap kernels: one wave per pixel; lane l holds the channel pairs l, l + 64, ... (4-byte loads, a pixel's channels are contiguous).  The
// per-pixel arithmetic is in double -- the kernels are bound by the two activation reads, and the result then carries the rounding of
// the stored activations only.  Forward: per-lane double sums over the wave's pixels, one double partial per workgroup, and one
// workgroup per image adds the partials in a fixed order (no float atomics: bit-identical run to run).
#include "gvf_common.h"
#include "gvf_lp.h"
#include "gvf_rowops.h"
#include "../../include/gvf_rast.h"
#include "../../include/gvf_dit.h"
#include "../../include/gvf_lpips.h"

namespace {

constexpr int NT = 256;
constexpr int WAVES = NT / GVF_WAVE;
constexpr int MAXW = 4;                 // channel pairs per lane: 512 / 2 / 64
constexpr int TAP_MAX_BLOCKS = 512;     // workgroups per image of the tap kernels

__device__ __forceinline__ bool positive16(unsigned short h) { return h != 0 && !(h & 0x8000u); }

// ---- pool ------------------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ unsigned short half_of(const uint4& v, int e) {
    const unsigned w = e < 2 ? v.x : (e < 4 ? v.y : (e < 6 ? v.z : v.w));
    return (unsigned short)((e & 1) ? (w >> 16) : (w & 0xffffu));
}

// index (0..3, row-major in the window) of the first maximum of channel e
__device__ __forceinline__ int argmax4(const float (&f)[4][8], int e) {
    int k = 0;
    float m = f[0][e];
#pragma unroll
    for (int i = 1; i < 4; ++i)
        if (f[i][e] > m) {
            m = f[i][e];
            k = i;
        }
    return k;
}

template <int DT>
__global__ __launch_bounds__(NT) void pool_fwd_kernel(const unsigned short* __restrict__ in, unsigned short* __restrict__ out, int H, int W,
                                                      int C, int64_t total) {
    const int Ho = H / 2, Wo = W / 2, C8 = C / 8;
    for (int64_t i = (int64_t)blockIdx.x * NT + threadIdx.x; i < total; i += (int64_t)gridDim.x * NT) {
        const int c8 = (int)(i % C8);
        int64_t p = i / C8;
        const int xo = (int)(p % Wo);
        p /= Wo;
        const int yo = (int)(p % Ho);
        const int64_t n = p / Ho;
        uint4 v[4];
        float f[4][8];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            v[k] = *(const uint4*)(in + ((n * H + 2 * yo + (k >> 1)) * W + 2 * xo + (k & 1)) * C + 8 * c8);
            gvf_unpack8<DT>(v[k], f[k]);
        }
        unsigned short r[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const int k = argmax4(f, e);
            r[e] = half_of(k == 0 ? v[0] : (k == 1 ? v[1] : (k == 2 ? v[2] : v[3])), e);
        }
        uint4 o;
        o.x = r[0] | ((unsigned)r[1] << 16); o.y = r[2] | ((unsigned)r[3] << 16);
        o.z = r[4] | ((unsigned)r[5] << 16); o.w = r[6] | ((unsigned)r[7] << 16);
        *(uint4*)(out + ((n * Ho + yo) * Wo + xo) * C + 8 * c8) = o;
    }
}

template <int DT>
__global__ __launch_bounds__(NT) void pool_bwd_kernel(const unsigned short* __restrict__ a, const unsigned short* __restrict__ gp,
                                                      const unsigned short* __restrict__ tg, unsigned short* __restrict__ z, int H, int W,
                                                      int C, int64_t total) {
    typedef GvfLp<0> G;                                   // gradients are bf16
    const int Ho = H / 2, Wo = W / 2, C8 = C / 8;
    for (int64_t i = (int64_t)blockIdx.x * NT + threadIdx.x; i < total; i += (int64_t)gridDim.x * NT) {
        const int c8 = (int)(i % C8);
        int64_t p = i / C8;
        const int x = (int)(p % W);
        p /= W;
        const int y = (int)(p % H);
        const int64_t n = p / H;
        const int64_t o = ((n * H + y) * W + x) * C + 8 * c8;
        const uint4 own = *(const uint4*)(a + o);
        float t[8], g[8];
        gvf_unpack8<0>(*(const uint4*)(tg + o), t);
        bool mine[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            mine[e] = false;
            g[e] = 0.f;
        }
        const int yo = y >> 1, xo = x >> 1;
        if (yo < Ho && xo < Wo) {
            float f[4][8];
#pragma unroll
            for (int k = 0; k < 4; ++k)
                gvf_unpack8<DT>(*(const uint4*)(a + ((n * H + 2 * yo + (k >> 1)) * W + 2 * xo + (k & 1)) * C + 8 * c8), f[k]);
            gvf_unpack8<0>(*(const uint4*)(gp + ((n * Ho + yo) * Wo + xo) * C + 8 * c8), g);
            const int me = ((y & 1) << 1) | (x & 1);
#pragma unroll
            for (int e = 0; e < 8; ++e) mine[e] = argmax4(f, e) == me;
        }
        float r[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const float v = mine[e] ? g[e] + t[e] : t[e];
            r[e] = positive16(half_of(own, e)) ? v : 0.f;
        }
        uint4 w;
        w.x = G::pack(r[0], r[1]); w.y = G::pack(r[2], r[3]); w.z = G::pack(r[4], r[5]); w.w = G::pack(r[6], r[7]);
        *(uint4*)(z + o) = w;
    }
}

// ---- taps ------------------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
    for (int off = GVF_WAVE / 2; off > 0; off >>= 1) v += __shfl_xor(v, off, GVF_WAVE);
    return v;                                             // the same value in every lane (a butterfly: a fixed order)
}

__device__ __forceinline__ double block_sum(double v, double* red) {
    v = wave_sum(v);
    if ((threadIdx.x & (GVF_WAVE - 1)) == 0) red[threadIdx.x / GVF_WAVE] = v;
    __syncthreads();
    double s = 0.0;
    if (threadIdx.x == 0)
        for (int w = 0; w < WAVES; ++w) s += red[w];
    __syncthreads();
    return s;   // valid in thread 0
}

// one pixel of both images: u = ax / (|ax| + eps), v = ay / (|ay| + eps) of this lane's channels; returns |ax| and D = |ax| + eps
template <int DT>
struct Pixel {
    double u[MAXW][2], v[MAXW][2], ax[MAXW][2];
    double rx, dxn;
    __device__ __forceinline__ void load(const unsigned* __restrict__ px, const unsigned* __restrict__ py, int nw, int lane) {
        typedef GvfLp<DT> L;
        double sx = 0.0, sy = 0.0;
#pragma unroll
        for (int i = 0; i < MAXW; ++i) {
            const int wd = lane + GVF_WAVE * i;
            const unsigned a = wd < nw ? px[wd] : 0u, b = wd < nw ? py[wd] : 0u;
            ax[i][0] = (double)L::lo(a); ax[i][1] = (double)L::hi(a);
            v[i][0] = (double)L::lo(b); v[i][1] = (double)L::hi(b);
            sx += ax[i][0] * ax[i][0] + ax[i][1] * ax[i][1];
            sy += v[i][0] * v[i][0] + v[i][1] * v[i][1];
        }
        rx = sqrt(wave_sum(sx));
        dxn = rx + 1e-10;
        const double dyn = sqrt(wave_sum(sy)) + 1e-10;
#pragma unroll
        for (int i = 0; i < MAXW; ++i)
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                u[i][h] = ax[i][h] / dxn;
                v[i][h] = v[i][h] / dyn;
            }
    }
};

__device__ __forceinline__ void load_lin(const float* __restrict__ lin, int nw, int lane, double (&l)[MAXW][2]) {
#pragma unroll
    for (int i = 0; i < MAXW; ++i) {
        const int wd = lane + GVF_WAVE * i;
        l[i][0] = wd < nw ? (double)lin[2 * wd] : 0.0;
        l[i][1] = wd < nw ? (double)lin[2 * wd + 1] : 0.0;
    }
}

template <int DT>
__global__ __launch_bounds__(NT) void tap_fwd_kernel(const unsigned* __restrict__ ax, const unsigned* __restrict__ ay, const float* __restrict__ lin,
                                                     int64_t hw, int C, double* __restrict__ part) {
    __shared__ double s_red[WAVES];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nw = C / 2;
    const int64_t n = blockIdx.y;
    double l[MAXW][2];
    load_lin(lin, nw, lane, l);
    double acc = 0.0;
    Pixel<DT> px;
    for (int64_t p = (int64_t)blockIdx.x * WAVES + wave; p < hw; p += (int64_t)gridDim.x * WAVES) {
        const int64_t o = (n * hw + p) * nw;
        px.load(ax + o, ay + o, nw, lane);
#pragma unroll
        for (int i = 0; i < MAXW; ++i)
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                const double d = px.u[i][h] - px.v[i][h];
                acc += l[i][h] * d * d;
            }
    }
    const double s = block_sum(acc, s_red);
    if (threadIdx.x == 0) part[n * gridDim.x + blockIdx.x] = s;
}

// one workgroup per image: the partials in a fixed order
__global__ __launch_bounds__(NT) void tap_reduce_kernel(const double* __restrict__ part, int nblk, int64_t hw, float* __restrict__ terms) {
    __shared__ double s_red[WAVES];
    const int64_t n = blockIdx.x;
    double s = 0.0;
    for (int i = threadIdx.x; i < nblk; i += NT) s += part[n * nblk + i];
    s = block_sum(s, s_red);
    if (threadIdx.x == 0) terms[n] = (float)(s / (double)hw);
}

template <int DT>
__global__ __launch_bounds__(NT) void tap_bwd_kernel(const unsigned* __restrict__ ax, const unsigned* __restrict__ ay, const float* __restrict__ lin,
                                                     const float* __restrict__ upstream, int64_t hw, int C, int relu_mask,
                                                     unsigned* __restrict__ grad) {
    typedef GvfLp<0> G;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nw = C / 2;
    const int64_t n = blockIdx.y;
    double l[MAXW][2];
    load_lin(lin, nw, lane, l);
    const double scale = 2.0 * (double)upstream[n] / (double)hw;
    Pixel<DT> px;
    for (int64_t p = (int64_t)blockIdx.x * WAVES + wave; p < hw; p += (int64_t)gridDim.x * WAVES) {
        const int64_t o = (n * hw + p) * nw;
        px.load(ax + o, ay + o, nw, lane);
        double w[MAXW][2], dot = 0.0;
#pragma unroll
        for (int i = 0; i < MAXW; ++i)
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                w[i][h] = scale * l[i][h] * (px.u[i][h] - px.v[i][h]);
                dot += w[i][h] * px.u[i][h];
            }
        dot = wave_sum(dot);
        const double inv_r = px.rx > 0.0 ? 1.0 / px.rx : 0.0;
#pragma unroll
        for (int i = 0; i < MAXW; ++i) {
            const int wd = lane + GVF_WAVE * i;
            if (wd >= nw) continue;
            float g[2];
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                g[h] = (float)((w[i][h] - px.ax[i][h] * inv_r * dot) / px.dxn);
                if (relu_mask && !(px.ax[i][h] > 0.0)) g[h] = 0.f;
            }
            grad[o + wd] = G::pack(g[0], g[1]);
        }
    }
}

bool dtype_ok(int dt) { return dt == GVF_DT_BF16 || dt == GVF_DT_F16; }
bool chan_ok(int c) { return c == 64 || c == 128 || c == 256 || c == 512; }
bool aligned16(const void* p) { return ((uintptr_t)p & 15u) == 0; }
bool size_ok(int N, int H, int W) { return N > 0 && H > 0 && W > 0 && (int64_t)N * H * W <= ((int64_t)1 << 31); }

unsigned grid_for(int64_t total) {
    const int64_t b = (total + NT - 1) / NT;
    return (unsigned)(b < 65536 ? (b < 1 ? 1 : b) : 65536);
}

int tap_blocks(int64_t hw) {
    const int64_t b = (hw + 4 * WAVES - 1) / (4 * WAVES);
    return (int)(b < TAP_MAX_BLOCKS ? b : TAP_MAX_BLOCKS);
}

}  // namespace

extern "C" int gvf_maxpool2x2_forward(const void* in, void* out, int N, int H, int W, int C, int dtype, void* stream) {
    if (!in || !out || !dtype_ok(dtype) || !size_ok(N, H, W) || H < 2 || W < 2 || C <= 0 || C % 8 || C > 512 || !aligned16(in) || !aligned16(out))
        return GVF_EINVAL;
    const int64_t total = (int64_t)N * (H / 2) * (W / 2) * (C / 8);
    GVF_LP_DISPATCH(dtype, (pool_fwd_kernel<DT><<<grid_for(total), NT, 0, (hipStream_t)stream>>>((const unsigned short*)in, (unsigned short*)out, H, W,
                                                                                                 C, total)));
    GVF_CHECK_LAUNCH();
    return GVF_OK;
}

extern "C" int gvf_maxpool2x2_backward(const void* a, const void* g_pooled, const void* tap_grad, void* z, int N, int H, int W, int C, int dtype,
                                       void* stream) {
    if (!a || !g_pooled || !tap_grad || !z || !dtype_ok(dtype) || !size_ok(N, H, W) || H < 2 || W < 2 || C <= 0 || C % 8 || C > 512 ||
        !aligned16(a) || !aligned16(g_pooled) || !aligned16(tap_grad) || !aligned16(z))
        return GVF_EINVAL;
    const int64_t total = (int64_t)N * H * W * (C / 8);
    GVF_LP_DISPATCH(dtype, (pool_bwd_kernel<DT><<<grid_for(total), NT, 0, (hipStream_t)stream>>>(
                               (const unsigned short*)a, (const unsigned short*)g_pooled, (const unsigned short*)tap_grad, (unsigned short*)z, H,
                               W, C, total)));
    GVF_CHECK_LAUNCH();
    return GVF_OK;
}

extern "C" int gvf_lpips_tap_scratch_bytes(int N, int H, int W, size_t* out) {
    if (!out || !size_ok(N, H, W)) return GVF_EINVAL;
    *out = gvf_align_up((size_t)N * tap_blocks((int64_t)H * W) * sizeof(double), 256);
    return GVF_OK;
}

extern "C" int gvf_lpips_tap_forward(const void* ax, const void* ay, const float* lin, int N, int H, int W, int C, int dtype, float* terms_out,
                                     void* scratch, size_t scratch_bytes, void* stream) {
    if (!ax || !ay || !lin || !terms_out || !scratch || !dtype_ok(dtype) || !chan_ok(C) || !size_ok(N, H, W) || N > 65535 || !aligned16(ax) ||
        !aligned16(ay) || !aligned16(scratch))
        return GVF_EINVAL;
    const int64_t hw = (int64_t)H * W;
    const int nblk = tap_blocks(hw);
    if (scratch_bytes < (size_t)N * nblk * sizeof(double)) return GVF_ENOSPC;
    hipStream_t s = (hipStream_t)stream;
    GVF_LP_DISPATCH(dtype, (tap_fwd_kernel<DT><<<dim3((unsigned)nblk, (unsigned)N), NT, 0, s>>>((const unsigned*)ax, (const unsigned*)ay, lin, hw, C,
                                                                                                 (double*)scratch)));
    GVF_CHECK_LAUNCH();
    tap_reduce_kernel<<<(unsigned)N, NT, 0, s>>>((const double*)scratch, nblk, hw, terms_out);
    GVF_CHECK_LAUNCH();
    return GVF_OK;
}

extern "C" int gvf_lpips_tap_backward(const void* ax, const void* ay, const float* lin, const float* upstream, int N, int H, int W, int C, int dtype,
                                      int flags, void* grad_out, void* stream) {
    if (!ax || !ay || !lin || !upstream || !grad_out || !dtype_ok(dtype) || !chan_ok(C) || !size_ok(N, H, W) || N > 65535 ||
        (flags & ~GVF_TAP_RELU_MASK) || !aligned16(ax) || !aligned16(ay) || !aligned16(grad_out))
        return GVF_EINVAL;
    const int64_t hw = (int64_t)H * W;
    GVF_LP_DISPATCH(dtype, (tap_bwd_kernel<DT><<<dim3((unsigned)tap_blocks(hw), (unsigned)N), NT, 0, (hipStream_t)stream>>>(
                               (const unsigned*)ax, (const unsigned*)ay, lin, upstream, hw, C, flags & GVF_TAP_RELU_MASK, (unsigned*)grad_out)));
    GVF_CHECK_LAUNCH();
    return GVF_OK;
}
