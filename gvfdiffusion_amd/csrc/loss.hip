// loss.hip -- fused L1 + SSIM image loss (forward and gradient), gfx950.  C ABI and formulas: include/gvf_loss.h.
//
// Tiling (both stencil kernels): one 256-thread workgroup per 64 x 16 output tile of one plane.  The tile and its 5-pixel
// halo (74 x 26) are staged in LDS with zero padding outside the image; a horizontal 11-tap pass writes 64 x 26 rows of
// horizontal sums to LDS (one wave per row, conflict-free); the vertical 11-tap pass gives each thread one column and four
// consecutive rows, so 14 LDS rows feed 4 outputs.
//   forward:  5 moments (p, g, pp, gg, pg) -> S, |p - g| -> per-workgroup double partials; with the SSIM gradient requested it
//             also writes the three partial-derivative maps a, b, c (gvf_loss.h).  The no-grad forward writes no per-pixel output.
//   backward: the window over a, b, c (3 channels, same tiling), then grad = c_l1 sign(p - g) + c_ssim (G*a + 2p G*b + g G*c).
//   reduce:   one workgroup sums the partials in a fixed order (deterministic, no atomics).
// Built with -ffp-contract=off (_build.py): fmaf only where written, so that identical inputs give identical numerator and
// denominator terms (S = 1 exactly up to the rounding of the division).
#include "gvf_common.h"
#include "gvf_rowops.h"
#include "../../include/gvf_rast.h"
#include "../../include/gvf_loss.h"

namespace {

constexpr int NT = 256;                 // threads per workgroup
constexpr int TW = 64, TH = 16;         // output tile
constexpr int R = GVF_SSIM_WINDOW / 2;  // 5
constexpr int K = GVF_SSIM_WINDOW;      // 11
constexpr int SW = TW + 2 * R, SH = TH + 2 * R;   // staged region 74 x 26
constexpr int RPT = TH / (NT / TW);     // output rows per thread: 4
constexpr float C1 = 0.01f * 0.01f, C2 = 0.03f * 0.03f;
static_assert(RPT * (NT / TW) == TH, "tile rows");

// utils/loss_util.py:gaussian(11, 1.5): exp in double, rounded to fp32, normalised by their fp32 sum (bit patterns as torch computes them)
__constant__ float c_win[K] = {0x1.0d956cp-10f, 0x1.f1fe02p-8f, 0x1.26eb18p-5f, 0x1.bff0fep-4f, 0x1.b43c3ep-3f, 0x1.106560p-2f,
                               0x1.b43c3ep-3f,  0x1.bff0fep-4f, 0x1.26eb18p-5f, 0x1.f1fe02p-8f, 0x1.0d956cp-10f};
const float h_win[K] = {0x1.0d956cp-10f, 0x1.f1fe02p-8f, 0x1.26eb18p-5f, 0x1.bff0fep-4f, 0x1.b43c3ep-3f, 0x1.106560p-2f,
                        0x1.b43c3ep-3f,  0x1.bff0fep-4f, 0x1.26eb18p-5f, 0x1.f1fe02p-8f, 0x1.0d956cp-10f};

struct Tile {
    int x0, y0;
    int64_t base;   // offset of the plane
};

__device__ __forceinline__ Tile tile_of(int tiles_x, int tiles_y, int H, int W) {
    const int64_t b = blockIdx.x;
    const int tx = (int)(b % tiles_x);
    const int64_t t = b / tiles_x;
    const int ty = (int)(t % tiles_y);
    const int64_t plane = t / tiles_y;
    return {tx * TW, ty * TH, plane * (int64_t)H * W};
}

// stage `NC` planes of the (SH x SW) region around the tile, zero outside the image.  Every load of the thread is issued before
// the first LDS store (registers v), so a workgroup waits for one memory latency rather than one per element it stages.
constexpr int STAGE_IT = (SH * SW + NT - 1) / NT;   // 8
template <int NC>
__device__ __forceinline__ void stage(float (*s)[SH][SW], const float* const* src, const Tile& t, int H, int W) {
    float v[STAGE_IT][NC];
#pragma unroll
    for (int it = 0; it < STAGE_IT; ++it) {
        const int i = threadIdx.x + it * NT;
        const int r = i / SW, c = i - r * SW;
        const int y = t.y0 - R + r, x = t.x0 - R + c;
        const bool in = i < SH * SW && y >= 0 && y < H && x >= 0 && x < W;
        const int64_t o = t.base + (int64_t)y * W + x;
#pragma unroll
        for (int ch = 0; ch < NC; ++ch) v[it][ch] = in ? src[ch][o] : 0.f;
    }
#pragma unroll
    for (int it = 0; it < STAGE_IT; ++it) {
        const int i = threadIdx.x + it * NT;
        if (i < SH * SW) {
            const int r = i / SW, c = i - r * SW;
#pragma unroll
            for (int ch = 0; ch < NC; ++ch) s[ch][r][c] = v[it][ch];
        }
    }
}

// vertical 11-tap pass for one column and RPT rows: acc[j][ch] = sum_k w[k] h[ch][r0 + j + k][c]
template <int NC>
__device__ __forceinline__ void vpass(float (*h)[SH][TW], int r0, int c, float (&acc)[RPT][NC]) {
#pragma unroll
    for (int j = 0; j < RPT; ++j)
#pragma unroll
        for (int ch = 0; ch < NC; ++ch) acc[j][ch] = 0.f;
#pragma unroll
    for (int k = 0; k < K + RPT - 1; ++k) {
        float v[NC];
#pragma unroll
        for (int ch = 0; ch < NC; ++ch) v[ch] = h[ch][r0 + k][c];
#pragma unroll
        for (int j = 0; j < RPT; ++j) {
            const int tap = k - j;
            if (tap >= 0 && tap < K) {
#pragma unroll
                for (int ch = 0; ch < NC; ++ch) acc[j][ch] = fmaf(c_win[tap], v[ch], acc[j][ch]);
            }
        }
    }
}

template <bool GRAD>
__global__ __launch_bounds__(NT) void image_loss_fwd_kernel(const float* __restrict__ pred, const float* __restrict__ gt, int H, int W,
                                                            int tiles_x, int tiles_y, int64_t n, double* __restrict__ part,
                                                            float* __restrict__ maps) {
    __shared__ float s_in[2][SH][SW];       // p, g               15.2 KiB
    __shared__ float s_h[5][SH][TW];        // horizontal sums    32.5 KiB
    __shared__ double s_red[2][NT / GVF_WAVE];
    const Tile t = tile_of(tiles_x, tiles_y, H, W);
    const float* src[2] = {pred, gt};
    stage<2>(s_in, src, t, H, W);
    __syncthreads();
    for (int i = threadIdx.x; i < SH * TW; i += NT) {
        const int r = i / TW, c = i - r * TW;
        float a1 = 0.f, a2 = 0.f, a11 = 0.f, a22 = 0.f, a12 = 0.f;
#pragma unroll
        for (int k = 0; k < K; ++k) {
            const float pv = s_in[0][r][c + k], gv = s_in[1][r][c + k];
            const float wp = c_win[k] * pv, wg = c_win[k] * gv;
            a1 += wp;
            a2 += wg;
            a11 = fmaf(wp, pv, a11);
            a22 = fmaf(wg, gv, a22);
            a12 = fmaf(wp, gv, a12);
        }
        s_h[0][r][c] = a1; s_h[1][r][c] = a2; s_h[2][r][c] = a11; s_h[3][r][c] = a22; s_h[4][r][c] = a12;
    }
    __syncthreads();
    const int c = threadIdx.x % TW, r0 = (threadIdx.x / TW) * RPT;
    float m[RPT][5];
    vpass<5>(s_h, r0, c, m);
    const int x = t.x0 + c;
    float ssum = 0.f, lsum = 0.f;
#pragma unroll
    for (int j = 0; j < RPT; ++j) {
        const int y = t.y0 + r0 + j;
        if (x >= W || y >= H) continue;
        const float mu1 = m[j][0], mu2 = m[j][1];
        const float mu1mu2 = mu1 * mu2, mu1sq = mu1 * mu1, mu2sq = mu2 * mu2;
        const float s1 = m[j][2] - mu1sq, s2 = m[j][3] - mu2sq, s12 = m[j][4] - mu1mu2;
        const float A1 = 2.f * mu1mu2 + C1, A2 = 2.f * s12 + C2;
        const float B1 = mu1sq + mu2sq + C1, B2 = s1 + s2 + C2;
        const float D = B1 * B2;
        const float S = (A1 * A2) / D;
        ssum += S;
        lsum += fabsf(s_in[0][r0 + j + R][c + R] - s_in[1][r0 + j + R][c + R]);
        if (GRAD) {
            const float dmu1 = (2.f * mu2 * A2) / D - (2.f * mu1 * S) / B1;   // dS/dmu1 at fixed s1, s12
            const float ds1 = -S / B2;                                        // dS/ds1
            const float ds12 = (2.f * A1) / D;                                // dS/ds12
            const float da = dmu1 - 2.f * mu1 * ds1 - mu2 * ds12;             // total derivative in G*p
            const int64_t o = t.base + (int64_t)y * W + x;
            maps[o] = da;
            maps[n + o] = ds1;
            maps[2 * n + o] = ds12;
        }
    }
    const double bs = gvf_block_sum_waves<NT>((double)ssum, s_red[0]);
    const double bl = gvf_block_sum_waves<NT>((double)lsum, s_red[1]);
    if (threadIdx.x == 0) {
        part[2 * (int64_t)blockIdx.x] = bs;
        part[2 * (int64_t)blockIdx.x + 1] = bl;
    }
}

// one workgroup: fixed-order sum of the per-workgroup partials -> terms[3] = loss, mean L1, mean SSIM
__global__ __launch_bounds__(NT) void image_loss_reduce_kernel(const double* __restrict__ part, int64_t nblk, int64_t n, float w_l1,
                                                               float w_ssim, float* __restrict__ terms) {
    __shared__ double s_red[2][NT / GVF_WAVE];
    double s = 0.0, l = 0.0;
    for (int64_t i = threadIdx.x; i < nblk; i += NT) {
        s += part[2 * i];
        l += part[2 * i + 1];
    }
    s = gvf_block_sum_waves<NT>(s, s_red[0]);
    l = gvf_block_sum_waves<NT>(l, s_red[1]);
    if (threadIdx.x == 0) {
        const double ms = s / (double)n, ml = l / (double)n;
        terms[0] = (float)((double)w_l1 * ml + (double)w_ssim * (1.0 - ms));
        terms[1] = (float)ml;
        terms[2] = (float)ms;
    }
}

struct Coef {
    float l1, ss;
};

// c_l1 = (t0 w_l1 + t1) / n, c_ss = (t2 - t0 w_ssim) / n; the division as torch's mean backward does it (times the fp32 1/n)
__device__ __forceinline__ Coef coef_of(const float* __restrict__ gterms, float w_l1, float w_ssim, int64_t n) {
    const float inv_n = 1.f / (float)n;
    const float t0 = gterms[0], t1 = gterms[1], t2 = gterms[2];
    return {(t0 * w_l1 + t1) * inv_n, (t2 - t0 * w_ssim) * inv_n};
}

__device__ __forceinline__ float sgn(float d) { return d > 0.f ? 1.f : (d < 0.f ? -1.f : 0.f); }

__global__ __launch_bounds__(NT) void image_loss_bwd_kernel(const float* __restrict__ pred, const float* __restrict__ gt, int H, int W,
                                                            int tiles_x, int tiles_y, int64_t n, const float* __restrict__ maps,
                                                            const float* __restrict__ gterms, float w_l1, float w_ssim,
                                                            float* __restrict__ grad) {
    __shared__ float s_in[3][SH][SW];       // a, b, c            22.8 KiB
    __shared__ float s_h[3][SH][TW];        // horizontal sums    19.5 KiB
    const Tile t = tile_of(tiles_x, tiles_y, H, W);
    const float* src[3] = {maps, maps + n, maps + 2 * n};
    stage<3>(s_in, src, t, H, W);
    __syncthreads();
    for (int i = threadIdx.x; i < SH * TW; i += NT) {
        const int r = i / TW, c = i - r * TW;
        float h0 = 0.f, h1 = 0.f, h2 = 0.f;
#pragma unroll
        for (int k = 0; k < K; ++k) {
            h0 = fmaf(c_win[k], s_in[0][r][c + k], h0);
            h1 = fmaf(c_win[k], s_in[1][r][c + k], h1);
            h2 = fmaf(c_win[k], s_in[2][r][c + k], h2);
        }
        s_h[0][r][c] = h0; s_h[1][r][c] = h1; s_h[2][r][c] = h2;
    }
    __syncthreads();
    const int c = threadIdx.x % TW, r0 = (threadIdx.x / TW) * RPT;
    float m[RPT][3];
    vpass<3>(s_h, r0, c, m);
    const Coef k = coef_of(gterms, w_l1, w_ssim, n);
    const int x = t.x0 + c;
#pragma unroll
    for (int j = 0; j < RPT; ++j) {
        const int y = t.y0 + r0 + j;
        if (x >= W || y >= H) continue;
        const int64_t o = t.base + (int64_t)y * W + x;
        const float pv = pred[o], gv = gt[o];
        const float ds = m[j][0] + (2.f * pv) * m[j][1] + gv * m[j][2];
        grad[o] = k.l1 * sgn(pv - gv) + k.ss * ds;
    }
}

// L1 part only (no SSIM maps): element-wise
__global__ __launch_bounds__(NT) void image_loss_bwd_l1_kernel(const float* __restrict__ pred, const float* __restrict__ gt, int64_t n,
                                                               const float* __restrict__ gterms, float w_l1, float w_ssim,
                                                               float* __restrict__ grad) {
    const Coef k = coef_of(gterms, w_l1, w_ssim, n);
    for (int64_t i = (int64_t)blockIdx.x * NT + threadIdx.x; i < n; i += (int64_t)gridDim.x * NT) grad[i] = k.l1 * sgn(pred[i] - gt[i]);
}

struct Geom {
    int64_t n, nblk;
    int tiles_x, tiles_y;
    size_t part_bytes, map_off, bytes;
};

bool geom_of(int64_t planes, int H, int W, int flags, Geom& g) {
    if (planes <= 0 || H <= 0 || W <= 0 || (flags & ~GVF_IMAGE_LOSS_SSIM_GRAD)) return false;
    const int64_t hw = (int64_t)H * W;
    if (planes > ((int64_t)1 << 60) / 12 / hw) return false;        // 3 maps of n fp32 must fit
    g.n = planes * hw;
    g.tiles_x = (W + TW - 1) / TW;
    g.tiles_y = (H + TH - 1) / TH;
    const int64_t tiles = (int64_t)g.tiles_x * g.tiles_y;
    if (planes > (int64_t)0x7fffffff / tiles) return false;          // 1-D grid
    g.nblk = planes * tiles;
    g.part_bytes = gvf_align_up((size_t)g.nblk * 2 * sizeof(double), 256);
    g.map_off = g.part_bytes;
    g.bytes = g.part_bytes + ((flags & GVF_IMAGE_LOSS_SSIM_GRAD) ? (size_t)g.n * 3 * sizeof(float) : 0);
    return true;
}

}  // namespace

extern "C" int gvf_ssim_window(float* taps) {
    if (!taps) return GVF_EINVAL;
    for (int k = 0; k < K; ++k) taps[k] = h_win[k];
    return GVF_OK;
}

extern "C" int gvf_image_loss_scratch_bytes(int64_t planes, int H, int W, int flags, size_t* out) {
    Geom g;
    if (!out || !geom_of(planes, H, W, flags, g)) return GVF_EINVAL;
    *out = g.bytes;
    return GVF_OK;
}

extern "C" int gvf_image_loss_forward(const float* pred, const float* gt, int64_t planes, int H, int W, float w_l1, float w_ssim,
                                      float* terms_out, void* scratch, size_t scratch_bytes, int flags, void* stream) {
    Geom g;
    if (!pred || !gt || !terms_out || !scratch || !geom_of(planes, H, W, flags, g)) return GVF_EINVAL;
    if (scratch_bytes < g.bytes) return GVF_ENOSPC;
    hipStream_t s = (hipStream_t)stream;
    double* part = (double*)scratch;
    if (flags & GVF_IMAGE_LOSS_SSIM_GRAD)
        image_loss_fwd_kernel<true><<<dim3((unsigned)g.nblk), NT, 0, s>>>(pred, gt, H, W, g.tiles_x, g.tiles_y, g.n, part,
                                                                          (float*)((char*)scratch + g.map_off));
    else
        image_loss_fwd_kernel<false><<<dim3((unsigned)g.nblk), NT, 0, s>>>(pred, gt, H, W, g.tiles_x, g.tiles_y, g.n, part, nullptr);
    GVF_CHECK_LAUNCH();
    image_loss_reduce_kernel<<<1, NT, 0, s>>>(part, g.nblk, g.n, w_l1, w_ssim, terms_out);
    GVF_CHECK_LAUNCH();
    return GVF_OK;
}

extern "C" int gvf_image_loss_backward(const float* pred, const float* gt, int64_t planes, int H, int W, float w_l1, float w_ssim,
                                       const float* grad_terms, float* grad_pred, const void* scratch, size_t scratch_bytes, int flags,
                                       void* stream) {
    Geom g;
    if (!pred || !gt || !grad_terms || !grad_pred || !geom_of(planes, H, W, flags, g)) return GVF_EINVAL;
    hipStream_t s = (hipStream_t)stream;
    if (flags & GVF_IMAGE_LOSS_SSIM_GRAD) {
        if (!scratch) return GVF_EINVAL;
        if (scratch_bytes < g.bytes) return GVF_ENOSPC;
        image_loss_bwd_kernel<<<dim3((unsigned)g.nblk), NT, 0, s>>>(pred, gt, H, W, g.tiles_x, g.tiles_y, g.n,
                                                                    (const float*)((const char*)scratch + g.map_off), grad_terms, w_l1,
                                                                    w_ssim, grad_pred);
    } else {
        const int64_t blocks = (g.n + NT - 1) / NT;
        image_loss_bwd_l1_kernel<<<dim3((unsigned)(blocks < 8192 ? blocks : 8192)), NT, 0, s>>>(pred, gt, g.n, grad_terms, w_l1, w_ssim,
                                                                                               grad_pred);
    }
    GVF_CHECK_LAUNCH();
    return GVF_OK;
}
