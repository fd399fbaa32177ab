// rgba.hip -- RGBA condition preprocessing: alpha bounding box, and Pillow's crop + premultiplied-alpha resize + composite, gfx950.
//
// Replaces the per-frame host loops over Pillow and numpy in front of the image encoder (see include/gvf_image.h).  Byte
// streaming work: per image 4 B read per source pixel of the crop window, 4 B written and ~ksize cached re-reads per
// intermediate pixel, 3 to 12 B written per canvas pixel.
//   bbox:       one workgroup per 4 image rows, one 32-bit load per pixel (lanes read neighbouring pixels), integer min / max
//               folded through LDS atomics, five global atomics per workgroup.
//   horizontal: one workgroup per (up to) 4 rows of the crop window; the rows are read through the window (zero outside the
//               image), premultiplied and staged in LDS as one 32-bit word per pixel; thread x produces output column x of all
//               staged rows, so a coefficient is fetched once per 4 rows and the tap-major table makes those fetches coalesced.
//   vertical:   one thread per canvas pixel; a tap is one 32-bit load of the RGBa intermediate (lanes read neighbouring
//               pixels), four int32 accumulators; the epilogue un-premultiplies with exact integer division and writes the
//               requested composite.
// Compiled with -ffp-contract=off: the composites are fp32 / fp64 sequences rounded operation by operation.
#include "gvf_common.h"
#include "../../include/gvf_rast.h"
#include "../../include/gvf_image.h"

namespace {

constexpr int RB = 256;
constexpr int PREC = GVF_RESAMPLE_PRECISION_BITS;
constexpr int HR = 4;                  // crop-window rows per workgroup of the horizontal pass (fewer when a row is wide)
constexpr int LDS_PIXELS = 16384;      // 64 KiB of staged 32-bit pixels
constexpr int BR = 4;                  // image rows per workgroup of the bounding-box pass

__device__ __forceinline__ uint32_t clip8(int32_t acc) {
    const int32_t v = acc >> PREC;
    return (uint32_t)(v < 0 ? 0 : (v > 255 ? 255 : v));
}

// RGBA -> RGBa of one little-endian pixel word (R in the low byte, A in the high one)
__device__ __forceinline__ uint32_t premultiply(uint32_t w) {
    const uint32_t a = w >> 24;
    uint32_t o = w & 0xff000000u;
#pragma unroll
    for (int s = 0; s < 24; s += 8) {
        const uint32_t t = ((w >> s) & 255u) * a + 128u;
        o |= (((t >> 8) + t) >> 8) << s;
    }
    return o;
}

// RGBa -> RGBA of one colour value: truncating division, clamped (filter overshoot leaves p > a)
__device__ __forceinline__ uint32_t unpremultiply(uint32_t p, uint32_t a) {
    if (a == 0u || a == 255u) return p;
    const uint32_t q = (255u * p) / a;
    return q > 255u ? 255u : q;
}

// the source pixel behind crop-window position (x, y): zero outside the image
__device__ __forceinline__ uint32_t window_pixel(const uint32_t* __restrict__ img, int in_h, int in_w, int sx, int sy) {
    return (sx >= 0 && sx < in_w && sy >= 0 && sy < in_h) ? img[(int64_t)sy * in_w + sx] : 0u;
}

__global__ __launch_bounds__(RB) void bbox_init_kernel(int32_t* __restrict__ out, int64_t n, int h, int w) {
    const int64_t i = (int64_t)blockIdx.x * RB + threadIdx.x;
    if (i >= n) return;
    out[i * 5 + 0] = w; out[i * 5 + 1] = h; out[i * 5 + 2] = -1; out[i * 5 + 3] = -1; out[i * 5 + 4] = 255;
}

__global__ __launch_bounds__(RB) void bbox_kernel(const uint32_t* __restrict__ src, int h, int w, int threshold, int32_t* __restrict__ out) {
    __shared__ int32_t red[5];
    const uint32_t* img = src + (int64_t)blockIdx.y * h * w;
    const int y0 = blockIdx.x * BR, y1 = min(h, y0 + BR);
    if (threadIdx.x == 0) { red[0] = w; red[1] = h; red[2] = -1; red[3] = -1; red[4] = 255; }
    __syncthreads();
    int32_t xmin = w, ymin = h, xmax = -1, ymax = -1, amin = 255;
    for (int y = y0; y < y1; ++y)
        for (int x = threadIdx.x; x < w; x += RB) {
            const int32_t a = (int32_t)(img[(int64_t)y * w + x] >> 24);
            amin = min(amin, a);
            if (a > threshold) { xmin = min(xmin, x); xmax = max(xmax, x); ymin = min(ymin, y); ymax = max(ymax, y); }
        }
    if (amin < 255) atomicMin(&red[4], amin);
    if (xmax >= 0) { atomicMin(&red[0], xmin); atomicMin(&red[1], ymin); atomicMax(&red[2], xmax); atomicMax(&red[3], ymax); }
    __syncthreads();
    if (threadIdx.x == 0) {
        int32_t* o = out + (int64_t)blockIdx.y * 5;
        if (red[4] < 255) atomicMin(o + 4, red[4]);
        if (red[2] >= 0) { atomicMin(o + 0, red[0]); atomicMin(o + 1, red[1]); atomicMax(o + 2, red[2]); atomicMax(o + 3, red[3]); }
    }
}

// No horizontal resampling but a vertical one: the window's pixels, premultiplied, are the intermediate image.
__global__ __launch_bounds__(RB) void premultiply_window_kernel(const uint32_t* __restrict__ src, uint32_t* __restrict__ dst, int in_h, int in_w,
                                                                int cx0, int cy0, int cw, int ch) {
    const int x = blockIdx.x * RB + threadIdx.x, y = blockIdx.y;
    if (x >= cw) return;
    const int64_t n = blockIdx.z;
    dst[(n * ch + y) * cw + x] = premultiply(window_pixel(src + n * in_h * in_w, in_h, in_w, cx0 + x, cy0 + y));
}

// One workgroup = `hr` (<= HR) consecutive rows of one image's crop window, premultiplied into LDS; thread x owns output column x.
__global__ __launch_bounds__(RB) void resample_h_rgba_kernel(const uint32_t* __restrict__ src, uint32_t* __restrict__ dst, int in_h, int in_w,
                                                             int cx0, int cy0, int cw, int ch, int out_w, int hr,
                                                             const int32_t* __restrict__ first, const int32_t* __restrict__ count,
                                                             const int32_t* __restrict__ coef) {
    extern __shared__ uint32_t px[];                      // hr x cw
    const int64_t n = blockIdx.y;
    const uint32_t* img = src + n * in_h * in_w;
    const int r0 = blockIdx.x * hr;
    const int nr = min(hr, ch - r0);
    for (int r = 0; r < nr; ++r)
        for (int x = threadIdx.x; x < cw; x += RB) px[r * cw + x] = premultiply(window_pixel(img, in_h, in_w, cx0 + x, cy0 + r0 + r));
    __syncthreads();
    int row[HR];
#pragma unroll
    for (int r = 0; r < HR; ++r) row[r] = min(r, nr - 1) * cw;       // rows past the last one repeat it; their results are not stored
    for (int x = threadIdx.x; x < out_w; x += RB) {
        const int f = first[x], cnt = count[x];
        int32_t acc[HR][4];
#pragma unroll
        for (int r = 0; r < HR; ++r)
#pragma unroll
            for (int c = 0; c < 4; ++c) acc[r][c] = 1 << (PREC - 1);
        for (int k = 0; k < cnt; ++k) {
            const int32_t c = coef[(int64_t)k * out_w + x];
#pragma unroll
            for (int r = 0; r < HR; ++r) {
                const uint32_t w = px[row[r] + f + k];
                acc[r][0] += (int32_t)(w & 255u) * c;
                acc[r][1] += (int32_t)((w >> 8) & 255u) * c;
                acc[r][2] += (int32_t)((w >> 16) & 255u) * c;
                acc[r][3] += (int32_t)(w >> 24) * c;
            }
        }
#pragma unroll
        for (int r = 0; r < HR; ++r)
            if (r < nr)
                dst[(n * ch + r0 + r) * out_w + x] = clip8(acc[r][0]) | (clip8(acc[r][1]) << 8) | (clip8(acc[r][2]) << 16) | (clip8(acc[r][3]) << 24);
    }
}

enum { SRC_TAPS = 0, SRC_MID = 1, SRC_WINDOW = 2 };     // vertical taps over the intermediate / the intermediate as it is / the source (copy)

// One thread = one canvas pixel.  SRC_TAPS, SRC_MID: `mid` holds RGBa rows of `mid_w` pixels; SRC_WINDOW: `mid` is the RGBA source, read
// through the crop window without any conversion (Pillow returns a copy when the size does not change).
template <int SRC, int MODE>
__global__ __launch_bounds__(RB) void resample_v_rgba_kernel(const uint32_t* __restrict__ mid, int mid_rows, int mid_w, int in_h, int in_w, int cx0,
                                                             int cy0, int out_h, void* __restrict__ dst, uint8_t* __restrict__ mask, int dst_h,
                                                             int dst_w, int off_y, int off_x, int pad, const int32_t* __restrict__ first,
                                                             const int32_t* __restrict__ count, const int32_t* __restrict__ coef) {
    const int x = blockIdx.x * RB + threadIdx.x, y = blockIdx.y;
    if (x >= dst_w) return;
    const int64_t n = blockIdx.z;
    const int sy = y - off_y, sx = x - off_x;
    const bool covered = sy >= 0 && sy < out_h && sx >= 0 && sx < mid_w;
    uint32_t r = 0, g = 0, b = 0, a = 0;
    if (covered) {
        uint32_t w;
        if (SRC == SRC_WINDOW) {
            w = window_pixel(mid + n * in_h * in_w, in_h, in_w, cx0 + sx, cy0 + sy);
        } else if (SRC == SRC_MID) {
            w = mid[(n * mid_rows + sy) * mid_w + sx];
        } else {
            const uint32_t* col = mid + n * mid_rows * mid_w + sx;
            const int f = first[sy], cnt = count[sy];
            int32_t a0 = 1 << (PREC - 1), a1 = a0, a2 = a0, a3 = a0;
            for (int k = 0; k < cnt; ++k) {
                const uint32_t t = col[(int64_t)(f + k) * mid_w];
                const int32_t c = coef[(int64_t)k * out_h + sy];
                a0 += (int32_t)(t & 255u) * c;
                a1 += (int32_t)((t >> 8) & 255u) * c;
                a2 += (int32_t)((t >> 16) & 255u) * c;
                a3 += (int32_t)(t >> 24) * c;
            }
            w = clip8(a0) | (clip8(a1) << 8) | (clip8(a2) << 16) | (clip8(a3) << 24);
        }
        r = w & 255u; g = (w >> 8) & 255u; b = (w >> 16) & 255u; a = w >> 24;
        if (SRC != SRC_WINDOW) { r = unpremultiply(r, a); g = unpremultiply(g, a); b = unpremultiply(b, a); }
    }
    const int64_t pix = (n * dst_h + y) * dst_w + x;
    if (MODE == GVF_RGBA_OUT_RGBA) {
        const uint32_t p = (uint32_t)pad;
        ((uint32_t*)dst)[pix] = covered ? (r | (g << 8) | (b << 16) | (a << 24)) : (p | (p << 8) | (p << 16) | (p << 24));
    } else if (MODE == GVF_RGBA_OUT_F32) {
        // (c / 255f) * (a / 255f), kept in fp32, planar
        float* o = (float*)dst + (n * 3 * dst_h + y) * dst_w + x;
        const int64_t plane = (int64_t)dst_h * dst_w;
        const float fa = (float)a / 255.0f, fp = (float)pad / 255.0f;
        o[0] = covered ? ((float)r / 255.0f) * fa : fp;
        o[plane] = covered ? ((float)g / 255.0f) * fa : fp;
        o[2 * plane] = covered ? ((float)b / 255.0f) * fa : fp;
    } else {
        uint8_t* o = (uint8_t*)dst + pix * 3;
        uint32_t v[3] = {r, g, b};
        const float fa = (float)a / 255.0f;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const float prod = ((float)v[c] / 255.0f) * fa;
            if (MODE == GVF_RGBA_OUT_BLACK) {
                v[c] = (uint32_t)(prod * 255.0f);                            // (rgb * alpha * 255).astype(uint8), all in fp32
            } else {
                const float wv = prod + (1.0f - fa) * 1.0f;                  // fp32, the product rounded before the add
                v[c] = (uint32_t)((double)wv * 255.0);                       // assigned into a float64 canvas, then * 255 -> uint8
            }
            o[c] = covered ? (uint8_t)v[c] : (uint8_t)pad;
        }
        if (MODE == GVF_RGBA_OUT_WHITE && mask) mask[pix] = covered ? (uint8_t)((double)fa * 255.0) : (uint8_t)0;
    }
}

bool table_ok(const GvfResampleTable* t) {
    return t->first && t->count && t->coef && t->ksize >= 1 && t->ksize <= GVF_RESAMPLE_MAX_TAPS && t->n_out >= 1 &&
           t->n_out <= GVF_RESAMPLE_MAX_WIDTH;
}

template <int SRC>
void launch_v(int mode, dim3 grid, hipStream_t s, const uint32_t* mid, int mid_rows, int mid_w, int in_h, int in_w, int cx0, int cy0, int out_h,
              void* dst, uint8_t* mask, int dst_h, int dst_w, int off_y, int off_x, int pad, const GvfResampleTable* tv) {
    const int32_t* f = tv ? tv->first : nullptr;
    const int32_t* c = tv ? tv->count : nullptr;
    const int32_t* k = tv ? tv->coef : nullptr;
#define GVF_V(M) resample_v_rgba_kernel<SRC, M><<<grid, RB, 0, s>>>(mid, mid_rows, mid_w, in_h, in_w, cx0, cy0, out_h, dst, mask, dst_h, dst_w, \
                                                                    off_y, off_x, pad, f, c, k)
    switch (mode) {
        case GVF_RGBA_OUT_RGBA: GVF_V(GVF_RGBA_OUT_RGBA); break;
        case GVF_RGBA_OUT_BLACK: GVF_V(GVF_RGBA_OUT_BLACK); break;
        case GVF_RGBA_OUT_WHITE: GVF_V(GVF_RGBA_OUT_WHITE); break;
        default: GVF_V(GVF_RGBA_OUT_F32); break;
    }
#undef GVF_V
}

}  // namespace

extern "C" int gvf_alpha_bbox_u8(const uint8_t* rgba, int64_t n, int h, int w, int threshold, int32_t* out, void* stream) {
    if (!rgba || !out || n < 0 || n > 65535 || h < 1 || w < 1 || h > GVF_RESAMPLE_MAX_WIDTH || w > GVF_RESAMPLE_MAX_WIDTH || threshold < 0 ||
        threshold > 255 || (((uintptr_t)rgba) & 3))
        return GVF_EINVAL;
    if (n == 0) return GVF_OK;
    hipStream_t s = (hipStream_t)stream;
    bbox_init_kernel<<<dim3((unsigned)((n + RB - 1) / RB)), RB, 0, s>>>(out, n, h, w);
    GVF_CHECK_LAUNCH();
    bbox_kernel<<<dim3((unsigned)((h + BR - 1) / BR), (unsigned)n), RB, 0, s>>>((const uint32_t*)rgba, h, w, threshold, out);
    GVF_CHECK_LAUNCH();
    return GVF_OK;
}

extern "C" int gvf_rgba_resample_u8(const uint8_t* src, int64_t n, int in_h, int in_w, int crop_x, int crop_y, int crop_w, int crop_h,
                                    const GvfResampleTable* tab_h, const GvfResampleTable* tab_v, uint8_t* tmp, int mode, void* dst, uint8_t* mask,
                                    int dst_h, int dst_w, int off_y, int off_x, int pad_value, void* stream) {
    const int lim = GVF_RESAMPLE_MAX_WIDTH;
    if (!src || !dst || n < 0 || n > 65535 || in_h < 1 || in_w < 1 || in_h > lim || in_w > lim || crop_w < 1 || crop_h < 1 || crop_w > lim ||
        crop_h > lim || crop_x < -lim || crop_x > lim || crop_y < -lim || crop_y > lim || dst_h < 1 || dst_w < 1 || dst_h > lim || dst_w > lim ||
        off_x < -lim || off_x > lim || off_y < -lim || off_y > lim || pad_value < 0 || pad_value > 255 || mode < GVF_RGBA_OUT_RGBA ||
        mode > GVF_RGBA_OUT_F32 || (((uintptr_t)src) & 3) || (((uintptr_t)dst) & 3 && mode != GVF_RGBA_OUT_BLACK && mode != GVF_RGBA_OUT_WHITE))
        return GVF_EINVAL;
    if (tab_h && !table_ok(tab_h)) return GVF_EINVAL;
    if (tab_v && !table_ok(tab_v)) return GVF_EINVAL;
    if ((tab_h || tab_v) && (!tmp || (((uintptr_t)tmp) & 3))) return GVF_EINVAL;
    if (n == 0) return GVF_OK;
    hipStream_t s = (hipStream_t)stream;
    const int mid_w = tab_h ? tab_h->n_out : crop_w;
    const int out_h = tab_v ? tab_v->n_out : crop_h;
    uint32_t* mid = (uint32_t*)tmp;                       // n x crop_h x mid_w RGBa pixels
    if (tab_h) {
        const int hr = crop_w * HR <= LDS_PIXELS ? HR : (LDS_PIXELS / crop_w > 0 ? LDS_PIXELS / crop_w : 1);
        resample_h_rgba_kernel<<<dim3((unsigned)((crop_h + hr - 1) / hr), (unsigned)n), RB, (size_t)hr * crop_w * 4, s>>>(
            (const uint32_t*)src, mid, in_h, in_w, crop_x, crop_y, crop_w, crop_h, mid_w, hr, tab_h->first, tab_h->count, tab_h->coef);
        GVF_CHECK_LAUNCH();
    } else if (tab_v) {
        premultiply_window_kernel<<<dim3((unsigned)((crop_w + RB - 1) / RB), (unsigned)crop_h, (unsigned)n), RB, 0, s>>>(
            (const uint32_t*)src, mid, in_h, in_w, crop_x, crop_y, crop_w, crop_h);
        GVF_CHECK_LAUNCH();
    }
    dim3 grid((unsigned)((dst_w + RB - 1) / RB), (unsigned)dst_h, (unsigned)n);
    if (tab_v)
        launch_v<SRC_TAPS>(mode, grid, s, mid, crop_h, mid_w, in_h, in_w, crop_x, crop_y, out_h, dst, mask, dst_h, dst_w, off_y, off_x, pad_value, tab_v);
    else if (tab_h)
        launch_v<SRC_MID>(mode, grid, s, mid, crop_h, mid_w, in_h, in_w, crop_x, crop_y, out_h, dst, mask, dst_h, dst_w, off_y, off_x, pad_value, nullptr);
    else
        launch_v<SRC_WINDOW>(mode, grid, s, (const uint32_t*)src, crop_h, mid_w, in_h, in_w, crop_x, crop_y, out_h, dst, mask, dst_h, dst_w, off_y,
                             off_x, pad_value, nullptr);
    GVF_CHECK_LAUNCH();
    return GVF_OK;
}
