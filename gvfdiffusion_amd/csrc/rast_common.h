// rast_common.h -- internal to the rasteriser's translation units (rast.hip = host pipeline + entry points, rast_front.hip = front end,
// rast_sort.hip = per-tile sort, rast_blend.hip = blend, rast_bwd.hip = backward): the constants and device helpers more than one stage uses,
// and the host functions through which the stages meet (the call plan they take: rast_plan.h).  Every kernel is defined and launched in ONE
// of those files; nothing here holds process state.
#pragma once
#include "gvf_common.h"
#include "../../include/gvf_rast.h"
#include "rast_plan.h"
using namespace gvf_rast;
static_assert(WAVE == GVF_WAVE, "rast_plan.h sizes its grids for this wave width");

namespace {

constexpr int BLEND_THREADS = TILE * TILE;
constexpr int MAX_SH_COEFFS = 16;
// The splat record holds the conic PRE-SCALED for the blend: (a, b, c) -> (CONIC_K1 a, CONIC_K2 b, CONIC_K1 c), so that
//   log2(e) * power = log2(e) * (-0.5 (a dx^2 + c dy^2) - b dx dy) = a' dx^2 + c' dy^2 + b' dx dy
// needs no scaling on its way into v_exp_f32 (upstream's form costs nine VALU instructions plus the exp's own log2(e) multiply; the
// compositing loop is VALU-bound).  Readers that need the conic itself un-scale it; the compositing kernels factor it (splat_cholesky below).
constexpr float CONIC_K1 = -0.7213475204444817f;   // -0.5 log2(e)
constexpr float CONIC_K2 = -1.4426950408889634f;   // -log2(e)
constexpr float CONIC_IK1 = -1.3862943611198906f;  // 1 / CONIC_K1 = -2 ln 2
constexpr float CONIC_IK2 = -0.6931471805599453f;  // 1 / CONIC_K2 = -ln 2
// The compositing kernels evaluate the exponent from the CHOLESKY factor of the (scaled, negated) conic in tile-relative coordinates:
//   -power_oct = m11 dx^2 + 2 m12 dx dy + m22 dy^2 = s1^2 + s2^2,   s1 = l11 dx + l12 dy,  s2 = l22 dy,   M = [[-a', -b'/2], [-b'/2, -c']]
// with dx = xr - px, dy = yr - py (splat centre and pixel relative to the tile origin):  s1 = c1 - l11 px - l12 py,  s2 = c2 - l22 py.
// Per (pixel, splat) that is 3 fma + 1 mul + 1 fma and the negation rides on v_exp_f32's source modifier -- against 2 subtractions + 5 for the
// conic form -- and the exponent cannot come out positive, so upstream's `power > 0` test (which only ever fires on rounding noise at the
// centre of a valid splat) has nothing to do: 3 of the ~21 vector instructions of a compositing step.  |c1|, |c2| stay small because a splat
// reaches a tile only within ~3 sigma (|c| <~ 3 + 16 / sigma), so the cancellation in s1 costs ~1e-5 of the exponent.  A conic that is not
// positive definite (NaN / overflowed covariances: upstream composites an indefinite form there) is dropped: its opacity is staged as 0.
struct SplatChol { float l11, l12, l22, c1, c2; bool ok; };
__device__ __forceinline__ SplatChol splat_cholesky(float x, float y, float ap, float bp, float cp, float tile_x0, float tile_y0) {
    SplatChol r;
    const float m11 = -ap, m12 = -0.5f * bp, m22 = -cp;
    const float il = __builtin_amdgcn_rsqf(m11);
    r.l11 = m11 * il;                                   // sqrt(m11)
    r.l12 = m12 * il;
    const float d = m22 - r.l12 * r.l12;
    r.l22 = __builtin_amdgcn_sqrtf(d);
    r.ok = m11 > 0.0f && d > 0.0f && m11 < __builtin_inff() && d < __builtin_inff();
    if (!r.ok) { r.l11 = 0.f; r.l12 = 0.f; r.l22 = 0.f; }
    const float xr = x - tile_x0, yr = y - tile_y0;
    r.c1 = r.ok ? __builtin_fmaf(r.l11, xr, r.l12 * yr) : 0.f;
    r.c2 = r.ok ? r.l22 * yr : 0.f;
    return r;
}
// s1^2 + s2^2 - lo = -(exponent + lo) (octaves) at tile-relative pixel (px, py).  lo = 0: minus the exponent itself; lo = log2(opacity): the
// compositing kernels' form -- alpha = exp2(log2(opacity) + exponent) costs no multiply by the opacity (the constant rides in the first square's
// fma), and an opacity of 0 (or a dropped splat) is lo = -inf -> alpha = 0.
__device__ __forceinline__ float splat_neg_exponent(float l11, float l12, float l22, float c1, float c2, float px, float py, float lo = 0.0f) {
    const float s1 = __builtin_fmaf(-l11, px, __builtin_fmaf(-l12, py, c1));
    const float s2 = __builtin_fmaf(-l22, py, c2);
    return __builtin_fmaf(s2, s2, __builtin_fmaf(s1, s1, -lo));
}

__constant__ float SH_C0 = 0.28209479177387814f;
__constant__ float SH_C1 = 0.4886025119029199f;
__constant__ float SH_C2[5] = {1.0925484305920792f, -1.0925484305920792f, 0.31539156525252005f,
                               -1.0925484305920792f, 0.5462742152960396f};
__constant__ float SH_C3[7] = {-0.5900435899266435f, 2.890611442640554f, -0.4570457994644658f,
                               0.3731763325901154f, -0.4570457994644658f, 1.445305721320277f,
                               -0.5900435899266435f};

// ---------------------------------------------------------------------------------------------
// G1: GaussianModel activations (gaussian_model.py:84-114); delta layout [xyz3|scale3|rot4|rgb3|op1]
// ---------------------------------------------------------------------------------------------
// exp / log1p of the activations: the SAME sequence of correctly rounded operations as oracle/rast_oracle.c::act_expf / act_log1pf (fma where
// written, + - * /, float <-> int conversions, bit operations; the rasteriser's files are compiled with -ffp-contract=off), so that scales and opacities --
// and with them every radius, tile rect, instance count and sort key of the fused-activation path -- are bit-identical to the oracle's
// (round 6; up to round 5 the device's math library and the oracle's libm differed by an ulp or two and a few of 6.3 M radii flipped).
// Each is within 1 ulp of the true value (tests/test_oracle_rast.py::test_shared_activation_arithmetic_stays_within_2ulp_of_libm).
__device__ __forceinline__ float act_expf(float x) {
    if (x != x) return x;
    if (x > 88.72283f) return __builtin_inff();
    if (x < -103.97208f) return 0.0f;
    const float kf = x * 1.44269502f + (x < 0.0f ? -0.5f : 0.5f);
    const int k = (int)kf;                                   // truncation toward zero = round half away of x log2 e
    const float t = (float)k;
    float r = __builtin_fmaf(t, -0.693145751953125f, x);     // ln 2 = 0.693145751953125 (16 bits: t * it is exact) + 1.42860677e-6
    r = __builtin_fmaf(t, -1.42860677e-6f, r);
    float p = 1.98412698e-4f;                                // e^r, |r| <= 0.347: degree-7 Taylor polynomial, Horner
    p = __builtin_fmaf(p, r, 1.38888889e-3f);
    p = __builtin_fmaf(p, r, 8.33333377e-3f);
    p = __builtin_fmaf(p, r, 4.16666679e-2f);
    p = __builtin_fmaf(p, r, 1.66666672e-1f);
    p = __builtin_fmaf(p, r, 0.5f);
    p = __builtin_fmaf(p, r, 1.0f);
    p = __builtin_fmaf(p, r, 1.0f);
    const int k1 = k / 2, k2 = k - k1;                       // k in [-150, 128]: both factors are normal powers of two
    return (p * __uint_as_float((uint32_t)(k1 + 127) << 23)) * __uint_as_float((uint32_t)(k2 + 127) << 23);
}
__device__ __forceinline__ float act_log1pf(float y) {      // y >= 0 (or NaN)
    if (!(y >= 5.9604645e-8f)) return y;                     // < 2^-24: log1p(y) = y to the last bit (and NaN)
    if (y > 3.4028235e38f) return y;                         // +inf
    int k = 0;
    float c = 0.0f, f = y;
    if (y >= 0.41421354f) {                                  // 1 + y >= sqrt 2: split off the exponent
        const float u = 1.0f + y;
        uint32_t iu = __float_as_uint(u) + (0x3f800000u - 0x3f3504f3u);
        k = (int)(iu >> 23) - 127;
        if (k < 25) c = (k >= 2 ? 1.0f - (u - y) : y - (u - 1.0f)) / u;
        iu = (iu & 0x007fffffu) + 0x3f3504f3u;
        f = __uint_as_float(iu) - 1.0f;
    }
    const float s = f / (2.0f + f);
    const float z = s * s, w = z * z;
    const float t1 = w * (0.40000972152f + w * 0.24279078841f);
    const float t2 = z * (0.66666662693f + w * 0.28498786688f);
    const float R = t2 + t1;
    const float hfsq = (0.5f * f) * f;
    const float dk = (float)k;
    float acc = s * (hfsq + R);
    acc = acc + (dk * 9.0580006145e-6f + c);
    acc = acc - hfsq;
    acc = acc + f;
    return acc + dk * 6.9313812256e-1f;
}
__device__ __forceinline__ float act_scale(float x, const GvfGaussianActivation& a) {
    float s = a.scaling_activation == 0 ? act_expf(x) : (x > 20.0f ? x : act_log1pf(act_expf(x)));
    return sqrtf(s * s + a.min_kernel_size * a.min_kernel_size);
}

struct ActGaussian {
    float p[3], s[3], q[4], op, drgb[3];
};

// The raw parameters of one Gaussian after the operations that do not depend on the delta row: a launch that walks several frames per thread
// (preprocess_kernel<false, true>) loads them once and finishes the activation per frame.
struct ActRaw {
    float p[3], s[3], q[4], op;
};
__device__ __forceinline__ ActRaw activate_raw(int i, const GvfGaussianActivation& a,
                                               const float* __restrict__ xyz_raw,
                                               const float* __restrict__ scaling_raw,
                                               const float* __restrict__ rotation_raw,
                                               const float* __restrict__ opacity_raw) {
    ActRaw r;
#pragma unroll
    for (int k = 0; k < 3; ++k) r.p[k] = xyz_raw[3 * (size_t)i + k] * a.aabb[3 + k] + a.aabb[k];
#pragma unroll
    for (int k = 0; k < 3; ++k) r.s[k] = scaling_raw[3 * (size_t)i + k] + a.scale_bias;
#pragma unroll
    for (int k = 0; k < 4; ++k) r.q[k] = rotation_raw[4 * (size_t)i + k] + (k == 0 ? 1.0f : 0.0f);
    r.op = opacity_raw[i] + a.opacity_bias;
    return r;
}
// dl: the delta row (zeros when d is false -- they are not added then, as the reference's get_* accessors do without a delta)
__device__ __forceinline__ ActGaussian activate_finish(const ActRaw& r, const GvfGaussianActivation& a, const float (&dl)[14], bool d) {
    ActGaussian g;
#pragma unroll
    for (int k = 0; k < 3; ++k) g.p[k] = d ? r.p[k] + dl[k] : r.p[k];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        float x = r.s[k];
        if (d) x = x + dl[3 + k];
        g.s[k] = act_scale(x, a);
    }
    float q[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        q[k] = r.q[k];
        if (d) q[k] = q[k] + dl[6 + k];
    }
    float n = sqrtf(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
    n = fmaxf(n, 1e-12f);
#pragma unroll
    for (int k = 0; k < 4; ++k) g.q[k] = q[k] / n;
    float x = r.op;
    if (d) x = x + dl[13];
    g.op = 1.0f / (1.0f + act_expf(-x));
    g.drgb[0] = dl[10]; g.drgb[1] = dl[11]; g.drgb[2] = dl[12];
    return g;
}
__device__ __forceinline__ ActGaussian activate_vals(int i, const GvfGaussianActivation& a,
                                                     const float* __restrict__ xyz_raw,
                                                     const float* __restrict__ scaling_raw,
                                                     const float* __restrict__ rotation_raw,
                                                     const float* __restrict__ opacity_raw,
                                                     const float (&dl)[14], bool d) {
    return activate_finish(activate_raw(i, a, xyz_raw, scaling_raw, rotation_raw, opacity_raw), a, dl, d);
}
__device__ __forceinline__ ActGaussian activate_one(int i, const GvfGaussianActivation& a,
                                                    const float* __restrict__ xyz_raw,
                                                    const float* __restrict__ scaling_raw,
                                                    const float* __restrict__ rotation_raw,
                                                    const float* __restrict__ opacity_raw,
                                                    const float* __restrict__ d /* delta row or null */) {
    float dl[14];
#pragma unroll
    for (int k = 0; k < 14; ++k) dl[k] = d ? d[k] : 0.0f;
    return activate_vals(i, a, xyz_raw, scaling_raw, rotation_raw, opacity_raw, dl, d != nullptr);
}

__device__ __forceinline__ void xform43(const float* m, const float* p, float* o) {
    o[0] = m[0] * p[0] + m[4] * p[1] + m[8] * p[2] + m[12];
    o[1] = m[1] * p[0] + m[5] * p[1] + m[9] * p[2] + m[13];
    o[2] = m[2] * p[0] + m[6] * p[1] + m[10] * p[2] + m[14];
}
__device__ __forceinline__ void xform44(const float* m, const float* p, float* o) {
    o[0] = m[0] * p[0] + m[4] * p[1] + m[8] * p[2] + m[12];
    o[1] = m[1] * p[0] + m[5] * p[1] + m[9] * p[2] + m[13];
    o[2] = m[2] * p[0] + m[6] * p[1] + m[10] * p[2] + m[14];
    o[3] = m[3] * p[0] + m[7] * p[1] + m[11] * p[2] + m[15];
}

__device__ __forceinline__ void cov3d_from_scale_rot(const float* s, float mod, const float* q, float* c6) {
    float sx = mod * s[0], sy = mod * s[1], sz = mod * s[2];
    float r = q[0], x = q[1], y = q[2], z = q[3];
    float R00 = 1.f - 2.f * (y * y + z * z), R01 = 2.f * (x * y - r * z), R02 = 2.f * (x * z + r * y);
    float R10 = 2.f * (x * y + r * z), R11 = 1.f - 2.f * (x * x + z * z), R12 = 2.f * (y * z - r * x);
    float R20 = 2.f * (x * z - r * y), R21 = 2.f * (y * z + r * x), R22 = 1.f - 2.f * (x * x + y * y);
    float L00 = R00 * sx, L01 = R01 * sy, L02 = R02 * sz;
    float L10 = R10 * sx, L11 = R11 * sy, L12 = R12 * sz;
    float L20 = R20 * sx, L21 = R21 * sy, L22 = R22 * sz;
    c6[0] = L00 * L00 + L01 * L01 + L02 * L02;
    c6[1] = L00 * L10 + L01 * L11 + L02 * L12;
    c6[2] = L00 * L20 + L01 * L21 + L02 * L22;
    c6[3] = L10 * L10 + L11 * L11 + L12 * L12;
    c6[4] = L10 * L20 + L11 * L21 + L12 * L22;
    c6[5] = L20 * L20 + L21 * L21 + L22 * L22;
}

// sh: this Gaussian's coefficients in LDS, [M][3]; dadd: rgb delta added to every coefficient
__device__ __forceinline__ void sh_to_rgb(int deg, const float* sh, const float* dadd, const float* p,
                                          const float* cam, float* rgb) {
    float dx = p[0] - cam[0], dy = p[1] - cam[1], dz = p[2] - cam[2];
    float len = sqrtf(dx * dx + dy * dy + dz * dz);
    float x = dx / len, y = dy / len, z = dz / len;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const float da = dadd[c];
        float res = SH_C0 * (sh[0 * 3 + c] + da);
        if (deg > 0) {
            res = res - SH_C1 * y * (sh[1 * 3 + c] + da) + SH_C1 * z * (sh[2 * 3 + c] + da) -
                  SH_C1 * x * (sh[3 * 3 + c] + da);
            if (deg > 1) {
                float xx = x * x, yy = y * y, zz = z * z, xy = x * y, yz = y * z, xz = x * z;
                res = res + SH_C2[0] * xy * (sh[4 * 3 + c] + da) + SH_C2[1] * yz * (sh[5 * 3 + c] + da) +
                      SH_C2[2] * (2.0f * zz - xx - yy) * (sh[6 * 3 + c] + da) +
                      SH_C2[3] * xz * (sh[7 * 3 + c] + da) + SH_C2[4] * (xx - yy) * (sh[8 * 3 + c] + da);
                if (deg > 2) {
                    res = res + SH_C3[0] * y * (3.0f * xx - yy) * (sh[9 * 3 + c] + da) +
                          SH_C3[1] * xy * z * (sh[10 * 3 + c] + da) +
                          SH_C3[2] * y * (4.0f * zz - xx - yy) * (sh[11 * 3 + c] + da) +
                          SH_C3[3] * z * (2.0f * zz - 3.0f * xx - 3.0f * yy) * (sh[12 * 3 + c] + da) +
                          SH_C3[4] * x * (4.0f * zz - xx - yy) * (sh[13 * 3 + c] + da) +
                          SH_C3[5] * z * (xx - yy) * (sh[14 * 3 + c] + da) +
                          SH_C3[6] * x * (xx - 3.0f * yy) * (sh[15 * 3 + c] + da);
                }
            }
        }
        res += 0.5f;
        rgb[c] = res < 0.f ? 0.f : res;
    }
}

struct TileRect { int x0, y0, x1, y1; };
__device__ __forceinline__ TileRect get_rect(float px, float py, float radius, int gx, int gy) {
    TileRect r;
    r.x0 = min(gx, max(0, (int)((px - radius) / (float)TILE)));
    r.y0 = min(gy, max(0, (int)((py - radius) / (float)TILE)));
    r.x1 = min(gx, max(0, (int)((px + radius + (float)(TILE - 1)) / (float)TILE)));
    r.y1 = min(gy, max(0, (int)((py + radius + (float)(TILE - 1)) / (float)TILE)));
    return r;
}

// Size classes of the per-tile sort (R4, rast_sort.hip; seg_scan_kernel in rast_front.hip files the segments by them).  SORT_SMALL_N: segments of up to this many keys are sorted in static LDS by tile_sort_kernel<0>, one
// workgroup of 256 threads each.  1536 since the end of round 6 (2048 before): 12 bytes of LDS per key = 18.4 KiB = EIGHT workgroups per CU instead
// of six -- the launch lives on how many segments are in flight (its waves are parked 75 % of the time) --; the few segments of 1537-2048 keys join
// the 512-thread LDS class.  Tile sort 0.137 -> 0.119 ms at the bench shape, the live render job -4 % (profiles/r06_tile_sort_classes.txt; sorting
// the segments of up to 256-512 keys four to a workgroup, one WAVE each, was built and measured on top of it: -3 % of the launch at best, not kept).
#ifndef GVF_SORT_SMALL_N                // (a variant build passes it to rast_front.hip AND rast_sort.hip)
#define GVF_SORT_SMALL_N 1536
#endif
constexpr int SORT_SMALL_N = GVF_SORT_SMALL_N;
static_assert(SORT_SMALL_N == 1536 || SORT_SMALL_N == 2048, "register class of the per-tile sort: 6 or 8 keys per thread");
constexpr int SORT_LARGE_N = 16384;
constexpr int SORT_LARGE_BLOCKS = 256, SORT_HUGE_BLOCKS = 64;   // grid of the launch that walks the two rare classes
constexpr int SORT_MEDIUM_N = 4096, SORT_MEDIUM_BLOCKS = 768;   // the LDS class's lower half has a launch of its own (tile_sort_kernel<1>)

// Which of the tile's four 8x8 quadrants can a splat reach with alpha >= 1/255?  Exact (up to a safety margin) test of
// the ellipse  e(dx, dy) = a' dx^2 + b' dx dy + c' dy^2 >= -log2(255 opacity)  against each quadrant's rectangle: e is
// concave, so its maximum over a rectangle that does not contain the centre sits on one of the four edges, at the
// clamped vertex of a 1-D parabola.  (The axis-aligned box (hx, hy) that the binning uses keeps ~25 % more pairs: the
// corners of the box of a rotated, elongated ellipse.)  The test only decides which (splat, quadrant) pairs are
// evaluated; a kept splat is evaluated by the compositing step's own arithmetic (the Cholesky form described above) and
// a culled one would have failed alpha >= 1/255 at every pixel of the quadrant (margin: 0.02 octaves on the threshold
// against ~1e-5 of rounding), so images do not depend on the test.
// max over t in [lo, hi] of  qa fixed^2 + qb fixed t + qc t^2   (qc < 0), the vertex slope kv = -qb / (2 qc) handed in: one hardware
// reciprocal per splat and orientation instead of an IEEE division per edge (round 3: the staging loop spent 8 divisions = ~100 of its 265
// vector instructions per instance on them; blend 0.87 -> 0.82 ms).  An inexact vertex only LOWERS the value (any t of the interval is a
// lower bound of a concave function's maximum) by ~qc dt^2 ~ 1e-13 -- against the 0.02-octave margin of the test, i.e. never visibly; the
// forward and the backward kernel share this function, so they evaluate the same splats.
// (written with explicit fmas: the rasteriser's files are compiled with -ffp-contract=off for the arithmetic it shares with the oracle, and as separate multiplies
// and adds the four edges of the four quadrants were 110 of the staging pass's 204 vector instructions per instance; the test has a 0.02-octave
// margin and is shared by the forward and the backward kernel, so its rounding only has to be the same in both)
__device__ __forceinline__ float edge_max(float qa, float qb, float qc, float kv, float fixed, float lo, float hi) {
    const float t = fminf(fmaxf(kv * fixed, lo), hi);                                   // the vertex of the parabola along the edge, clamped
    return __builtin_fmaf(__builtin_fmaf(qc, t, qb * fixed), t, (qa * fixed) * fixed);  // qa fixed^2 + (qb fixed + qc t) t
}
__device__ __forceinline__ unsigned quadrant_mask(float x, float y, float ap, float bp, float cp, float op, float hx,
                                                  float tile_x0, float tile_y0, bool no_cull) {
    if (hx < 0.0f) return 0u;                            // opacity < 1/255: alpha < 1/255 at every pixel
    if (no_cull || !(hx < __builtin_inff())) return 0xFu; // sub-pixel offsets / degenerate conic: keep everywhere
    const float lim = -(__log2f(255.0f * op) + 0.02f);
    const float kx = -0.5f * bp * __builtin_amdgcn_rcpf(cp), ky = -0.5f * bp * __builtin_amdgcn_rcpf(ap);   // vertex slopes: dy* = kx dx, dx* = ky dy
    const float xr = x - tile_x0, yr = y - tile_y0;
    unsigned m = 0u;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const float ox = (float)((q & 1) * 8), oy = (float)((q >> 1) * 8);
        const float dxl = xr - (ox + 7.0f), dxh = xr - ox, dyl = yr - (oy + 7.0f), dyh = yr - oy;   // offset ranges over the quadrant
        const bool inside = dxl <= 0.0f && dxh >= 0.0f && dyl <= 0.0f && dyh >= 0.0f;
        float e = edge_max(ap, bp, cp, kx, dxl, dyl, dyh);
        e = fmaxf(e, edge_max(ap, bp, cp, kx, dxh, dyl, dyh));
        e = fmaxf(e, edge_max(cp, bp, ap, ky, dyl, dxl, dxh));
        e = fmaxf(e, edge_max(cp, bp, ap, ky, dyh, dxl, dxh));
        m |= (inside || e >= lim) ? (1u << q) : 0u;
    }
    return m;
}

constexpr int BWD_ACC = 10;   // per Gaussian: d/dx, d/dy [pixels], d/d(conic a, b, c), d/d(opacity_eff), d/d(r, g, b), d/d(depth)

}  // namespace

namespace gvf_rast {   // host side: what crosses a file boundary

struct Workspace {
    GvfRastFrame* frames;
    float4* splats;   // [F*P][4]: 64-byte records
    uint32_t* tiles_touched; int32_t* radii;
    uint32_t* block_sums; uint32_t* frame_base; uint32_t* total;
    uint64_t* keys; uint64_t* keys_alt; uint32_t* vals; uint32_t* vals_alt; uint32_t* ids;
    uint2* ranges; uint32_t* cls;
    uint32_t* tile_count; uint32_t* cursor;            // bucket binning: [F*ntiles] each
    uint32_t* partial;
    uint32_t* order; uint32_t* order_alt; uint32_t* mhist; uint32_t* mm;
    uint4* binrec;                                     // room for [F*P] 16-byte bin records {x0|y0<<16, x1|y1<<16, depth bits, -}; a call whose
                                                       // plan says rec8 keeps [F*P] 8-byte ones {x0|y0<<8|x1<<16|y1<<24, depth bits} in its first half
    void* sort_tmp; size_t sort_tmp_bytes;
    size_t bytes; bool ok;
};

// rast.hip: the layout of a call's workspace -- the forward and the backward of a call carve it with the same arguments
Workspace carve(void* ws, size_t bytes, int P, int F, int H, int W, int64_t max_rendered);

// One forward call's arguments, as the entry points hand them to the pipeline and the pipeline to the front end.  Inputs are either
// activated tensors (fused = false: a0 = means3D, a1 = scales, a2 = rotations, a3 = opacities, sh = shs) or raw GaussianModel parameters
// (fused: a0 = _xyz, a1 = _scaling, a2 = _rotation, a3 = _opacity, sh = _features_dc, delta[n_delta][P][14]).
struct RastCall {
    const GvfRastSettings* st; const GvfRastFrame* frames_host; int F, P, M;
    bool fused; const GvfGaussianActivation* act;
    const float *a0, *a1, *a2, *a3, *sh, *colors_precomp, *cov3D_precomp, *delta; int n_delta;
    const float* subpixel_offset;
    int64_t max_rendered;
    int32_t* out_radii; uint32_t* out_num_rendered;
};

// Stage-timer mark k of a profiled call (gvf_rast_profile_*): marks = the call's events, null when the call is not timed
inline void prof_mark(hipStream_t s, const hipEvent_t* marks, int k) {
    if (marks != nullptr) (void)hipEventRecord(marks[k], s);
}

// rast_front.hip: the launches in front of the per-tile sort, from the call's plan (rast_plan.h).  upload_frames: the camera blocks to
// w.frames, and the call's tables cleared.  front_end_*: one per binning algorithm, marks 0 .. 5 at the stage boundaries; they leave the
// tile ranges, the per-frame counts and the unsorted tile segments (bucket: keys in w.keys; radix: where *keys_sorted / *vals_by_tile say).
int upload_frames(hipStream_t stream, const RastCall& c, const RastPlan& plan, const Workspace& w);
int front_end_bucket(hipStream_t stream, const RastCall& c, const RastPlan& plan, const Workspace& w, const hipEvent_t* marks);
int front_end_radix(hipStream_t stream, const RastCall& c, const RastPlan& plan, const Workspace& w, const hipEvent_t* marks,
                    uint64_t** keys_sorted, uint32_t** vals_by_tile);

// rast_sort.hip: classify + the size classes of the per-tile sort over nseg segments (cls: 2 + 2 nseg words of scratch; cls_state: see there)
int launch_tile_sort(hipStream_t stream, const uint2* ranges, uint64_t* keys, const uint32_t* vals, uint32_t* ids, uint32_t* cls,
                     uint32_t nseg, int cls_state);
int tile_sort_set_lds_limit();

// rast_blend.hip: blend_kernel over (tiles, F); tile_order non-null: blend_order_kernel first (heaviest tiles first, the order goes to
// tile_order).  `ordered`, when non-null, is recorded between the two (the profiler's stage boundary)
int launch_blend(hipStream_t stream, const GvfRastSettings& st, int P, int F, const uint2* ranges, const uint32_t* point_list,
                 const float4* splats, const float* subpixel_offset, float* out_color, float* out_alpha, float* out_depth,
                 unsigned char* out_u8, const uint32_t* rec_of, uint32_t* tile_order, hipEvent_t ordered);
}  // namespace gvf_rast
using namespace gvf_rast;
