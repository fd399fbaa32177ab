// rast_front.hip -- the rasteriser's front end (R1..R3, R5 + G1): every kernel that runs in front of the per-tile sort -- the GaussianModel
// activations, the Morton order, preprocess, the bin passes, the scans, the radix comparison path's duplicate / ranges, the upload launch --
// and the host functions that launch them from a call plan (rast_plan.h): upload_frames, front_end_bucket, front_end_radix.  The pipeline
// that calls them and the overview of the launch structure are in rast.hip.  The arithmetic is the floating-point contract of
// oracle/rast_oracle.c (this file is compiled with -ffp-contract=off).  All front-end kernels live in this one file, so that each keeps the
// inlining context it was tuned in.
#include "rast_common.h"
#include "gvf_sort.h"

namespace {

// preprocess_kernel runs on a (Gaussian blocks, frame groups) grid.  Measured and not adopted (profiles/r05_preprocess_variants_ab.txt): an
// XCD-aware workgroup order and requesting the next frame's delta row ahead -- the launch waits neither on L2 hits nor on bytes in flight.
// The fused launch reads its delta rows straight from global memory: staging them through LDS costs occupancy and is slower
// (profiles/r07_preprocess_forms_ab.txt).
// Bucket binning of the calls without shared activation (preprocess_kernel<false>): the bin records are stored at the Gaussian's own index
// (coalesced lines), the count pass (bin_index_kernel) walks them in index order against a whole-frame LDS tile table, and the scatter pass
// (bin_kernel) gathers them in Morton order, each XCD taking whole frames.  Records at the Morton slot, or both passes in one order, are
// slower (profiles/r07_bin_layout_ab.txt).  The shared-activation path keeps its records at the Morton slot.
// The bin records come in two forms, chosen by the call's plan (RastPlan::rec8) and compiled into preprocess_kernel, bin_index_kernel and
// bin_kernel as a template argument: 8 bytes (BinRec8) when the tile grid is at most 255 x 255, so that a rect coordinate fits 8 bits --
// half the bytes through the stores and both passes, and a frame's records (P x 8 B) fit one XCD's L2 in the gather at P = 262144 --, else
// 16 bytes (BinRec16).  Both hold the rect and the depth bits losslessly: the keys and counts of a call are the same either way.

struct PreParams {
    int P, M, deg, H, W, mode;
    int gx, gy;           // tile grid
    float kernel_size, scale_modifier;
    // fused activation (raw GaussianModel parameters) -- used when fused != 0
    int fused;
    GvfGaussianActivation act;
    int n_delta;
    int upstream_binning;   // 1: bin the whole 3-sigma tile rect as upstream does
    int F;                  // frames of the call (grid.y covers them PRE_FB at a time)
    int delta_lds;          // read by no kernel (always 0); kept so that the kernel arguments stay as they are
};

__global__ __launch_bounds__(256) void activate_kernel(GvfGaussianActivation a, int P, int M,
                                                       const float* __restrict__ xyz_raw,
                                                       const float* __restrict__ features_dc,
                                                       const float* __restrict__ scaling_raw,
                                                       const float* __restrict__ rotation_raw,
                                                       const float* __restrict__ opacity_raw,
                                                       const float* __restrict__ delta, float* __restrict__ means3D,
                                                       float* __restrict__ scales, float* __restrict__ rotations,
                                                       float* __restrict__ shs, float* __restrict__ opacities) {
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= P) return;
    const float* d = delta ? delta + 14 * (size_t)i : nullptr;
    ActGaussian g = activate_one(i, a, xyz_raw, scaling_raw, rotation_raw, opacity_raw, d);
    for (int k = 0; k < 3; ++k) { means3D[3 * (size_t)i + k] = g.p[k]; scales[3 * (size_t)i + k] = g.s[k]; }
    for (int k = 0; k < 4; ++k) rotations[4 * (size_t)i + k] = g.q[k];
    opacities[i] = g.op;
    for (int m = 0; m < M; ++m)
        for (int c = 0; c < 3; ++c) {
            float v = features_dc[((size_t)i * M + m) * 3 + c];
            shs[((size_t)i * M + m) * 3 + c] = d ? v + g.drgb[c] : v;
        }
}

// ---------------------------------------------------------------------------------------------
// R1: preprocess
// ---------------------------------------------------------------------------------------------
// Shared activation (round 5).  The reference renders one timestep from many cameras (utils/inference_utils.py:256-269: for t in 32, for cam in
// 128), i.e. consecutive frames of a batched call select the SAME delta slice: activations (gaussian_model.py:84-114) and the 3-D covariance do
// not depend on the camera.  When a call's F frames use few distinct slices, stage A computes them once per (slice, Gaussian) into a 64-byte
// record {x, y, z, opacity | S00, S01, S02, S11 | S12, S22, drgb0, drgb1 | drgb2, -, -, -} and preprocess_kernel<true> reads the record
// (one cache line, four 16-byte loads) instead of 112 B of strided raw inputs + the activation arithmetic per frame.  Same functions, same
// operation order, no contraction (-ffp-contract=off): every output bit equals the fused path's (tests/test_rast_gpu.py::test_shared_activation_*).
struct ActSlices { int n; int di[ACT_MAX_SLICES]; };
__global__ __launch_bounds__(256) void activate_cov_kernel(GvfGaussianActivation a, float scale_modifier, int P, ActSlices sl,
                                                           const float* __restrict__ xyz_raw, const float* __restrict__ scaling_raw,
                                                           const float* __restrict__ rotation_raw, const float* __restrict__ opacity_raw,
                                                           const float* __restrict__ delta, float4* __restrict__ rec3d,
                                                           const uint32_t* __restrict__ slot_of /* Gaussian -> Morton slot, or null */,
                                                           const float* __restrict__ sh, int sh_floats, float* __restrict__ sh_by_slot) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= P) return;
    // SLOT ORDER (slot_of != null): the record of Gaussian i goes to its Morton slot (a whole 64-byte line, scattered ONCE per slice) and slice 0's
    // workgroups also copy the SH rows into slot order; the per-frame launch then runs over slots: its record reads, its splat records and its bin
    // records (8 or 16 bytes each, scattered to the slot by the index-ordered form: 21 % of that launch at 16) are all contiguous.
    const size_t dst = slot_of != nullptr ? (size_t)slot_of[i] : (size_t)i;
    if (sh_by_slot != nullptr && blockIdx.y == 0)
        for (int k = 0; k < sh_floats; ++k) sh_by_slot[dst * sh_floats + k] = sh[(size_t)i * sh_floats + k];
    const int di = sl.di[blockIdx.y];
    const float* d = (delta != nullptr && di >= 0) ? delta + ((size_t)di * P + i) * 14 : nullptr;
    const ActGaussian g = activate_one(i, a, xyz_raw, scaling_raw, rotation_raw, opacity_raw, d);
    float c6[6];
    cov3d_from_scale_rot(g.s, scale_modifier, g.q, c6);
    float4* r = rec3d + 4 * ((size_t)blockIdx.y * P + dst);
    r[0] = make_float4(g.p[0], g.p[1], g.p[2], g.op);
    r[1] = make_float4(c6[0], c6[1], c6[2], c6[3]);
    r[2] = make_float4(c6[4], c6[5], g.drgb[0], g.drgb[1]);
    r[3] = make_float4(g.drgb[2], 0.f, 0.f, 0.f);
}

// Inputs are either activated tensors (fused == 0: a0=means3D, a1=scales, a2=rotations, a3=opacities,
// sh=shs/colors) or raw GaussianModel parameters (fused != 0: a0=_xyz, a1=_scaling, a2=_rotation,
// a3=_opacity, sh=_features_dc, delta[n_delta][P][14]).
// Half extents (hx, hy) of the axis-aligned box around the splat centre outside which
// alpha = opacity * exp(power) < 1/255 for certain ( ca dx^2 + 2 cb dx dy + cc dy^2 <= 2 ln(255 opacity) ),
// inflated so that float noise can only keep extra splats, never drop one.  hx < 0: never visible;
// +inf: degenerate conic, keep everywhere.  Built from correctly rounded + * / sqrt and bit operations only
// (ln_upper: exponent + tangent envelope of log2, no libm), so oracle/rast_oracle.c reproduces them bit for
// bit and the culled instance counts can be compared exactly.  Used for (1) instance culling: a (Gaussian,
// tile) pair whose tile the box does not reach is never binned -- the blend would skip it at every pixel --
// and (2) the blend's per-quadrant culling.
__device__ __forceinline__ float ln_upper(float z) {
    const uint32_t b = __float_as_uint(z);
    const int e = (int)(b >> 23) - 127;
    const float m = __uint_as_float((b & 0x7fffffu) | 0x3f800000u);
    float L = (m - 1.0f) * 1.4426951f;
    L = fminf(L, 0.32192809f + (m - 1.25f) * 1.1541561f);
    L = fminf(L, 0.5849625f + (m - 1.5f) * 0.96179669f);
    L = fminf(L, 0.80735492f + (m - 1.75f) * 0.8243972f);
    L = fminf(L, 1.0f + (m - 2.0f) * 0.72134752f);
    return ((float)e + (L + 1e-5f)) * 0.69314724f;
}

__device__ __forceinline__ float2 cull_extent(float ca, float cb, float cc, float op) {
    if (op < 1.0f / 255.0f) return make_float2(-1.0f, -1.0f);
    const float det = ca * cc - cb * cb;
    const float inf = __builtin_inff();
    if (!(det > 0.0f) || !(ca > 0.0f) || !(cc > 0.0f)) return make_float2(inf, inf);
    const float tau = 2.0f * ln_upper(255.0f * op) * 1.001f + 1e-3f;
    const float inv = 1.0f / det;
    return make_float2(sqrtf(tau * cc * inv) * 1.001f + 0.01f, sqrtf(tau * ca * inv) * 1.001f + 0.01f);
}

// tiles t owning a pixel p in [16t, 16t+15] with |p - c| <= h, clipped to [lo, hi)
__device__ __forceinline__ void tight_range(float c, float h, int lo, int hi, int n, int& t0, int& t1) {
    if (h < 0.0f) { t0 = lo; t1 = lo; return; }
    const float a = fminf(fmaxf(ceilf((c - h - (float)(TILE - 1)) / (float)TILE), 0.0f), (float)n);
    const float b = fminf(fmaxf(floorf((c + h) / (float)TILE) + 1.0f, 0.0f), (float)n);
    t0 = max((int)a, lo);
    t1 = min((int)b, hi);
    if (t1 < t0) t1 = t0;
}

__device__ __forceinline__ TileRect tight_rect(TileRect r, float px, float py, float hx, float hy, int gx, int gy) {
    TileRect t;
    tight_range(px, hx, r.x0, r.x1, gx, t.x0, t.x1);
    tight_range(py, hy, r.y0, r.y1, gy, t.y0, t.y1);
    return t;
}

// Bin record of a (frame, Gaussian): the final tile rect and the depth bits.  An empty rect is all-zero coordinates.
//   BinRec16 = uint4 {x0 | y0 << 16, x1 | y1 << 16, depth bits, 0}                any grid
//   BinRec8  = uint2 {x0 | y0 << 8 | x1 << 16 | y1 << 24, depth bits}             gx, gy <= BIN_REC8_MAX_GRID (coordinates lie in [0, gx], [0, gy])
typedef uint4 BinRec16;
typedef uint2 BinRec8;
template <typename REC> __device__ __forceinline__ REC binrec_pack(TileRect r, uint32_t depth_bits);
template <> __device__ __forceinline__ BinRec16 binrec_pack<BinRec16>(TileRect r, uint32_t depth_bits) {
    return make_uint4((uint32_t)r.x0 | ((uint32_t)r.y0 << 16), (uint32_t)r.x1 | ((uint32_t)r.y1 << 16), depth_bits, 0u);
}
template <> __device__ __forceinline__ BinRec8 binrec_pack<BinRec8>(TileRect r, uint32_t depth_bits) {
    return make_uint2((uint32_t)r.x0 | ((uint32_t)r.y0 << 8) | ((uint32_t)r.x1 << 16) | ((uint32_t)r.y1 << 24), depth_bits);
}
__device__ __forceinline__ TileRect binrec_rect16(uint32_t w0, uint32_t w1) {
    return TileRect{(int)(w0 & 0xffffu), (int)(w0 >> 16), (int)(w1 & 0xffffu), (int)(w1 >> 16)};
}
__device__ __forceinline__ TileRect binrec_rect8(uint32_t w) {
    return TileRect{(int)(w & 0xffu), (int)((w >> 8) & 0xffu), (int)((w >> 16) & 0xffu), (int)(w >> 24)};
}
__device__ __forceinline__ TileRect binrec_rect(const BinRec16& b) { return binrec_rect16(b.x, b.y); }
__device__ __forceinline__ TileRect binrec_rect(const BinRec8& b) { return binrec_rect8(b.x); }
__device__ __forceinline__ uint32_t binrec_depth(const BinRec16& b) { return b.z; }
__device__ __forceinline__ uint32_t binrec_depth(const BinRec8& b) { return b.y; }

// SHARED: a0 = the stage-A records [slices][P][4 x float4] (see activate_cov_kernel), frames[f].reserved[0] = the frame's slice
// WAVE_FRAMES (bucket binning without shared activation; block_sums and tiles_touched are null by construction): the workgroup owns 64
// consecutive Gaussians instead of 256 and its four waves walk different frames -- wave w takes frames 4 G by + w + 4 ff, ff = 0 .. G - 1
// (G = PRE_WAVE_FB) -- so the SH rows are staged once per 4 G frames and the raw inputs come across the fabric once per 4 G frames, on a grid
// that keeps ceil(P / 64) x ceil(F / 4G) workgroups.  One barrier, after the staging; the waves never meet again.  What a wave loads and stores
// per frame (delta rows, quad-transposed splat records, bin records) and the per-Gaussian arithmetic are those of the other mapping.
// REC: the bin-record form (binrec points at [F*P] of them).
template <bool SHARED, bool WAVE_FRAMES = false, typename REC = BinRec16>
__global__ __launch_bounds__(PRE_THREADS) void preprocess_kernel(
    PreParams pp, const GvfRastFrame* __restrict__ frames, const float* __restrict__ a0,
    const float* __restrict__ a1, const float* __restrict__ a2, const float* __restrict__ a3,
    const float* __restrict__ sh, const float* __restrict__ colors_precomp,
    const float* __restrict__ cov3D_precomp, const float* __restrict__ delta, float4* __restrict__ splats,
    uint32_t* __restrict__ tiles_touched,
    int32_t* __restrict__ radii, uint32_t* __restrict__ block_sums, REC* __restrict__ binrec,
    const uint32_t* __restrict__ bin_slot /* Gaussian -> position of its bin record inside a frame; null = identity */) {
    static_assert(!(SHARED && WAVE_FRAMES), "the shared-activation launch keeps the 256-Gaussian mapping");
    extern __shared__ __attribute__((aligned(16))) float sh_lds[];  // [PRE_GPB][M*3] + 4 wave sums
    constexpr int PRE_GPB = WAVE_FRAMES ? GVF_WAVE : PRE_THREADS;   // Gaussians per workgroup
    const int t = threadIdx.x;
    const int P = pp.P, M = pp.M;
    const int nbx = (P + PRE_THREADS - 1) / PRE_THREADS;
    const int bx = blockIdx.x, by = blockIdx.y;
    const int row = WAVE_FRAMES ? (t & (GVF_WAVE - 1)) : t;        // this thread's Gaussian inside the workgroup (= its SH row in LDS)
    const int i = bx * PRE_GPB + row;

    // Stage this block's SH coefficients through LDS with coalesced 16-byte loads: PRE_GPB Gaussians x
    // M*3 floats are one contiguous span of the [P][M][3] tensor.
    const int sh_stride = M * 3;
    if (sh != nullptr) {
        const size_t span0 = (size_t)bx * PRE_GPB * sh_stride;
        const int nvalid = min(PRE_GPB, P - bx * PRE_GPB);
        const int total = nvalid * sh_stride;
        const float4* src4 = reinterpret_cast<const float4*>(sh + span0);  // span0*4 B is 16-B aligned
        float4* dst4 = reinterpret_cast<float4*>(sh_lds);
        const int n4 = total >> 2;
        for (int k = t; k < n4; k += PRE_THREADS) dst4[k] = src4[k];
        for (int k = (n4 << 2) + t; k < total; k += PRE_THREADS) sh_lds[k] = sh[span0 + k];
    }
    __syncthreads();

  const uint32_t my_slot = (bin_slot != nullptr && i < P) ? bin_slot[i] : (uint32_t)i;
  // wave-frames mapping: the raw parameters and their delta-independent first operations once, in front of the frame loop (78 -> 90 vector
  // registers, 5 waves per SIMD as on the other mapping: -23 us per launch at 24 frames)
  ActRaw raw = {};
  if (WAVE_FRAMES && pp.fused && i < P) raw = activate_raw(i, pp.act, a0, a1, a2, a3);
  // first frame, frame stride and frame count of this thread's wave.  The wave index goes through readfirstlane: the frame index must be
  // a scalar, or the camera block (frames[f]: 40 floats) is fetched with per-lane loads into vector registers instead of s_load into scalars
  const int f_first = WAVE_FRAMES ? by * (PRE_WAVES * PRE_WAVE_FB) + __builtin_amdgcn_readfirstlane(t >> 6) : by * PRE_FB;
  constexpr int F_STEP = WAVE_FRAMES ? PRE_WAVES : 1, F_COUNT = WAVE_FRAMES ? PRE_WAVE_FB : PRE_FB;
#pragma unroll 1
  for (int ff = 0; ff < F_COUNT; ++ff) {
    const int f = f_first + ff * F_STEP;
    if (f >= pp.F) break;
    const GvfRastFrame* fr = frames + f;
    uint32_t touched = 0;
    int radius_out = 0;
    float4 gA = make_float4(0.f, 0.f, 0.f, 0.f), gB = gA, gC = gA;
    TileRect rect = {0, 0, 0, 0};

    if (i < P) {
        float p[3], s[3], q[4], op, dadd[3] = {0.f, 0.f, 0.f};
        float c6s[6];
        if (SHARED) {
            const float4* r3 = reinterpret_cast<const float4*>(a0) + 4 * ((size_t)fr->reserved[0] * P + i);
            const float4 r0 = r3[0], r1 = r3[1], r2 = r3[2], r3v = r3[3];
            p[0] = r0.x; p[1] = r0.y; p[2] = r0.z; op = r0.w;
            c6s[0] = r1.x; c6s[1] = r1.y; c6s[2] = r1.z; c6s[3] = r1.w; c6s[4] = r2.x; c6s[5] = r2.y;
            dadd[0] = r2.z; dadd[1] = r2.w; dadd[2] = r3v.x;
        } else if (pp.fused) {
            const int di = fr->delta_index;
            const float* d = (delta != nullptr && di >= 0) ? delta + ((size_t)di * P + i) * 14 : nullptr;
            ActGaussian g;
            if (WAVE_FRAMES) {
                float dl[14];
#pragma unroll
                for (int k = 0; k < 14; ++k) dl[k] = d ? d[k] : 0.0f;
                g = activate_finish(raw, pp.act, dl, d != nullptr);
            } else {
                g = activate_one(i, pp.act, a0, a1, a2, a3, d);
            }
#pragma unroll
            for (int k = 0; k < 3; ++k) { p[k] = g.p[k]; s[k] = g.s[k]; dadd[k] = g.drgb[k]; }
#pragma unroll
            for (int k = 0; k < 4; ++k) q[k] = g.q[k];
            op = g.op;
        } else {
#pragma unroll
            for (int k = 0; k < 3; ++k) p[k] = a0[3 * (size_t)i + k];
            if (cov3D_precomp == nullptr) {
#pragma unroll
                for (int k = 0; k < 3; ++k) s[k] = a1[3 * (size_t)i + k];
#pragma unroll
                for (int k = 0; k < 4; ++k) q[k] = a2[4 * (size_t)i + k];
            }
            op = a3[i];
        }

        float pv[3];
        xform43(fr->viewmatrix, p, pv);
        bool vis = pv[2] > 0.2f;
        if (vis) {
            float ph[4];
            xform44(fr->projmatrix, p, ph);
            float pw = 1.0f / (ph[3] + 0.0000001f);
            float projx = ph[0] * pw, projy = ph[1] * pw;

            float c6[6];
            if (SHARED) {
#pragma unroll
                for (int k = 0; k < 6; ++k) c6[k] = c6s[k];
            } else if (!pp.fused && cov3D_precomp != nullptr) {
#pragma unroll
                for (int k = 0; k < 6; ++k) c6[k] = cov3D_precomp[6 * (size_t)i + k];
            } else {
                cov3d_from_scale_rot(s, pp.scale_modifier, q, c6);
            }

            const float tanfovx = fr->tanfovx, tanfovy = fr->tanfovy;
            float focal_x = (float)pp.W / (2.0f * tanfovx);
            float focal_y = (float)pp.H / (2.0f * tanfovy);
            float limx = 1.3f * tanfovx, limy = 1.3f * tanfovy;
            float txtz = pv[0] / pv[2], tytz = pv[1] / pv[2];
            float tx = fminf(limx, fmaxf(-limx, txtz)) * pv[2];
            float ty = fminf(limy, fmaxf(-limy, tytz)) * pv[2];
            float tz = pv[2];
            float J00 = focal_x / tz, J02 = -(focal_x * tx) / (tz * tz);
            float J11 = focal_y / tz, J12 = -(focal_y * ty) / (tz * tz);
            float A0[3], A1[3];
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                float w0 = fr->viewmatrix[c * 4 + 0], w1 = fr->viewmatrix[c * 4 + 1], w2 = fr->viewmatrix[c * 4 + 2];
                A0[c] = J00 * w0 + J02 * w2;
                A1[c] = J11 * w1 + J12 * w2;
            }
            float S[3][3] = {{c6[0], c6[1], c6[2]}, {c6[1], c6[3], c6[4]}, {c6[2], c6[4], c6[5]}};
            float B0[3], B1[3];
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                B0[c] = A0[0] * S[0][c] + A0[1] * S[1][c] + A0[2] * S[2][c];
                B1[c] = A1[0] * S[0][c] + A1[1] * S[1][c] + A1[2] * S[2][c];
            }
            float cxx = B0[0] * A0[0] + B0[1] * A0[1] + B0[2] * A0[2];
            float cxy = B0[0] * A1[0] + B0[1] * A1[1] + B0[2] * A1[2];
            float cyy = B1[0] * A1[0] + B1[1] * A1[1] + B1[2] * A1[2];

            float coef = 1.0f;
            if (pp.mode == GVF_RAST_MODE_MIP) {
                float det0 = fmaxf(1e-6f, cxx * cyy - cxy * cxy);
                float det1 = fmaxf(1e-6f, (cxx + pp.kernel_size) * (cyy + pp.kernel_size) - cxy * cxy);
                coef = sqrtf(det0 / (det1 + 1e-6f) + 1e-6f);
                if (det0 <= 1e-6f || det1 <= 1e-6f) coef = 0.0f;
                cxx += pp.kernel_size;
                cyy += pp.kernel_size;
            } else {
                cxx += 0.3f;
                cyy += 0.3f;
            }
            float det = cxx * cyy - cxy * cxy;
            if (det != 0.0f) {
                float det_inv = 1.f / det;
                float ca = cyy * det_inv, cb = -cxy * det_inv, cc = cxx * det_inv;
                float mid = 0.5f * (cxx + cyy);
                float lam1 = mid + sqrtf(fmaxf(0.1f, mid * mid - det));
                float lam2 = mid - sqrtf(fmaxf(0.1f, mid * mid - det));
                float my_radius = ceilf(3.f * sqrtf(fmaxf(lam1, lam2)));
                float px = ((projx + 1.0f) * (float)pp.W - 1.0f) * 0.5f;
                float py = ((projy + 1.0f) * (float)pp.H - 1.0f) * 0.5f;
                TileRect r = get_rect(px, py, my_radius, pp.gx, pp.gy);
                uint32_t cnt = (uint32_t)((r.x1 - r.x0) * (r.y1 - r.y0));
                if (cnt != 0) {
                    float rgb[3];
                    if (colors_precomp != nullptr) {
                        rgb[0] = colors_precomp[3 * (size_t)i + 0];
                        rgb[1] = colors_precomp[3 * (size_t)i + 1];
                        rgb[2] = colors_precomp[3 * (size_t)i + 2];
                    } else {
                        sh_to_rgb(pp.deg, sh_lds + row * sh_stride, dadd, p, fr->campos, rgb);
                    }
                    radius_out = (int)my_radius;
                    const float2 ext = cull_extent(ca, cb, cc, op * coef);
                    if (!pp.upstream_binning) {
                        r = tight_rect(r, px, py, ext.x, ext.y, pp.gx, pp.gy);
                        cnt = (uint32_t)((r.x1 - r.x0) * (r.y1 - r.y0));
                    }
                    touched = cnt;
                    rect = r;
                    gA = make_float4(px, py, ca * CONIC_K1, cb * CONIC_K2);
                    gB = make_float4(cc * CONIC_K1, op * coef, rgb[0], rgb[1]);
                    gC = make_float4(rgb[2], pv[2], ext.x, ext.y);
                }
            }
        }
        const size_t o = (size_t)f * P + i;
        if (!WAVE_FRAMES && tiles_touched != nullptr) tiles_touched[o] = touched;   // radix binning only
        if (radii != nullptr) {
            // slot order (SHARED with a1 = the slot -> Gaussian table): thread i works on slot i, the radii stay indexed by Gaussian
            const uint32_t* gid_of = SHARED ? reinterpret_cast<const uint32_t*>(a1) : nullptr;
            radii[gid_of != nullptr ? (size_t)f * P + gid_of[i] : o] = radius_out;
        }
        // bucket binning: the final tile rect and the depth, 8 or 16 B that the count / scatter passes read (one store per lane: whole
        // lines per wave in index and slot order)
        if (binrec != nullptr) binrec[(size_t)f * P + my_slot] = binrec_pack<REC>(rect, __float_as_uint(gC.y));
    }

    // Quad-transposed record store: lane 4 g + j writes piece j (16 bytes; piece 3 = the padding) of the records of lanes
    // 4 g + k, k = 0 .. 3, so ONE instruction stores 16 whole 64-byte lines where the per-lane form stores 64 quarter lines three times (48 of a
    // line's 64 bytes, masked at the memory side).  The launch is bound by its stores (no record stores: -26 %, no bin-record stores: -21 %,
    // profiles/r05_preprocess_store_ablation.txt); this form: live job 146-148 -> 141-142 ms per sample.  All 64 lanes run it (a lane past P or
    // with a culled Gaussian has touched = 0 and zero pieces), lanes of a quad exchange through DPP quad broadcasts.
    const int lj = t & 3;
    float4* qbase = splats + 4 * ((size_t)f * P + (size_t)(i & ~3));
#define GVF_QB(v_, k_) __builtin_bit_cast(float, __builtin_amdgcn_mov_dpp(__builtin_bit_cast(int, (v_)), (k_) * 0x55, 0xF, 0xF, true))
#define GVF_QSTORE(k_)                                                                                          \
    {                                                                                                       \
        const int tk = __builtin_amdgcn_mov_dpp((int)touched, (k_) * 0x55, 0xF, 0xF, true);                 \
        float4 o4;                                                                                          \
        { const float a = GVF_QB(gA.x, k_), b = GVF_QB(gB.x, k_), c = GVF_QB(gC.x, k_); o4.x = lj == 0 ? a : (lj == 1 ? b : (lj == 2 ? c : 0.f)); } \
        { const float a = GVF_QB(gA.y, k_), b = GVF_QB(gB.y, k_), c = GVF_QB(gC.y, k_); o4.y = lj == 0 ? a : (lj == 1 ? b : (lj == 2 ? c : 0.f)); } \
        { const float a = GVF_QB(gA.z, k_), b = GVF_QB(gB.z, k_), c = GVF_QB(gC.z, k_); o4.z = lj == 0 ? a : (lj == 1 ? b : (lj == 2 ? c : 0.f)); } \
        { const float a = GVF_QB(gA.w, k_), b = GVF_QB(gB.w, k_), c = GVF_QB(gC.w, k_); o4.w = lj == 0 ? a : (lj == 1 ? b : (lj == 2 ? c : 0.f)); } \
        if (tk != 0) qbase[4 * (k_) + lj] = o4;                                                             \
    }
    GVF_QSTORE(0) GVF_QSTORE(1) GVF_QSTORE(2) GVF_QSTORE(3)
#undef GVF_QSTORE
#undef GVF_QB

    // block sum of tiles_touched (feeds the instance-offset scan, R2; radix binning only)
    if (!WAVE_FRAMES && block_sums != nullptr) {
        const unsigned lane = t & 63, w = t >> 6;
        uint32_t incl = gvf_wave_incl_scan(touched, lane);
        __shared__ uint32_t wsum[PRE_THREADS / GVF_WAVE];
        __syncthreads();
        if (lane == 63) wsum[w] = incl;
        __syncthreads();
        if (t == 0) block_sums[(size_t)f * nbx + bx] = wsum[0] + wsum[1] + wsum[2] + wsum[3];
    }
  }
}

// ---------------------------------------------------------------------------------------------
// R2: exclusive scan of the F*nb block sums (single workgroup), per-frame counts and grand total
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(1024) void scan_sums_kernel(uint32_t* __restrict__ block_sums, int nb, int F,
                                                         uint32_t* __restrict__ frame_base /*[F+1]*/,
                                                         uint32_t* __restrict__ num_rendered /*[F]*/,
                                                         uint32_t* __restrict__ total_out, uint32_t max_rendered) {
    __shared__ uint32_t wsum[16];
    __shared__ uint32_t carry_s;
    const int t = threadIdx.x;
    const unsigned lane = t & 63, w = t >> 6;
    const int n = nb * F;
    if (t == 0) carry_s = 0;
    __syncthreads();
    for (int base = 0; base < n; base += 1024) {
        int j = base + t;
        uint32_t v = j < n ? block_sums[j] : 0u;
        uint32_t incl = gvf_wave_incl_scan(v, lane);
        if (lane == 63) wsum[w] = incl;
        __syncthreads();
        uint32_t wbase = 0, tot = 0;
        for (unsigned k = 0; k < 16; ++k) { if (k < w) wbase += wsum[k]; tot += wsum[k]; }
        uint32_t carry = carry_s;
        uint32_t excl = carry + wbase + incl - v;
        if (j < n) {
            block_sums[j] = excl;
            if (j % nb == 0) frame_base[j / nb] = excl;
        }
        __syncthreads();
        if (t == 0) carry_s = carry + tot;
        __syncthreads();
    }
    // Overflow (D > workspace capacity): render nothing (n = 0) but still report the true counts, so
    // the caller can detect it from num_rendered and retry with a larger workspace.
    if (t == 0) { frame_base[F] = carry_s; *total_out = carry_s > max_rendered ? 0u : carry_s; }
    __syncthreads();
    for (int f = t; f < F; f += 1024) num_rendered[f] = frame_base[f + 1] - frame_base[f];
}

// ---------------------------------------------------------------------------------------------
// R3: duplicate with keys
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(PRE_THREADS) void duplicate_kernel(
    int P, int gx, int gy, const float4* __restrict__ splats,
    const uint32_t* __restrict__ tiles_touched, const int32_t* __restrict__ radii_ws,
    const uint32_t* __restrict__ block_base, uint64_t* __restrict__ keys, uint32_t* __restrict__ vals,
    uint32_t max_rendered, int upstream_binning) {
    __shared__ uint32_t wsum[PRE_THREADS / GVF_WAVE];
    const int t = threadIdx.x, f = blockIdx.y;
    const int i = blockIdx.x * PRE_THREADS + t;
    const unsigned lane = t & 63, w = t >> 6;
    const size_t o = (size_t)f * P + i;
    uint32_t touched = i < P ? tiles_touched[o] : 0u;
    uint32_t incl = gvf_wave_incl_scan(touched, lane);
    if (lane == 63) wsum[w] = incl;
    __syncthreads();
    uint32_t wbase = 0;
    for (unsigned k = 0; k < w; ++k) wbase += wsum[k];
    uint32_t off = block_base[(size_t)f * gridDim.x + blockIdx.x] + wbase + incl - touched;
    if (touched == 0) return;
    if ((uint64_t)off + touched > (uint64_t)max_rendered) return;  // overflow: caller checks num_rendered
    const float4 a = splats[4 * o];
    const float4 c = splats[4 * o + 2];
    const float depth = c.y;
    TileRect r = get_rect(a.x, a.y, (float)radii_ws[o], gx, gy);
    if (!upstream_binning) r = tight_rect(r, a.x, a.y, c.z, c.w, gx, gy);
    const uint64_t tile0 = (uint64_t)f * (uint32_t)(gx * gy);
    const uint32_t dbits = __float_as_uint(depth);
    for (int y = r.y0; y < r.y1; ++y)
        for (int x = r.x0; x < r.x1; ++x) {
            uint64_t key = ((tile0 + (uint32_t)(y * gx + x)) << 32) | dbits;
            keys[off] = key;
            vals[off] = (uint32_t)i;
            ++off;
        }
}

// ---------------------------------------------------------------------------------------------
// R2-R5, bucket form: per-tile counts (preprocess) -> exclusive scan = tile ranges -> scatter into the tile segments.
// No global sort: the order inside a segment is whatever the atomics produced, the per-tile sort below keys on
// (depth, id) and makes it deterministic.
// ---------------------------------------------------------------------------------------------
// order-preserving float <-> uint32 map (atomicMin / atomicMax on floats of either sign)
__device__ __forceinline__ uint32_t float_ordered(float f) {
    const uint32_t u = __float_as_uint(f);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float float_unordered(uint32_t o) {
    return __uint_as_float((o & 0x80000000u) ? (o & 0x7fffffffu) : ~o);
}

// Exclusive scan of the per-segment counters (segment = (frame, tile); F * tiles of them) in two
// launches: block sums of 4096 counters, then every block adds up the sums in front of it (at most a few hundred
// values) and rescans its own chunk.  Writes segment ranges + cursors, per-frame D, the grand total.
__global__ __launch_bounds__(1024) void seg_sums_kernel(const uint32_t* __restrict__ cnt, int n, uint32_t* __restrict__ partial) {
    __shared__ uint32_t wsum[16];
    const int t = threadIdx.x, j0 = blockIdx.x * SCAN_CHUNK + 4 * t;
    uint32_t s = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) s += j0 + k < n ? cnt[j0 + k] : 0u;
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) s += __shfl_xor(s, d, 64);
    if ((t & 63) == 0) wsum[t >> 6] = s;
    __syncthreads();
    if (t == 0) { uint32_t tot = 0; for (int k = 0; k < 16; ++k) tot += wsum[k]; partial[blockIdx.x] = tot; }
}

__global__ __launch_bounds__(1024) void seg_scan_kernel(const uint32_t* __restrict__ cnt, int n, int ntiles, int F,
                                                        const uint32_t* __restrict__ partial, int nblocks,
                                                        uint2* __restrict__ ranges, uint32_t* __restrict__ cursor,
                                                        uint32_t* __restrict__ frame_base /*[F+1]*/,
                                                        uint32_t* __restrict__ num_rendered /*[F]*/,
                                                        uint32_t* __restrict__ total_out, uint32_t max_rendered,
                                                        uint32_t* __restrict__ cls /* sort size classes, as classify_kernel */) {
    __shared__ uint32_t wsum[16], wtot[16];
    __shared__ uint32_t s_base, s_total;
    const int t = threadIdx.x;
    const unsigned lane = t & 63, w = t >> 6;
    // offset of this chunk and the grand total from the block sums
    uint32_t before = 0, all = 0;
    for (int k = t; k < nblocks; k += 1024) { const uint32_t p = partial[k]; all += p; if (k < (int)blockIdx.x) before += p; }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) { before += __shfl_xor(before, d, 64); all += __shfl_xor(all, d, 64); }
    if (lane == 0) { wsum[w] = before; wtot[w] = all; }
    __syncthreads();
    if (t == 0) {
        uint32_t b = 0, a = 0;
        for (int k = 0; k < 16; ++k) { b += wsum[k]; a += wtot[k]; }
        s_base = b; s_total = a;
    }
    __syncthreads();
    const uint32_t total = s_total;
    const bool overflow = total > max_rendered;
    const int j0 = blockIdx.x * SCAN_CHUNK + 4 * t;
    uint32_t c[4], s = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) { c[k] = j0 + k < n ? cnt[j0 + k] : 0u; s += c[k]; }
    const uint32_t incl = gvf_wave_incl_scan(s, lane);
    __syncthreads();
    if (lane == 63) wsum[w] = incl;
    __syncthreads();
    uint32_t run = s_base + incl - s;
    for (unsigned k = 0; k < w; ++k) run += wsum[k];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int j = j0 + k;
        if (j < n) {
            // Overflow (D > workspace capacity): render nothing, but the true counts let the caller retry.
            ranges[j] = overflow ? make_uint2(0u, 0u) : make_uint2(run, run + c[k]);
            cursor[j] = run;
            if (!overflow && c[k] > (uint32_t)SORT_SMALL_N) {           // rare: a segment for the LDS / global sort classes
                if (c[k] > (uint32_t)SORT_LARGE_N) cls[2 + n + atomicAdd(&cls[1], 1u)] = (uint32_t)j;
                else cls[2 + atomicAdd(&cls[0], 1u)] = (uint32_t)j | (c[k] > (uint32_t)SORT_MEDIUM_N ? 0x80000000u : 0u);   // top bit: the upper half of the LDS class
            }
            if (j % ntiles == 0) frame_base[j / ntiles] = run;
        }
        run += c[k];
    }
    if (blockIdx.x == 0 && t == 0) { frame_base[F] = total; *total_out = overflow ? 0u : total; }
}

// per-frame instance counts from the frame bases (separate tiny launch: needs every block of seg_scan_kernel done)
__global__ void frame_counts_kernel(const uint32_t* __restrict__ frame_base, int F, uint32_t* __restrict__ num_rendered) {
    const int f = blockIdx.x * blockDim.x + threadIdx.x;
    if (f < F) num_rendered[f] = frame_base[f + 1] - frame_base[f];
}

// Count / scatter passes over the compact bin records, BIN_SPT slots per thread, slots taken in Morton order
// (`order` = the Gaussian of each slot, may be null = identity): the rects of one block then fall into a small window of tiles, instances are
// counted in an LDS table and every touched tile costs ONE global atomic per block (count pass: += tile_count;
// scatter pass: cursor allocation, the base is left in the table and an LDS counter hands out the slots).  A block
// whose window exceeds WIN_MAX tiles (incoherent order) pays one global atomic per instance instead.
// rec_by_id = 0: the records sit at their slots (preprocess_kernel's bin_slot) and are read as one stream; 1: they sit at the Gaussian's index
// and are gathered, and xcd_frames = 1 then lays the grid out 1-D so that each XCD takes whole frames (see the host).  REC: the record form.
constexpr int WIN_MAX = 2048;

template <bool SCATTER, typename REC>
__global__ __launch_bounds__(PRE_THREADS) void bin_kernel(int P, int gx, int gy, const REC* __restrict__ binrec,
                                                          const uint32_t* __restrict__ order,
                                                          uint32_t* __restrict__ tile_count /* count pass */,
                                                          uint32_t* __restrict__ cursor /* scatter pass */,
                                                          const uint32_t* __restrict__ total,
                                                          uint64_t* __restrict__ payload,
                                                          const uint32_t* __restrict__ frame_base, uint32_t* __restrict__ num_rendered,
                                                          int rec_by_id, int xcd_frames, int F) {
    __shared__ uint32_t s_tab[WIN_MAX];
    __shared__ uint32_t s_run[SCATTER ? WIN_MAX : 1];
    __shared__ int s_box[4];
    int blk = (int)blockIdx.x, f = (int)blockIdx.y;
    if (xcd_frames) {
        // frame 8 g + n % 8 of frame group g, block (n / 8) % nblk of it: every (frame, block) exactly once.  A performance heuristic, measured
        // (scatter pass 95 us with it at the bench shape), not derived: it assumes the dispatcher hands workgroup n to XCD n % 8, so that one
        // XCD gathers a frame's records from its own L2; another dispatch order costs only speed.
        const int nblk = (P + BIN_SLOTS - 1) / BIN_SLOTS, k = (int)(blockIdx.x >> 3);
        f = (k / nblk) * 8 + (int)(blockIdx.x & 7u);
        blk = k - (k / nblk) * nblk;
        if (f >= F) return;                          // the grid is rounded up to whole groups of 8 frames (workgroup-uniform)
    }
    // scatter pass: the per-frame instance counts from the frame bases the scan left (saves a launch of its own)
    if (SCATTER && num_rendered != nullptr && blk == 0 && threadIdx.x == 0)
        num_rendered[f] = frame_base[f + 1] - frame_base[f];
    if (SCATTER && *total == 0u) return;            // nothing visible, or capacity overflow (uniform)
    const int t = threadIdx.x, lane = t & 63;
    if (t == 0) { s_box[0] = 0x7fffffff; s_box[1] = 0x7fffffff; s_box[2] = 0; s_box[3] = 0; }
    int x0[BIN_SPT], y0[BIN_SPT], x1[BIN_SPT], y1[BIN_SPT];
    uint64_t key[BIN_SPT];
    int bx0 = 0x7fffffff, by0 = 0x7fffffff, bx1 = 0, by1 = 0;
#pragma unroll
    for (int k = 0; k < BIN_SPT; ++k) {
        const int s = blk * BIN_SLOTS + k * PRE_THREADS + t;
        x0[k] = y0[k] = x1[k] = y1[k] = 0; key[k] = 0;
        if (s < P) {
            const uint32_t id = order != nullptr ? order[s] : (uint32_t)s;
            const REC br = binrec[(size_t)f * P + (rec_by_id ? id : (uint32_t)s)];
            const TileRect r = binrec_rect(br);
            x0[k] = r.x0; y0[k] = r.y0; x1[k] = r.x1; y1[k] = r.y1;
            key[k] = ((uint64_t)binrec_depth(br) << 32) | id;          // depth bits above the Gaussian id
            if (x1[k] > x0[k] && y1[k] > y0[k]) {
                bx0 = min(bx0, x0[k]); by0 = min(by0, y0[k]); bx1 = max(bx1, x1[k]); by1 = max(by1, y1[k]);
            } else {
                x1[k] = x0[k];                                          // empty: the loops below do nothing
            }
        }
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        bx0 = min(bx0, __shfl_xor(bx0, d, 64)); by0 = min(by0, __shfl_xor(by0, d, 64));
        bx1 = max(bx1, __shfl_xor(bx1, d, 64)); by1 = max(by1, __shfl_xor(by1, d, 64));
    }
    __syncthreads();                                 // s_box initialised
    if (lane == 0 && bx1 > bx0) {
        atomicMin(&s_box[0], bx0); atomicMin(&s_box[1], by0); atomicMax(&s_box[2], bx1); atomicMax(&s_box[3], by1);
    }
    __syncthreads();
    const int wx0 = s_box[0], wy0 = s_box[1], ww = s_box[2] - s_box[0], wh = s_box[3] - s_box[1];
    if (ww <= 0 || wh <= 0) return;                  // no instance in this block (uniform)
    uint32_t* gtab = (SCATTER ? cursor : tile_count) + (size_t)f * gx * gy;
    if (ww * wh <= WIN_MAX) {
        const int area = ww * wh;
        for (int e = t; e < area; e += PRE_THREADS) { s_tab[e] = 0u; if (SCATTER) s_run[e] = 0u; }
        __syncthreads();
#pragma unroll
        for (int k = 0; k < BIN_SPT; ++k)
            for (int y = y0[k]; y < y1[k]; ++y)
                for (int x = x0[k]; x < x1[k]; ++x) atomicAdd(&s_tab[(y - wy0) * ww + (x - wx0)], 1u);
        __syncthreads();
        for (int e = t; e < area; e += PRE_THREADS) {
            const uint32_t c = s_tab[e];
            if (c != 0u) {
                const int seg = (wy0 + e / ww) * gx + wx0 + e % ww;
                if (SCATTER) s_tab[e] = atomicAdd(&gtab[seg], c);
                else atomicAdd(&gtab[seg], c);
            }
        }
        if (SCATTER) {
            __syncthreads();
#pragma unroll
            for (int k = 0; k < BIN_SPT; ++k)
                for (int y = y0[k]; y < y1[k]; ++y)
                    for (int x = x0[k]; x < x1[k]; ++x) {
                        const int e = (y - wy0) * ww + (x - wx0);
                        payload[s_tab[e] + atomicAdd(&s_run[e], 1u)] = key[k];
                    }
        }
    } else {
#pragma unroll
        for (int k = 0; k < BIN_SPT; ++k)
            for (int y = y0[k]; y < y1[k]; ++y)
                for (int x = x0[k]; x < x1[k]; ++x) {
                    const uint32_t pos = atomicAdd(&gtab[y * gx + x], 1u);
                    if (SCATTER) payload[pos] = key[k];
                }
    }
}

// Count pass in index order: a workgroup takes BINX_PER_WG consecutive Gaussians of one frame, whose bin records preprocess_kernel<false>
// stored at their own index, and counts their instances in a whole-frame LDS table of tiles, so that every touched tile
// costs ONE global atomic per workgroup however the Gaussians are ordered in space.  The host takes this path only when the frame's tiles
// fit the table (ntiles <= BINX_TAB).  cursor, total, payload, frame_base and num_rendered are read by no code; they keep the
// kernel's arguments as they were when it also had a scatter form.
constexpr int BINX_THREADS = 512;
constexpr int BINX_SPT = 4;                          // 16-byte loads in flight per thread

// the instances of one rect into the workgroup's tile table
__device__ __forceinline__ void binx_count(uint32_t* s_tab, int gx, TileRect r) {
    for (int y = r.y0; y < r.y1; ++y)
        for (int x = r.x0; x < r.x1; ++x) atomicAdd(&s_tab[y * gx + x], 1u);
}

// REC: the record form.  Either form keeps BINX_SPT 16-byte loads in flight per thread; a load brings one 16-byte record or two 8-byte
// ones.  The pairs of the 8-byte form are taken at even positions of the whole [F*P] array (frame f starts at record f P, which may be
// odd), so every load is 16-byte aligned; a pair's record outside the workgroup's own range [a0, a1) is dropped.  The last pair of the
// array may reach one record past F P: the array has room for 16 bytes per record (carve).
template <typename REC>
__global__ __launch_bounds__(BINX_THREADS) void bin_index_kernel(int P, int gx, const REC* __restrict__ binrec,
                                                                 uint32_t* __restrict__ tile_count,
                                                                 uint32_t* __restrict__ cursor,
                                                                 const uint32_t* __restrict__ total,
                                                                 uint64_t* __restrict__ payload, int ntiles,
                                                                 const uint32_t* __restrict__ frame_base, uint32_t* __restrict__ num_rendered) {
    __shared__ uint32_t s_tab[BINX_TAB];
    const int t = threadIdx.x, f = blockIdx.y;
    const int g0 = (int)blockIdx.x * BINX_PER_WG, g1 = min(P, g0 + BINX_PER_WG);
    for (int e = t; e < ntiles; e += BINX_THREADS) s_tab[e] = 0u;
    __syncthreads();
    if constexpr (sizeof(REC) == 16) {
        const uint4* rec = binrec + (size_t)f * P;
        for (int base = g0; base < g1; base += BINX_SPT * BINX_THREADS) {
            uint4 br[BINX_SPT];
#pragma unroll
            for (int k = 0; k < BINX_SPT; ++k) {
                const int s = base + k * BINX_THREADS + t;
                br[k] = s < g1 ? rec[s] : make_uint4(0u, 0u, 0u, 0u);     // {0, 0, 0, 0}: an empty rect
            }
#pragma unroll
            for (int k = 0; k < BINX_SPT; ++k) binx_count(s_tab, gx, binrec_rect16(br[k].x, br[k].y));
        }
    } else {
        const size_t a0 = (size_t)f * P + g0, a1 = (size_t)f * P + g1;   // this workgroup's records, as positions in the whole array
        const uint4* pairs = reinterpret_cast<const uint4*>(binrec);       // pair j = records 2 j, 2 j + 1
        for (size_t jbase = a0 >> 1; 2 * jbase < a1; jbase += BINX_SPT * BINX_THREADS) {
            uint4 br[BINX_SPT];
#pragma unroll
            for (int k = 0; k < BINX_SPT; ++k) {
                const size_t j = jbase + k * BINX_THREADS + t;
                br[k] = 2 * j < a1 ? pairs[j] : make_uint4(0u, 0u, 0u, 0u);
            }
#pragma unroll
            for (int k = 0; k < BINX_SPT; ++k) {
                const size_t a = 2 * (jbase + k * BINX_THREADS + t);
                binx_count(s_tab, gx, binrec_rect8(a >= a0 ? br[k].x : 0u));       // (a < a1, or the pair is zero)
                binx_count(s_tab, gx, binrec_rect8(a + 1 < a1 ? br[k].z : 0u));    // (a + 1 >= a0 always)
            }
        }
    }
    __syncthreads();
    uint32_t* gtab = tile_count + (size_t)f * ntiles;
    for (int e = t; e < ntiles; e += BINX_THREADS) {
        const uint32_t c = s_tab[e];
        if (c != 0u) atomicAdd(&gtab[e], c);
    }
}

// ---------------------------------------------------------------------------------------------
// Spatial order of the Gaussians (once per call, shared by all frames): 15-bit Morton code of the position inside
// the bounding box, counting-sorted.  Purely a locality device for the bin passes: any order gives the same image.
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void bbox_kernel(int P, const float* __restrict__ xyz, uint32_t* __restrict__ mm) {
    __shared__ uint32_t s_mm[6];
    if (threadIdx.x < 6) s_mm[threadIdx.x] = threadIdx.x < 3 ? 0xffffffffu : 0u;
    __syncthreads();
    uint32_t lo[3] = {0xffffffffu, 0xffffffffu, 0xffffffffu}, hi[3] = {0u, 0u, 0u};
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < P; i += gridDim.x * blockDim.x) {
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const float v = xyz[3 * (size_t)i + k];
            if (v == v && fabsf(v) < 3.0e38f) {
                const uint32_t o = float_ordered(v);
                lo[k] = min(lo[k], o); hi[k] = max(hi[k], o);
            }
        }
    }
#pragma unroll
    for (int k = 0; k < 3; ++k) {
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) {
            lo[k] = min(lo[k], (uint32_t)__shfl_xor((int)lo[k], d, 64));
            hi[k] = max(hi[k], (uint32_t)__shfl_xor((int)hi[k], d, 64));
        }
        if ((threadIdx.x & 63) == 0) { atomicMin(&s_mm[k], lo[k]); atomicMax(&s_mm[3 + k], hi[k]); }
    }
    __syncthreads();
    if (threadIdx.x < 3) atomicMin(&mm[threadIdx.x], s_mm[threadIdx.x]);
    else if (threadIdx.x < 6) atomicMax(&mm[threadIdx.x], s_mm[threadIdx.x]);
}

__device__ __forceinline__ uint32_t spread5(uint32_t v) {   // 5 bits -> every third bit
    return (v & 1u) | ((v & 2u) << 2) | ((v & 4u) << 4) | ((v & 8u) << 6) | ((v & 16u) << 8);
}


__device__ __forceinline__ uint32_t morton15(int i, const float* __restrict__ xyz, const uint32_t* __restrict__ mm) {
    uint32_t code = 0;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const float lo = float_unordered(mm[k]), hi = float_unordered(mm[3 + k]);
        const float v = xyz[3 * (size_t)i + k];
        float q = (v - lo) / fmaxf(hi - lo, 1e-30f) * 32.0f;
        q = (q == q) ? fminf(fmaxf(q, 0.0f), 31.0f) : 0.0f;
        code |= spread5((uint32_t)q) << k;
    }
    return code;
}

// counting sort by Morton cell: histogram -> exclusive scan -> scatter (order inside a cell is arbitrary)
__global__ __launch_bounds__(256) void morton_count_kernel(int P, const float* __restrict__ xyz,
                                                           const uint32_t* __restrict__ mm, uint32_t* __restrict__ codes,
                                                           uint32_t* __restrict__ hist) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= P) return;
    const uint32_t c = morton15(i, xyz, mm);
    codes[i] = c;
    atomicAdd(&hist[c], 1u);
}

__global__ __launch_bounds__(1024) void morton_scan_kernel(uint32_t* __restrict__ hist) {
    __shared__ uint32_t wsum[16];
    const int t = threadIdx.x;
    const unsigned lane = t & 63, w = t >> 6;
    constexpr int PER = MORTON_BINS / 1024;
    uint32_t v[PER], s = 0;
#pragma unroll
    for (int k = 0; k < PER; ++k) { v[k] = hist[t * PER + k]; s += v[k]; }
    const uint32_t incl = gvf_wave_incl_scan(s, lane);
    if (lane == 63) wsum[w] = incl;
    __syncthreads();
    uint32_t run = incl - s;
    for (unsigned k = 0; k < w; ++k) run += wsum[k];
#pragma unroll
    for (int k = 0; k < PER; ++k) { hist[t * PER + k] = run; run += v[k]; }
}

// codes_rank: in = the Gaussian's Morton code, out = its slot in the order (the inverse permutation: the shared-activation launch writes
// the bin records at their slots, so the bin passes read them as one contiguous stream)
__global__ __launch_bounds__(256) void morton_scatter_kernel(int P, uint32_t* codes_rank, uint32_t* __restrict__ hist,
                                                             uint32_t* __restrict__ order) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= P) return;
    const uint32_t slot = atomicAdd(&hist[codes_rank[i]], 1u);
    order[slot] = (uint32_t)i;
    codes_rank[i] = slot;
}

// ---------------------------------------------------------------------------------------------
// R5: tile ranges
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void ranges_kernel(const uint64_t* __restrict__ keys,
                                                     const uint32_t* __restrict__ n_ptr, uint32_t n_cap,
                                                     uint2* __restrict__ ranges, uint32_t n_ranges) {
    uint32_t n = *n_ptr;
    n = n < n_cap ? n : n_cap;
    for (uint32_t k = blockIdx.x * blockDim.x + threadIdx.x; k < n; k += gridDim.x * blockDim.x) {
        uint32_t cur = (uint32_t)(keys[k] >> 32);
        if (cur >= n_ranges) continue;
        if (k == 0) ranges[cur].x = 0;
        else {
            uint32_t prev = (uint32_t)(keys[k - 1] >> 32);
            if (cur != prev) { if (prev < n_ranges) ranges[prev].y = k; ranges[cur].x = k; }
        }
        if (k == n - 1) ranges[cur].y = n;
    }
}

// Camera blocks travel as kernel arguments (16 per launch): no host buffer has to outlive the call
// and the upload is capturable in a hipGraph.
struct FrameChunk { GvfRastFrame f[16]; };
// The first upload launch of a call also clears the call's tables (one launch instead of six memsets, each a ~4 us bubble in a
// 1.5 ms step): blocks >= 1 zero the tile ranges, the tile counters, the Morton histogram and the sort-class counters, and
// set the bounding-box accumulators (min slots to all-ones, max slots to zero).
struct CallTables {
    uint32_t* ranges; uint32_t n_ranges;             // words
    uint32_t* tile_count; uint32_t n_tile_count;
    uint32_t* mhist; uint32_t n_mhist;
    uint32_t* cls;                                    // 2 words
    uint32_t* mm;                                     // 6 words + the layout word mm[LAYOUT_WORD]
    uint32_t layout;                                  // LAYOUT_* of this call, for the backward (gvf_rast_backward*)
};
__global__ void upload_frames_kernel(FrameChunk c, int count, GvfRastFrame* __restrict__ dst, CallTables tab) {
    if (blockIdx.x == 0) {
        const int words = (int)(sizeof(GvfRastFrame) / 4) * count;
        const uint32_t* src = reinterpret_cast<const uint32_t*>(&c);
        for (int k = threadIdx.x; k < words; k += blockDim.x) reinterpret_cast<uint32_t*>(dst)[k] = src[k];
        if (tab.cls != nullptr && threadIdx.x < 2) tab.cls[threadIdx.x] = 0u;
        if (tab.mm != nullptr && threadIdx.x < 6) tab.mm[threadIdx.x] = threadIdx.x < 3 ? 0xffffffffu : 0u;
        if (tab.mm != nullptr && threadIdx.x == LAYOUT_WORD) tab.mm[LAYOUT_WORD] = tab.layout;
        return;
    }
    const uint32_t t = (blockIdx.x - 1) * blockDim.x + threadIdx.x, nt = (gridDim.x - 1) * blockDim.x;
    for (uint32_t k = t; k < tab.n_ranges; k += nt) tab.ranges[k] = 0u;
    for (uint32_t k = t; k < tab.n_tile_count; k += nt) tab.tile_count[k] = 0u;
    for (uint32_t k = t; k < tab.n_mhist; k += nt) tab.mhist[k] = 0u;
}

// ---------------------------------------------------------------------------------------------
// host side: the launches of a call, from its plan
// ---------------------------------------------------------------------------------------------
PreParams pre_params(const RastCall& c, const RastPlan& plan) {
    const GvfRastSettings& st = *c.st;
    PreParams pp;
    pp.P = c.P; pp.M = c.colors_precomp ? 0 : c.M; pp.deg = st.sh_degree; pp.H = st.image_height; pp.W = st.image_width; pp.mode = st.mode;
    pp.gx = plan.gx; pp.gy = plan.gy; pp.kernel_size = st.kernel_size; pp.scale_modifier = st.scale_modifier;
    pp.fused = c.fused ? 1 : 0; pp.n_delta = c.n_delta; pp.F = c.F;
    pp.upstream_binning = plan.upstream_binning;
    if (c.fused) pp.act = *c.act; else pp.act = GvfGaussianActivation{};
    pp.delta_lds = 0;
    return pp;
}

// The pointers of a preprocess launch by name: a call site sets what it passes, the rest stays null.  The frames and the splat records are
// the workspace's in every launch.
struct PreArgs {
    const float *a0 = nullptr, *a1 = nullptr, *a2 = nullptr, *a3 = nullptr;   // activated or raw inputs; SHARED: a0 = the stage-A records, a1 = slot -> Gaussian
    const float *sh = nullptr, *colors_precomp = nullptr, *cov3D_precomp = nullptr, *delta = nullptr;
    uint32_t* tiles_touched = nullptr;   // radix binning
    int32_t* radii = nullptr;
    uint32_t* block_sums = nullptr;      // radix binning
    uint4* binrec = nullptr;             // bucket binning
    const uint32_t* bin_slot = nullptr;  // Gaussian -> position of its bin record inside a frame; null = identity
};
template <bool SHARED, bool WAVE_FRAMES = false>
void launch_preprocess(hipStream_t stream, const RastPlan& plan, const PreParams& pp, const Workspace& w, const PreArgs& a) {
    const int32_t* g = WAVE_FRAMES ? plan.wf_grid : plan.pre_grid;
    const size_t lds = (size_t)(WAVE_FRAMES ? plan.wf_lds_bytes : plan.pre_lds_bytes);
    if (plan.rec8)
        hipLaunchKernelGGL((preprocess_kernel<SHARED, WAVE_FRAMES, BinRec8>), dim3(g[0], g[1]), dim3(PRE_THREADS), lds, stream, pp, w.frames,
                           a.a0, a.a1, a.a2, a.a3, a.sh, a.colors_precomp, a.cov3D_precomp, a.delta, w.splats, a.tiles_touched, a.radii,
                           a.block_sums, reinterpret_cast<BinRec8*>(a.binrec), a.bin_slot);
    else
        hipLaunchKernelGGL((preprocess_kernel<SHARED, WAVE_FRAMES, BinRec16>), dim3(g[0], g[1]), dim3(PRE_THREADS), lds, stream, pp, w.frames,
                           a.a0, a.a1, a.a2, a.a3, a.sh, a.colors_precomp, a.cov3D_precomp, a.delta, w.splats, a.tiles_touched, a.radii,
                           a.block_sums, a.binrec, a.bin_slot);
}

// The count pass (index order, or bin_kernel<false> over the Morton slots) and the scatter pass over records of form REC
template <typename REC>
void launch_bin_count(hipStream_t stream, const RastCall& c, const RastPlan& plan, const Workspace& w, const uint32_t* order) {
    const REC* rec = reinterpret_cast<const REC*>(w.binrec);
    const int gather = plan.rec_gather ? 1 : 0;
    if (plan.index_count)
        hipLaunchKernelGGL((bin_index_kernel<REC>), dim3(plan.binx_grid[0], plan.binx_grid[1]), dim3(BINX_THREADS), 0, stream, c.P, plan.gx, rec,
                           w.tile_count, w.cursor, w.total, w.keys, plan.ntiles, nullptr, nullptr);
    else
        hipLaunchKernelGGL((bin_kernel<false, REC>), dim3(plan.bin_grid[0], plan.bin_grid[1]), dim3(PRE_THREADS), 0, stream, c.P, plan.gx, plan.gy,
                           rec, order, w.tile_count, w.cursor, w.total, w.keys, nullptr, nullptr, gather, gather, c.F);
}
template <typename REC>
void launch_bin_scatter(hipStream_t stream, const RastCall& c, const RastPlan& plan, const Workspace& w, const uint32_t* order) {
    const int gather = plan.rec_gather ? 1 : 0;
    hipLaunchKernelGGL((bin_kernel<true, REC>), dim3(plan.bin_grid[0], plan.bin_grid[1]), dim3(PRE_THREADS), 0, stream, c.P, plan.gx, plan.gy,
                       reinterpret_cast<const REC*>(w.binrec), order, w.tile_count, w.cursor, w.total, w.keys, w.frame_base,
                       c.out_num_rendered, gather, gather, c.F);
}

// The call's own inputs, as both fused launches (wave-frames or not) and the radix path read them
PreArgs input_args(const RastCall& c) {
    PreArgs a;
    a.a0 = c.a0; a.a1 = c.a1; a.a2 = c.a2; a.a3 = c.a3;
    a.sh = c.colors_precomp ? nullptr : c.sh; a.colors_precomp = c.colors_precomp; a.cov3D_precomp = c.cov3D_precomp; a.delta = c.delta;
    return a;
}

// Morton order of the Gaussians into w.order (slot -> Gaussian) and w.order_alt (Gaussian -> slot); the bounding box accumulators and the
// histogram were cleared by the upload launch
void launch_morton_order(hipStream_t stream, const RastCall& c, const Workspace& w) {
    int bb = (c.P + 255) / 256; if (bb > 128) bb = 128;
    const int pb = (c.P + 255) / 256;
    hipLaunchKernelGGL(bbox_kernel, dim3(bb), dim3(256), 0, stream, c.P, c.a0, w.mm);
    hipLaunchKernelGGL(morton_count_kernel, dim3(pb), dim3(256), 0, stream, c.P, c.a0, w.mm, w.order_alt, w.mhist);
    hipLaunchKernelGGL(morton_scan_kernel, dim3(1), dim3(1024), 0, stream, w.mhist);
    hipLaunchKernelGGL(morton_scatter_kernel, dim3(pb), dim3(256), 0, stream, c.P, w.order_alt, w.mhist, w.order);
}

// Shared activation: stage A once per (slice, Gaussian) into keys_alt (which only the radix binning uses), then the per-frame launch over
// the records.  `order`: the Morton order (w.order) or null.
void launch_shared_preprocess(hipStream_t stream, const RastCall& c, const RastPlan& plan, const PreParams& pp, const Workspace& w,
                              const uint32_t* order) {
    const int P = c.P;
    ActSlices slices;
    slices.n = plan.n_slices;
    for (int k = 0; k < plan.n_slices; ++k) slices.di[k] = plan.di[k];
    float4* rec3d = reinterpret_cast<float4*>(w.keys_alt);
    float* sh_by_slot = plan.slot_mode ? reinterpret_cast<float*>(rec3d + 4 * (size_t)plan.n_slices * (size_t)P) : nullptr;
    hipLaunchKernelGGL(activate_cov_kernel, dim3((P + 255) / 256, plan.n_slices), dim3(256), 0, stream, *c.act, c.st->scale_modifier, P, slices,
                       c.a0, c.a1, c.a2, c.a3, c.delta, rec3d, plan.slot_mode ? w.order_alt : nullptr, c.sh, pp.M * 3, sh_by_slot);
    PreArgs a;
    a.a0 = reinterpret_cast<const float*>(rec3d);
    a.radii = c.out_radii == nullptr ? nullptr : w.radii;
    a.binrec = w.binrec;
    if (plan.slot_mode) {
        // thread i = slot i: records, SH rows, splat records and bin records are all read / written at i; the sorted lists keep Gaussian
        // ids (ties break by index, as upstream's stable sort does) and the blend looks the record index up (rec_of = w.order_alt)
        a.a1 = reinterpret_cast<const float*>(order);
        a.sh = sh_by_slot;
    } else {
        a.sh = c.colors_precomp ? nullptr : c.sh;
        a.colors_precomp = c.colors_precomp;
        a.bin_slot = order != nullptr ? w.order_alt : nullptr;
    }
    launch_preprocess<true>(stream, plan, pp, w, a);
}

int key_end_bit(int F, int ntiles) {
    uint64_t m = (uint64_t)F * (uint64_t)ntiles;
    int bits = 0;
    while (((uint64_t)1 << bits) < m) ++bits;
    return 32 + bits;
}

}  // namespace

int gvf_rast::upload_frames(hipStream_t stream, const RastCall& c, const RastPlan& plan, const Workspace& w) {
    for (int f0 = 0; f0 < c.F; f0 += 16) {
        FrameChunk ch;
        const int cnt = c.F - f0 < 16 ? c.F - f0 : 16;
        for (int k = 0; k < cnt; ++k) {
            ch.f[k] = c.frames_host[f0 + k];
            ch.f[k].reserved[0] = plan.frame_slice[(size_t)(f0 + k)];       // the device copy's slice index (the caller's block is not touched)
        }
        CallTables tab = {};
        if (f0 == 0) {
            tab.ranges = reinterpret_cast<uint32_t*>(w.ranges); tab.n_ranges = 2u * (uint32_t)plan.nseg;
            tab.tile_count = w.tile_count; tab.n_tile_count = (uint32_t)plan.nseg;
            tab.mhist = w.mhist; tab.n_mhist = plan.morton ? (uint32_t)MORTON_BINS : 0u;
            tab.cls = w.cls; tab.mm = w.mm; tab.layout = (uint32_t)plan.layout;
        }
        hipLaunchKernelGGL(upload_frames_kernel, dim3(1 + (f0 == 0 ? plan.clear_blocks : 0)), dim3(256), 0, stream, ch, cnt, w.frames + f0, tab);
    }
    GVF_CHECK_LAUNCH();
    return GVF_OK;
}

// Bucket binning: [Morton order] -> preprocess -> count pass -> segment scan -> scatter pass.  Leaves (depth bits << 32 | id) keys in the
// tile segments of w.keys, in arbitrary order inside a segment.
int gvf_rast::front_end_bucket(hipStream_t stream, const RastCall& c, const RastPlan& plan, const Workspace& w, const hipEvent_t* marks) {
    const int P = c.P, F = c.F;
    prof_mark(stream, marks, 0);
    const uint32_t* order = nullptr;
    if (plan.morton) {
        launch_morton_order(stream, c, w);
        order = w.order;
        GVF_CHECK_LAUNCH();
    }
    prof_mark(stream, marks, 1);
    const PreParams pp = pre_params(c, plan);
    if (plan.shared) {
        launch_shared_preprocess(stream, c, plan, pp, w, order);
    } else {
        PreArgs a = input_args(c);
        a.radii = c.out_radii == nullptr ? nullptr : w.radii;
        a.binrec = w.binrec;
        // wave-frames mapping: 64 Gaussians and their SH rows per workgroup, one frame per wave at a time
        if (plan.wave_frames) launch_preprocess<false, true>(stream, plan, pp, w, a);
        else launch_preprocess<false>(stream, plan, pp, w, a);
    }
    // bin passes (bin_kernel): Morton order over records at their slots (shared activation) or gathered from the Gaussians' indices, the
    // gather with a 1-D grid in which each XCD takes whole frames.  The count pass only sums per segment, so it may walk the records in
    // index order instead (bin_index_kernel).  Both passes read the record form the projection launch stored (plan.rec8).
    if (plan.rec8) launch_bin_count<BinRec8>(stream, c, plan, w, order);
    else launch_bin_count<BinRec16>(stream, c, plan, w, order);
    GVF_CHECK_LAUNCH();
    prof_mark(stream, marks, 2);
    hipLaunchKernelGGL(seg_sums_kernel, dim3(plan.scan_blocks), dim3(1024), 0, stream, w.tile_count, plan.nseg, w.partial);
    hipLaunchKernelGGL(seg_scan_kernel, dim3(plan.scan_blocks), dim3(1024), 0, stream, w.tile_count, plan.nseg, plan.ntiles, F,
                       w.partial, plan.scan_blocks, w.ranges, w.cursor, w.frame_base, c.out_num_rendered, w.total,
                       (uint32_t)c.max_rendered, w.cls);
    if (c.max_rendered <= 0)                   // otherwise the scatter pass writes the per-frame counts on its way
        hipLaunchKernelGGL(frame_counts_kernel, dim3((F + 63) / 64), dim3(64), 0, stream, w.frame_base, F, c.out_num_rendered);
    GVF_CHECK_LAUNCH();
    prof_mark(stream, marks, 3);
    if (c.max_rendered > 0) {
        if (plan.rec8) launch_bin_scatter<BinRec8>(stream, c, plan, w, order);
        else launch_bin_scatter<BinRec16>(stream, c, plan, w, order);
        GVF_CHECK_LAUNCH();
    }
    if (c.out_radii != nullptr &&
        hipMemcpyAsync(c.out_radii, w.radii, sizeof(int32_t) * (size_t)F * P, hipMemcpyDeviceToDevice, stream) != hipSuccess)
        return GVF_ELAUNCH;
    prof_mark(stream, marks, 4);
    prof_mark(stream, marks, 5);                // (the radix path's global sort sits between these two)
    return GVF_OK;
}

// Radix binning (kept for comparison): preprocess (+ block sums) -> scan -> duplicate keys + ids -> stable radix sort on the (frame, tile)
// key bits -> tile ranges.  *keys_sorted / *vals_by_tile: where the sorted segments ended up.
int gvf_rast::front_end_radix(hipStream_t stream, const RastCall& c, const RastPlan& plan, const Workspace& w, const hipEvent_t* marks,
                              uint64_t** keys_sorted, uint32_t** vals_by_tile) {
    const int P = c.P, F = c.F;
    prof_mark(stream, marks, 0);
    prof_mark(stream, marks, 1);
    const PreParams pp = pre_params(c, plan);
    PreArgs a = input_args(c);
    a.tiles_touched = w.tiles_touched; a.radii = w.radii; a.block_sums = w.block_sums;
    launch_preprocess<false>(stream, plan, pp, w, a);
    GVF_CHECK_LAUNCH();
    prof_mark(stream, marks, 2);
    hipLaunchKernelGGL(scan_sums_kernel, dim3(1), dim3(1024), 0, stream, w.block_sums, plan.nb, F, w.frame_base,
                       c.out_num_rendered, w.total, (uint32_t)c.max_rendered);
    GVF_CHECK_LAUNCH();
    prof_mark(stream, marks, 3);
    if (c.max_rendered > 0) {
        hipLaunchKernelGGL(duplicate_kernel, dim3(plan.nb, F), dim3(PRE_THREADS), 0, stream, P, plan.gx, plan.gy, w.splats,
                           w.tiles_touched, w.radii, w.block_sums, w.keys, w.vals, (uint32_t)c.max_rendered, pp.upstream_binning);
        GVF_CHECK_LAUNCH();
    }
    if (c.out_radii != nullptr &&
        hipMemcpyAsync(c.out_radii, w.radii, sizeof(int32_t) * (size_t)F * P, hipMemcpyDeviceToDevice, stream) != hipSuccess)
        return GVF_ELAUNCH;
    prof_mark(stream, marks, 4);
    *keys_sorted = w.keys; *vals_by_tile = w.vals;
    if (c.max_rendered > 0) {
        // (a) stable radix sort on the (frame, tile) bits only: segments become contiguous; (b) tile ranges
        int in_alt = 0;
        const int rc = gvf_sort_pairs_device_n(w.keys, w.keys_alt, w.vals, w.vals_alt, w.total, c.max_rendered, 32,
                                               key_end_bit(F, plan.ntiles), w.sort_tmp, w.sort_tmp_bytes, stream, &in_alt);
        if (rc != GVF_OK) return rc;
        if (in_alt) { *keys_sorted = w.keys_alt; *vals_by_tile = w.vals_alt; }
        int rblocks = (int)((c.max_rendered + 255) / 256);
        if (rblocks > 4096) rblocks = 4096;
        hipLaunchKernelGGL(ranges_kernel, dim3(rblocks), dim3(256), 0, stream, *keys_sorted, w.total, (uint32_t)c.max_rendered, w.ranges,
                           (uint32_t)plan.nseg);
        GVF_CHECK_LAUNCH();
    }
    prof_mark(stream, marks, 5);
    return GVF_OK;
}

extern "C" int gvf_gaussian_activate(const GvfGaussianActivation* act, int P, int M, const float* xyz_raw,
                                     const float* features_dc, const float* scaling_raw, const float* rotation_raw,
                                     const float* opacity_raw, const float* delta, float* means3D, float* scales,
                                     float* rotations, float* shs, float* opacities, void* stream) {
    if (!act || P < 0 || M < 1) return GVF_EINVAL;
    if (P == 0) return GVF_OK;
    if (!xyz_raw || !features_dc || !scaling_raw || !rotation_raw || !opacity_raw || !means3D || !scales ||
        !rotations || !shs || !opacities)
        return GVF_EINVAL;
    (void)hipGetLastError();
    hipLaunchKernelGGL(activate_kernel, dim3((P + 255) / 256), dim3(256), 0, (hipStream_t)stream, *act, P, M, xyz_raw,
                       features_dc, scaling_raw, rotation_raw, opacity_raw, delta, means3D, scales, rotations, shs,
                       opacities);
    GVF_CHECK_LAUNCH();
    return GVF_OK;
}
