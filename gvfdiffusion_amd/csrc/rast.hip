// rast.hip -- tile-based 3D-Gaussian-splatting rasteriser for gfx950 (MI355X).
//
// Implements the C ABI of include/gvf_rast.h, i.e. the operator behind the reference's
// GaussianRasterizer seam (renderers/gaussian_render.py:110-143,198-220) with the GaussianModel
// delta activations (representations/gaussian/gaussian_model.py:84-114) optionally fused in front.
// Stages follow SURVEY.md section 8a rows R1..R6 + G1; the arithmetic (operation order, fmaf
// placement, correctly rounded div/sqrt, no contraction: this file is compiled with
// -ffp-contract=off) is the floating-point contract stated in oracle/rast_oracle.c, so that all
// discrete decisions (cull, radius, tile rect, sort order) match the oracle bit for bit.
//
// Launch structure (F frames per call, everything stream-ordered, no host sync; D is read from device memory).
// Default = BUCKET binning (GvfRastSettings.bin_algo):
//   bbox, morton_count/scan/scatter      once per call: 15-bit Morton order of the Gaussians (locality for the bin passes)
//   preprocess   grid (ceil(P/256), F/4) activations (+deltas), EWA covariance, 2D filter, radius, tile rect, alpha-box
//                                        instance culling, SH -> RGB; writes one 64-byte splat record + a 16-byte bin record
//                                        (without shared activation: grid (ceil(P/64), ceil(F/24)), one frame per wave at a time)
//   bin<count>   grid (ceil(P/1024), F)  per-(frame, tile) instance counts: LDS histogram per block, one global atomic
//                                        per touched tile
//   seg_sums, seg_scan, frame_counts     exclusive scan of the counters = tile ranges + cursors, per-frame D, overflow guard
//   bin<scatter> grid (ceil(P/1024), F)  (depth_bits << 32 | id) into the tile segments (order inside a segment arbitrary)
//   classify + tile_sort                 per-tile sort: registers+shuffles / static LDS for segments <= 1536 (SORT_SMALL_N), LDS <= 16384,
//                                        in-place global beyond; writes ordered ids (= upstream's stable (tile, depth) order)
//   blend        grid (tiles, F)         16x16 px per workgroup, 4 waves = the four 8x8 quadrants
// RADIX binning (kept for comparison): preprocess (+block sums) -> scan_sums -> duplicate ((frame*tiles + tile) << 32 |
// depth keys + ids) -> two stable 8-bit LSD passes over the (frame, tile) key bits (sort.hip) -> ranges -> tile_sort.
// Upstream sorts all 64-bit (tile, depth) keys with one global radix sort (>= 6 passes over 12 B per instance);
// here no global sort is left and the depth order is produced on chip.
// This file: front end, host pipeline, entry points.  Per-tile sort: rast_sort.hip; blend: rast_blend.hip; backward (R7): rast_bwd.hip;
// what they share: rast_common.h.
//
// HBM layout (caller-owned workspace, carved below): per (frame, Gaussian) ONE 64-byte, 64-byte-aligned record
//   float4 {x, y, conic_a, conic_b} | float4 {conic_c, opacity, r, g} | float4 {b, depth, hx, hy} | 16 B unused
// so the blend's gather of a (splat, tile) instance touches exactly one cache line (three 40-B-total arrays cost
// three lines per instance: 5.7 GB of fabric reads per 24-frame step measured with FETCH_SIZE, vs 1.1 GB
// algorithmic); hx, hy = half extents of the region where alpha can reach 1/255 (instance and quadrant culling),
// computed once per visible Gaussian.  A 16-byte bin record {x0|y0<<16, x1|y1<<16, depth bits, 0}; per
// (frame, tile) a range, a counter and a cursor; per instance one u64 key and one u32 ordered id (radix path:
// u64 key + u32 id, double buffered).
#include <atomic>
#include <cstdlib>
#include <vector>
#include "rast_common.h"
#include "gvf_sort.h"

namespace {

#ifndef GVF_PRE_FB
#define GVF_PRE_FB 4
#endif
constexpr int PRE_FB = GVF_PRE_FB;   // frames per preprocess workgroup: the frame-invariant inputs (xyz, scale, rotation, opacity,
                            // SH: 164 of the 220 input bytes per Gaussian at degree 2) come from HBM once per PRE_FB frames
// Wave-frames mapping (preprocess_kernel<false, true>, the bucket-binning launch without shared activation): 64 Gaussians per workgroup, each of
// its PRE_WAVES waves walks PRE_WAVE_FB frames, so the frame-invariant inputs come from HBM once per PRE_WAVES * PRE_WAVE_FB = 24 frames on
// a grid that keeps ceil(P / 64) workgroups per frame group.  Against PRE_FB = 4 on the 256-Gaussian mapping the launch takes 240 us instead
// of 275 at 24 frames; 3 frames per wave (twice as many, shorter workgroups) is not faster (profiles/r14_preprocess_wave_frames_ab.txt).
#ifndef GVF_PRE_WAVE_FB
#define GVF_PRE_WAVE_FB 6
#endif
constexpr int PRE_WAVES = PRE_THREADS / GVF_WAVE;
constexpr int PRE_WAVE_FB = GVF_PRE_WAVE_FB;
// preprocess_kernel runs on a (Gaussian blocks, frame groups) grid.  Measured and not adopted (profiles/r05_preprocess_variants_ab.txt): an
// XCD-aware workgroup order and requesting the next frame's delta row ahead -- the launch waits neither on L2 hits nor on bytes in flight.
// The fused launch reads its delta rows straight from global memory: staging them through LDS costs occupancy and is slower
// (profiles/r07_preprocess_forms_ab.txt).
// Bucket binning of the calls without shared activation (preprocess_kernel<false>): the bin records are stored at the Gaussian's own index
// (coalesced lines), the count pass (bin_index_kernel) walks them in index order against a whole-frame LDS tile table, and the scatter pass
// (bin_kernel) gathers them in Morton order, each XCD taking whole frames.  Records at the Morton slot, or both passes in one order, are
// slower (profiles/r07_bin_layout_ab.txt).  The shared-activation path keeps its records at the Morton slot.

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
constexpr int ACT_MAX_SLICES = 16;
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
    // records (16 bytes each, scattered to the slot by the index-ordered form: 21 % of that launch) are all contiguous.
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

// SHARED: a0 = the stage-A records [slices][P][4 x float4] (see activate_cov_kernel), frames[f].reserved[0] = the frame's slice
// WAVE_FRAMES (bucket binning without shared activation; block_sums and tiles_touched are null by construction): the workgroup owns 64
// consecutive Gaussians instead of 256 and its four waves walk different frames -- wave w takes frames 4 G by + w + 4 ff, ff = 0 .. G - 1
// (G = PRE_WAVE_FB) -- so the SH rows are staged once per 4 G frames and the raw inputs come across the fabric once per 4 G frames, on a grid
// that keeps ceil(P / 64) x ceil(F / 4G) workgroups.  One barrier, after the staging; the waves never meet again.  What a wave loads and stores
// per frame (delta rows, quad-transposed splat records, bin records) and the per-Gaussian arithmetic are those of the other mapping.
template <bool SHARED, bool WAVE_FRAMES = false>
__global__ __launch_bounds__(PRE_THREADS) void preprocess_kernel(
    PreParams pp, const GvfRastFrame* __restrict__ frames, const float* __restrict__ a0,
    const float* __restrict__ a1, const float* __restrict__ a2, const float* __restrict__ a3,
    const float* __restrict__ sh, const float* __restrict__ colors_precomp,
    const float* __restrict__ cov3D_precomp, const float* __restrict__ delta, float4* __restrict__ splats,
    uint32_t* __restrict__ tiles_touched,
    int32_t* __restrict__ radii, uint32_t* __restrict__ block_sums, uint4* __restrict__ binrec,
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
        // bucket binning: the final tile rect and the depth, 16 B that the count / scatter passes gather by id
        if (binrec != nullptr) {
            binrec[(size_t)f * P + my_slot] = make_uint4((uint32_t)rect.x0 | ((uint32_t)rect.y0 << 16),
                                                         (uint32_t)rect.x1 | ((uint32_t)rect.y1 << 16), __float_as_uint(gC.y), 0u);
        }
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
constexpr int SCAN_CHUNK = 4096;
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
// and are gathered, and xcd_frames = 1 then lays the grid out 1-D so that each XCD takes whole frames (see the host).
constexpr int WIN_MAX = 2048;
constexpr int BIN_SPT = 4;
constexpr int BIN_SLOTS = PRE_THREADS * BIN_SPT;

template <bool SCATTER>
__global__ __launch_bounds__(PRE_THREADS) void bin_kernel(int P, int gx, int gy, const uint4* __restrict__ binrec,
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
            const uint4 br = binrec[(size_t)f * P + (rec_by_id ? id : (uint32_t)s)];
            x0[k] = (int)(br.x & 0xffffu); y0[k] = (int)(br.x >> 16);
            x1[k] = (int)(br.y & 0xffffu); y1[k] = (int)(br.y >> 16);
            key[k] = ((uint64_t)br.z << 32) | id;                      // depth bits above the Gaussian id
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
constexpr int BINX_TAB = 4096;
constexpr int BINX_PER_WG = 8192;
constexpr int BINX_SPT = 4;                          // records in flight per thread

__global__ __launch_bounds__(BINX_THREADS) void bin_index_kernel(int P, int gx, const uint4* __restrict__ binrec,
                                                                 uint32_t* __restrict__ tile_count,
                                                                 uint32_t* __restrict__ cursor,
                                                                 const uint32_t* __restrict__ total,
                                                                 uint64_t* __restrict__ payload, int ntiles,
                                                                 const uint32_t* __restrict__ frame_base, uint32_t* __restrict__ num_rendered) {
    __shared__ uint32_t s_tab[BINX_TAB];
    const int t = threadIdx.x, f = blockIdx.y;
    const int g0 = (int)blockIdx.x * BINX_PER_WG, g1 = min(P, g0 + BINX_PER_WG);
    const uint4* rec = binrec + (size_t)f * P;
    for (int e = t; e < ntiles; e += BINX_THREADS) s_tab[e] = 0u;
    __syncthreads();
    for (int base = g0; base < g1; base += BINX_SPT * BINX_THREADS) {
        uint4 br[BINX_SPT];
#pragma unroll
        for (int k = 0; k < BINX_SPT; ++k) {
            const int s = base + k * BINX_THREADS + t;
            br[k] = s < g1 ? rec[s] : make_uint4(0u, 0u, 0u, 0u);     // {0, 0, 0, 0}: an empty rect
        }
#pragma unroll
        for (int k = 0; k < BINX_SPT; ++k) {
            const int x0 = (int)(br[k].x & 0xffffu), y0 = (int)(br[k].x >> 16);
            const int x1 = (int)(br[k].y & 0xffffu), y1 = (int)(br[k].y >> 16);
            for (int y = y0; y < y1; ++y)
                for (int x = x0; x < x1; ++x) atomicAdd(&s_tab[y * gx + x], 1u);
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

constexpr int MORTON_BINS = 1 << 15;

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
// host side
// ---------------------------------------------------------------------------------------------
// Opt-in stage timing (HIP events on the caller's stream), used by bench.py for the roofline figure.
// The only process-global state in this library; off by default.
constexpr int PROF_MAX_CALLS = 256;
constexpr int PROF_EVENTS = GVF_RAST_NSTAGES + 1;
struct Profiler {
    bool on = false;
    std::atomic<int> calls{0};          // slots are handed out to concurrent callers (one host thread per sample in flight)
    hipEvent_t ev[PROF_MAX_CALLS][PROF_EVENTS];
};
Profiler g_prof;
inline void prof_mark(hipStream_t s, int slot, int k) {
    if (slot >= 0) (void)hipEventRecord(g_prof.ev[slot][k], s);
}

int key_end_bit(int F, int ntiles) {
    uint64_t m = (uint64_t)F * (uint64_t)ntiles;
    int bits = 0;
    while (((uint64_t)1 << bits) < m) ++bits;
    return 32 + bits;
}

std::atomic<long long> g_shared_calls{0};

int run_pipeline(const GvfRastSettings& st, const GvfRastFrame* frames_host, int F, int P, int M, bool fused,
                 const GvfGaussianActivation* act, const float* a0, const float* a1, const float* a2,
                 const float* a3, const float* sh, const float* colors_precomp, const float* cov3D_precomp,
                 const float* delta, int n_delta, const float* subpixel_offset, void* workspace,
                 size_t workspace_bytes, int64_t max_rendered, float* out_color, float* out_alpha,
                 float* out_depth, int32_t* out_radii, uint32_t* out_num_rendered, hipStream_t stream,
                 unsigned char* out_u8 = nullptr /* instead of out_color: uint8 frames (gvf_rast_forward_batched_u8) */) {
    const int H = st.image_height, W = st.image_width;
    if (H <= 0 || W <= 0 || P < 0 || F <= 0 || max_rendered < 0 || max_rendered > 0xFFFFFFFFll) return GVF_EINVAL;
    if (st.sh_degree < 0 || st.sh_degree > 3) return GVF_EINVAL;
    if (st.mode != GVF_RAST_MODE_MIP && st.mode != GVF_RAST_MODE_DILATE) return GVF_EINVAL;
    if ((out_color == nullptr) == (out_u8 == nullptr) || !out_num_rendered || !frames_host || !workspace) return GVF_EINVAL;
    if (P > 0 && colors_precomp == nullptr) {
        if (sh == nullptr || M < (st.sh_degree + 1) * (st.sh_degree + 1) || M > MAX_SH_COEFFS) return GVF_EINVAL;
    }
    // hipGetLastError() is process-wide: clear what other users of the runtime (e.g. an event query that
    // returned hipErrorNotReady) left behind, so GVF_CHECK_LAUNCH reports only this call's launches.
    (void)hipGetLastError();
    if ((((uintptr_t)sh) & 15) != 0 || (((uintptr_t)workspace) & 255) != 0) return GVF_EINVAL;  // 16-B SH rows, 256-B workspace
    Workspace w = carve(workspace, workspace_bytes, P, F, H, W, max_rendered);
    if (!w.ok) return GVF_ENOSPC;

    const int gx = (W + TILE - 1) / TILE, gy = (H + TILE - 1) / TILE, ntiles = gx * gy;
    const int nb = (P + PRE_THREADS - 1) / PRE_THREADS;
    int slot = g_prof.on ? g_prof.calls.fetch_add(1) : -1;
    if (slot >= PROF_MAX_CALLS) slot = -1;

    // ---- shared activation (activate_cov_kernel): the call's distinct delta slices, if they are few.  The records live in keys_alt, which only
    // the radix binning uses (max_rendered x 8 bytes: room for max_rendered / (8 P) slices; a sizing call with max_rendered = 0 takes the fused path,
    // whose outputs are the same bits).  GVF_RAST_SHARED_ACT=0: measurement / test switch.
    ActSlices slices; slices.n = 0;
    bool shared = false;
    std::vector<int> frame_slice((size_t)F, 0);
    const char* shared_env = getenv("GVF_RAST_SHARED_ACT");          // read per call: tests switch it inside one process
    const bool shared_on = !(shared_env && shared_env[0] == '0');
    // GVF_RAST_PRE_WAVE_FRAMES=0: test switch, the bucket-binning fused launch on the 256-Gaussian mapping (preprocess_kernel<false>)
    const char* wf_env = getenv("GVF_RAST_PRE_WAVE_FRAMES");         // read per call, like the switch above
    const bool wave_frames_on = !(wf_env && wf_env[0] == '0');
    if (shared_on && fused && cov3D_precomp == nullptr && st.bin_algo != GVF_RAST_BIN_RADIX && P > 0 && F >= 2) {
        shared = true;
        for (int f = 0; f < F && shared; ++f) {
            const int di = (delta != nullptr && frames_host[f].delta_index >= 0) ? frames_host[f].delta_index : -1;
            int k = 0;
            while (k < slices.n && slices.di[k] != di) ++k;
            if (k == slices.n) {
                if (slices.n == ACT_MAX_SLICES) { shared = false; break; }
                slices.di[slices.n++] = di;
            }
            frame_slice[(size_t)f] = k;
        }
        // worth it from two frames per slice on; the records must fit into keys_alt
        if (shared && (F < 2 * slices.n || (size_t)slices.n * (size_t)P * 64u > (size_t)(max_rendered > 0 ? max_rendered : 0) * 8u)) shared = false;
    }
    // bucket binning without shared activation: bin_index_kernel takes the count pass when a frame's tiles fit its table
    const bool index_count = st.bin_algo != GVF_RAST_BIN_RADIX && !shared && ntiles <= BINX_TAB;
    const bool morton = st.bin_algo != GVF_RAST_BIN_RADIX && F >= 4 && P >= 4096;   // spatial order of the Gaussians (see below)
    // slot order of the shared-activation path (see activate_cov_kernel): needs the Morton order, SH input and room for the slot-ordered SH copy
    // behind the records.  Decided here, in front of the upload launch, which records it for the backward (LAYOUT_WORD).
    // GVF_RAST_SLOT_ORDER=0: measurement / test switch
    const char* slot_env = getenv("GVF_RAST_SLOT_ORDER");
    const size_t sh_floats = (size_t)(colors_precomp ? 0 : M) * 3;
    const bool slot_mode = shared && !(slot_env && slot_env[0] == '0') && morton && nb > 0 && colors_precomp == nullptr && sh != nullptr &&
                           (size_t)slices.n * (size_t)P * 64u + (size_t)P * sh_floats * 4u <= (size_t)max_rendered * 8u;
    const uint32_t layout = slot_mode ? LAYOUT_SLOT_ORDER : 0u;
    for (int f0 = 0; f0 < F; f0 += 16) {
        FrameChunk ch;
        const int cnt = F - f0 < 16 ? F - f0 : 16;
        for (int k = 0; k < cnt; ++k) {
            ch.f[k] = frames_host[f0 + k];
            ch.f[k].reserved[0] = shared ? frame_slice[(size_t)(f0 + k)] : 0;       // the device copy's slice index (the caller's block is not touched)
        }
        CallTables tab = {};
        if (f0 == 0) {
            const size_t nseg_all = (size_t)F * ntiles;
            tab.ranges = reinterpret_cast<uint32_t*>(w.ranges); tab.n_ranges = (uint32_t)(2 * nseg_all);
            tab.tile_count = w.tile_count; tab.n_tile_count = (uint32_t)nseg_all;
            tab.mhist = w.mhist; tab.n_mhist = morton ? (uint32_t)MORTON_BINS : 0u;
            tab.cls = w.cls; tab.mm = w.mm; tab.layout = layout;
        }
        const size_t clear_words = (size_t)tab.n_ranges + tab.n_tile_count + tab.n_mhist;
        const int zb = f0 == 0 ? (int)((clear_words + 4095) / 4096 < 256 ? (clear_words + 4095) / 4096 : 256) : 0;
        hipLaunchKernelGGL(upload_frames_kernel, dim3(1 + zb), dim3(256), 0, stream, ch, cnt, w.frames + f0, tab);
    }
    GVF_CHECK_LAUNCH();

    const uint32_t* blend_rec_of = nullptr;           // slot order: Gaussian id -> index of its splat record inside a frame
    if (P == 0 || nb == 0) {
        // nothing to splat: background only
        if (hipMemsetAsync(out_num_rendered, 0, sizeof(uint32_t) * F, stream) != hipSuccess) return GVF_ELAUNCH;
    } else {
        const bool bucket = st.bin_algo != GVF_RAST_BIN_RADIX;
        prof_mark(stream, slot, 0);
        // ---- spatial order of the Gaussians (bucket binning, several frames to amortise it over) ----
        const uint32_t* order = nullptr;
        if (morton) {                                  // (bounding box accumulators and histogram: cleared by the upload launch)
            int bb = (P + 255) / 256; if (bb > 128) bb = 128;
            const int pb = (P + 255) / 256;
            hipLaunchKernelGGL(bbox_kernel, dim3(bb), dim3(256), 0, stream, P, a0, w.mm);
            hipLaunchKernelGGL(morton_count_kernel, dim3(pb), dim3(256), 0, stream, P, a0, w.mm, w.order_alt, w.mhist);
            hipLaunchKernelGGL(morton_scan_kernel, dim3(1), dim3(1024), 0, stream, w.mhist);
            hipLaunchKernelGGL(morton_scatter_kernel, dim3(pb), dim3(256), 0, stream, P, w.order_alt, w.mhist, w.order);
            order = w.order;
            GVF_CHECK_LAUNCH();
        }
        // preprocess_kernel<false> stores the bin records at the Gaussians' indices, bin_kernel gathers them in Morton order
        const bool rec_gather = bucket && !shared && order != nullptr;
        const unsigned nseg = (unsigned)((size_t)F * ntiles);
        prof_mark(stream, slot, 1);
        PreParams pp;
        pp.P = P; pp.M = colors_precomp ? 0 : M; pp.deg = st.sh_degree; pp.H = H; pp.W = W; pp.mode = st.mode;
        pp.gx = gx; pp.gy = gy; pp.kernel_size = st.kernel_size; pp.scale_modifier = st.scale_modifier;
        pp.fused = fused ? 1 : 0; pp.n_delta = n_delta; pp.F = F;
        // per-pixel sub-pixel offsets move the sample positions: no box culling then (as in the blend)
        pp.upstream_binning = (st.upstream_binning != 0 || subpixel_offset != nullptr) ? 1 : 0;
        if (fused) pp.act = *act; else pp.act = GvfGaussianActivation{};
        const size_t sh_lds_bytes = gvf_align_up((size_t)PRE_THREADS * pp.M * 3 * sizeof(float), 16) + 16;
        pp.delta_lds = 0;
        const dim3 pre_grid(nb, (F + PRE_FB - 1) / PRE_FB);
        if (shared) {
            g_shared_calls.fetch_add(1, std::memory_order_relaxed);
            float4* rec3d = reinterpret_cast<float4*>(w.keys_alt);
            float* sh_by_slot = slot_mode ? reinterpret_cast<float*>(rec3d + 4 * (size_t)slices.n * (size_t)P) : nullptr;
            hipLaunchKernelGGL(activate_cov_kernel, dim3((P + 255) / 256, slices.n), dim3(256), 0, stream, *act, st.scale_modifier, P, slices,
                               a0, a1, a2, a3, delta, rec3d, slot_mode ? w.order_alt : nullptr, sh, (int)sh_floats, sh_by_slot);
            if (slot_mode) {
                // thread i = slot i: records, SH rows, splat records and bin records are all read / written at i; the sorted lists keep Gaussian
                // ids (ties break by index, as upstream's stable sort does) and the blend looks the record index up (rec_of)
                blend_rec_of = w.order_alt;
                hipLaunchKernelGGL(preprocess_kernel<true>, pre_grid, dim3(PRE_THREADS), sh_lds_bytes, stream, pp,
                                   w.frames, reinterpret_cast<const float*>(rec3d), reinterpret_cast<const float*>(order), nullptr, nullptr, sh_by_slot,
                                   nullptr, nullptr, nullptr, w.splats, nullptr, out_radii == nullptr ? nullptr : w.radii, nullptr, w.binrec, nullptr);
            } else
            hipLaunchKernelGGL(preprocess_kernel<true>, pre_grid, dim3(PRE_THREADS), sh_lds_bytes, stream, pp,
                               w.frames, reinterpret_cast<const float*>(rec3d), nullptr, nullptr, nullptr, colors_precomp ? nullptr : sh, colors_precomp,
                               nullptr, nullptr, w.splats, nullptr, out_radii == nullptr ? nullptr : w.radii, nullptr, w.binrec,
                               order != nullptr ? w.order_alt : nullptr);
        } else if (bucket && wave_frames_on) {
            // wave-frames mapping (preprocess_kernel<false, true>): 64 Gaussians and their SH rows per workgroup, one frame per wave at a time
            const size_t wf_lds_bytes = gvf_align_up((size_t)GVF_WAVE * pp.M * 3 * sizeof(float), 16) + 16;
            const dim3 wf_grid((P + GVF_WAVE - 1) / GVF_WAVE, (F + PRE_WAVES * PRE_WAVE_FB - 1) / (PRE_WAVES * PRE_WAVE_FB));
            hipLaunchKernelGGL((preprocess_kernel<false, true>), wf_grid, dim3(PRE_THREADS), wf_lds_bytes, stream, pp,
                               w.frames, a0, a1, a2, a3, colors_precomp ? nullptr : sh, colors_precomp, cov3D_precomp, delta,
                               w.splats, nullptr, out_radii == nullptr ? nullptr : w.radii, nullptr, w.binrec, nullptr);
        } else
        hipLaunchKernelGGL(preprocess_kernel<false>, pre_grid, dim3(PRE_THREADS), sh_lds_bytes, stream, pp,
                           w.frames, a0, a1, a2, a3, colors_precomp ? nullptr : sh, colors_precomp, cov3D_precomp, delta,
                           w.splats, bucket ? nullptr : w.tiles_touched, (bucket && out_radii == nullptr) ? nullptr : w.radii,
                           bucket ? nullptr : w.block_sums, bucket ? w.binrec : nullptr, nullptr);
        // bin passes (bin_kernel): Morton order over records at their slots (shared activation) or gathered from the Gaussians' indices, the
        // gather with a 1-D grid in which each XCD takes whole frames.  The count pass only sums per segment, so it may walk the records in
        // index order instead (bin_index_kernel).
        const int bnb = (P + BIN_SLOTS - 1) / BIN_SLOTS, xnb = (P + BINX_PER_WG - 1) / BINX_PER_WG;
        const dim3 bin_grid = rec_gather ? dim3((unsigned)((F + 7) / 8 * 8 * bnb)) : dim3(bnb, F);
        if (index_count)
            hipLaunchKernelGGL(bin_index_kernel, dim3(xnb, F), dim3(BINX_THREADS), 0, stream, P, gx, w.binrec,
                               w.tile_count, w.cursor, w.total, w.keys, ntiles, nullptr, nullptr);
        else if (bucket)
            hipLaunchKernelGGL(bin_kernel<false>, bin_grid, dim3(PRE_THREADS), 0, stream, P, gx, gy, w.binrec, order,
                               w.tile_count, w.cursor, w.total, w.keys, nullptr, nullptr, rec_gather ? 1 : 0, rec_gather ? 1 : 0, F);
        GVF_CHECK_LAUNCH();
        prof_mark(stream, slot, 2);
        if (bucket)
        {
            const int sblocks = (int)((nseg + SCAN_CHUNK - 1) / SCAN_CHUNK);
            hipLaunchKernelGGL(seg_sums_kernel, dim3(sblocks), dim3(1024), 0, stream, w.tile_count, (int)nseg, w.partial);
            hipLaunchKernelGGL(seg_scan_kernel, dim3(sblocks), dim3(1024), 0, stream, w.tile_count, (int)nseg, ntiles, F,
                               w.partial, sblocks, w.ranges, w.cursor, w.frame_base, out_num_rendered, w.total,
                               (uint32_t)max_rendered, w.cls);
            if (max_rendered <= 0)                   // otherwise the scatter pass writes the per-frame counts on its way
                hipLaunchKernelGGL(frame_counts_kernel, dim3((F + 63) / 64), dim3(64), 0, stream, w.frame_base, F, out_num_rendered);
        }
        else
            hipLaunchKernelGGL(scan_sums_kernel, dim3(1), dim3(1024), 0, stream, w.block_sums, nb, F, w.frame_base,
                               out_num_rendered, w.total, (uint32_t)max_rendered);
        GVF_CHECK_LAUNCH();
        prof_mark(stream, slot, 3);
        if (max_rendered > 0) {
            if (bucket)
                hipLaunchKernelGGL(bin_kernel<true>, bin_grid, dim3(PRE_THREADS), 0, stream, P, gx, gy, w.binrec, order,
                                   w.tile_count, w.cursor, w.total, w.keys, w.frame_base, out_num_rendered,
                                   rec_gather ? 1 : 0, rec_gather ? 1 : 0, F);
            else
                hipLaunchKernelGGL(duplicate_kernel, dim3(nb, F), dim3(PRE_THREADS), 0, stream, P, gx, gy, w.splats,
                                   w.tiles_touched, w.radii, w.block_sums, w.keys, w.vals, (uint32_t)max_rendered,
                                   pp.upstream_binning);
            GVF_CHECK_LAUNCH();
        }
        if (out_radii != nullptr) {
            if (hipMemcpyAsync(out_radii, w.radii, sizeof(int32_t) * (size_t)F * P, hipMemcpyDeviceToDevice, stream) != hipSuccess)
                return GVF_ELAUNCH;
        }
        prof_mark(stream, slot, 4);
        if (max_rendered > 0) {
            uint64_t* keys_sorted = w.keys;
            uint32_t* vals_by_tile = nullptr;
            if (!bucket) {
                // (a) stable radix sort on the (frame, tile) bits only: segments become contiguous; (b) tile ranges
                vals_by_tile = w.vals;
                int in_alt = 0;
                int rc = gvf_sort_pairs_device_n(w.keys, w.keys_alt, w.vals, w.vals_alt, w.total, max_rendered, 32,
                                                 key_end_bit(F, ntiles), w.sort_tmp, w.sort_tmp_bytes, stream, &in_alt);
                if (rc != GVF_OK) return rc;
                if (in_alt) { keys_sorted = w.keys_alt; vals_by_tile = w.vals_alt; }
                int rblocks = (int)((max_rendered + 255) / 256);
                if (rblocks > 4096) rblocks = 4096;
                hipLaunchKernelGGL(ranges_kernel, dim3(rblocks), dim3(256), 0, stream, keys_sorted, w.total,
                                   (uint32_t)max_rendered, w.ranges, (uint32_t)nseg);
                GVF_CHECK_LAUNCH();
            }
            prof_mark(stream, slot, 5);
            // per-tile on-chip sort by (depth, id)
            const int rc = launch_tile_sort(stream, w.ranges, keys_sorted, vals_by_tile, w.ids, w.cls, nseg, bucket ? 2 : 1);
            if (rc != GVF_OK) return rc;
        } else {
            prof_mark(stream, slot, 5);
        }
    }
    // heaviest tiles first (blend_order_kernel; the scatter pass is done with its cursors: their array takes the order).  Worth a launch when the
    // frames' workgroups outnumber the chip's resident slots; GVF_RAST_BLEND_ORDER=0: measurement switch
    const char* order_env = getenv("GVF_RAST_BLEND_ORDER");
    const bool order_tiles = !(order_env && order_env[0] == '0') && P > 0 && nb > 0 && max_rendered > 0 && (size_t)F * ntiles >= 2048;
    const int rc = launch_blend(stream, st, P, F, w.ranges, w.ids, w.splats, subpixel_offset, out_color, out_alpha, out_depth, out_u8,
                                blend_rec_of, order_tiles ? w.cursor : nullptr, slot >= 0 ? g_prof.ev[slot][6] : nullptr);
    if (rc != GVF_OK) return rc;
    prof_mark(stream, slot, 7);
    return GVF_OK;
}

}  // namespace

Workspace gvf_rast::carve(void* ws, size_t bytes, int P, int F, int H, int W, int64_t max_rendered) {
    Workspace w;
    GvfCarver c(ws, bytes);
    const int nb = (P + PRE_THREADS - 1) / PRE_THREADS;
    const int ntiles = ((W + TILE - 1) / TILE) * ((H + TILE - 1) / TILE);
    const size_t FP = (size_t)F * (size_t)(P > 0 ? P : 1);
    const size_t D = (size_t)(max_rendered > 0 ? max_rendered : 1);
    w.frames = c.take<GvfRastFrame>(F);
    w.splats = c.take<float4>(4 * FP);
    w.tiles_touched = c.take<uint32_t>(FP);
    w.radii = c.take<int32_t>(FP);
    w.block_sums = c.take<uint32_t>((size_t)F * (nb > 0 ? nb : 1));
    w.frame_base = c.take<uint32_t>(F + 1);
    w.total = c.take<uint32_t>(1);
    w.keys = c.take<uint64_t>(D);
    w.keys_alt = c.take<uint64_t>(D);
    w.vals = c.take<uint32_t>(D);
    w.vals_alt = c.take<uint32_t>(D);
    w.ids = c.take<uint32_t>(D);
    w.ranges = c.take<uint2>((size_t)F * ntiles);
    w.cls = c.take<uint32_t>(2 + 2 * (size_t)F * ntiles);
    w.tile_count = c.take<uint32_t>((size_t)F * ntiles);
    w.cursor = c.take<uint32_t>((size_t)F * ntiles);
    w.partial = c.take<uint32_t>(((size_t)F * ntiles + SCAN_CHUNK - 1) / SCAN_CHUNK + 1);
    const size_t Pp = (size_t)(P > 0 ? P : 1);
    w.order = c.take<uint32_t>(Pp);
    w.order_alt = c.take<uint32_t>(Pp);
    w.mhist = c.take<uint32_t>(1 << 15);
    w.mm = c.take<uint32_t>(8);
    w.binrec = c.take<uint4>(FP);
    w.sort_tmp_bytes = gvf_sort_tmp_bytes((int64_t)D);
    w.sort_tmp = c.take<char>(w.sort_tmp_bytes);
    w.bytes = gvf_align_up(c.off, 256);
    w.ok = c.ok;
    return w;
}

extern "C" int gvf_rast_workspace_bytes(int P, int F, int H, int W, int64_t max_rendered, size_t* bytes) {
    if (!bytes || P < 0 || F <= 0 || H <= 0 || W <= 0 || max_rendered < 0) return GVF_EINVAL;
    Workspace w = carve(nullptr, (size_t)-1, P, F, H, W, max_rendered);
    *bytes = w.bytes + 256;
    (void)tile_sort_set_lds_limit();        // best effort here (no device in a CPU-only process); launch_tile_sort insists
    return GVF_OK;
}

extern "C" int gvf_rast_forward(const GvfRastSettings* st, const GvfRastFrame* frame_host, int P, int M,
                                const float* means3D, const float* shs, const float* colors_precomp,
                                const float* opacities, const float* scales, const float* rotations,
                                const float* cov3D_precomp, const float* subpixel_offset, void* workspace,
                                size_t workspace_bytes, int64_t max_rendered, float* out_color, float* out_alpha,
                                float* out_depth, int32_t* out_radii, uint32_t* out_num_rendered, void* stream) {
    if (!st || !frame_host) return GVF_EINVAL;
    if (P > 0) {
        if (!means3D || !opacities) return GVF_EINVAL;
        // exactly one colour source and exactly one covariance source (upstream wrapper contract)
        if ((shs == nullptr) == (colors_precomp == nullptr)) return GVF_EINVAL;
        const bool have_sr = scales != nullptr && rotations != nullptr;
        if (have_sr == (cov3D_precomp != nullptr)) return GVF_EINVAL;
    }
    return run_pipeline(*st, frame_host, 1, P, M, false, nullptr, means3D, scales, rotations, opacities, shs,
                        colors_precomp, cov3D_precomp, nullptr, 0, subpixel_offset, workspace, workspace_bytes,
                        max_rendered, out_color, out_alpha, out_depth, out_radii, out_num_rendered,
                        (hipStream_t)stream);
}

extern "C" int gvf_rast_forward_batched(const GvfRastSettings* st, const GvfRastFrame* frames_host, int F,
                                        const GvfGaussianActivation* act, int P, int M, const float* xyz_raw,
                                        const float* features_dc, const float* scaling_raw,
                                        const float* rotation_raw, const float* opacity_raw, const float* delta,
                                        int n_delta, void* workspace, size_t workspace_bytes,
                                        int64_t max_rendered, float* out_color, float* out_alpha, float* out_depth,
                                        int32_t* out_radii, uint32_t* out_num_rendered, void* stream) {
    if (!st || !frames_host || !act || F <= 0) return GVF_EINVAL;
    if (P > 0 && (!xyz_raw || !features_dc || !scaling_raw || !rotation_raw || !opacity_raw)) return GVF_EINVAL;
    if (act->scaling_activation != 0 && act->scaling_activation != 1) return GVF_EINVAL;
    for (int f = 0; f < F; ++f) {
        int di = frames_host[f].delta_index;
        if (di >= 0 && (delta == nullptr || di >= n_delta)) return GVF_EINVAL;
    }
    return run_pipeline(*st, frames_host, F, P, M, true, act, xyz_raw, scaling_raw, rotation_raw, opacity_raw,
                        features_dc, nullptr, nullptr, delta, n_delta, nullptr, workspace, workspace_bytes,
                        max_rendered, out_color, out_alpha, out_depth, out_radii, out_num_rendered,
                        (hipStream_t)stream);
}

// the batched call with the frames leaving as uint8 (the reference's post-process, utils/inference_utils.py:280-286, in the blend's epilogue)
extern "C" int gvf_rast_forward_batched_u8(const GvfRastSettings* st, const GvfRastFrame* frames_host, int F,
                                           const GvfGaussianActivation* act, int P, int M, const float* xyz_raw,
                                           const float* features_dc, const float* scaling_raw,
                                           const float* rotation_raw, const float* opacity_raw, const float* delta,
                                           int n_delta, void* workspace, size_t workspace_bytes,
                                           int64_t max_rendered, uint8_t* out_rgb_u8, uint32_t* out_num_rendered, void* stream) {
    if (!st || !frames_host || !act || F <= 0 || !out_rgb_u8) return GVF_EINVAL;
    if (P > 0 && (!xyz_raw || !features_dc || !scaling_raw || !rotation_raw || !opacity_raw)) return GVF_EINVAL;
    if (act->scaling_activation != 0 && act->scaling_activation != 1) return GVF_EINVAL;
    for (int f = 0; f < F; ++f) {
        int di = frames_host[f].delta_index;
        if (di >= 0 && (delta == nullptr || di >= n_delta)) return GVF_EINVAL;
    }
    return run_pipeline(*st, frames_host, F, P, M, true, act, xyz_raw, scaling_raw, rotation_raw, opacity_raw,
                        features_dc, nullptr, nullptr, delta, n_delta, nullptr, workspace, workspace_bytes,
                        max_rendered, nullptr, nullptr, nullptr, nullptr, out_num_rendered, (hipStream_t)stream, out_rgb_u8);
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

extern "C" int gvf_rast_profile_enable(int on) {
    if (on && !g_prof.on) {
        for (int c = 0; c < PROF_MAX_CALLS; ++c)
            for (int k = 0; k < PROF_EVENTS; ++k)
                if (hipEventCreate(&g_prof.ev[c][k]) != hipSuccess) return GVF_ELAUNCH;
        g_prof.on = true;
        g_prof.calls = 0;
    } else if (!on && g_prof.on) {
        for (int c = 0; c < PROF_MAX_CALLS; ++c)
            for (int k = 0; k < PROF_EVENTS; ++k) (void)hipEventDestroy(g_prof.ev[c][k]);
        g_prof.on = false;
        g_prof.calls = 0;
    }
    return GVF_OK;
}

extern "C" int64_t gvf_rast_shared_activation_calls(void) { return (int64_t)g_shared_calls.load(std::memory_order_relaxed); }

extern "C" int gvf_rast_profile_read(float* ms_sum, int* calls) {
    if (!ms_sum || !calls) return GVF_EINVAL;
    for (int k = 0; k < GVF_RAST_NSTAGES; ++k) ms_sum[k] = 0.f;
    *calls = 0;
    if (!g_prof.on) return GVF_OK;
    const int n_calls = g_prof.calls.load() < PROF_MAX_CALLS ? g_prof.calls.load() : PROF_MAX_CALLS;
    for (int c = 0; c < n_calls; ++c) {
        if (hipEventSynchronize(g_prof.ev[c][PROF_EVENTS - 1]) != hipSuccess) return GVF_ELAUNCH;
        for (int k = 0; k < GVF_RAST_NSTAGES; ++k) {
            float ms = 0.f;
            if (hipEventElapsedTime(&ms, g_prof.ev[c][k], g_prof.ev[c][k + 1]) != hipSuccess) return GVF_ELAUNCH;
            ms_sum[k] += ms;
        }
    }
    *calls = n_calls;
    g_prof.calls = 0;
    return GVF_OK;
}

extern "C" int gvf_rast_sort_class_counts(const void* workspace, size_t workspace_bytes, int P, int F, int H, int W, int64_t max_rendered,
                                          uint32_t* counts_host, void* stream) {
    if (!workspace || !counts_host || H <= 0 || W <= 0 || P < 0 || F <= 0 || max_rendered < 0) return GVF_EINVAL;
    if ((((uintptr_t)workspace) & 255) != 0) return GVF_EINVAL;
    Workspace w = carve(const_cast<void*>(workspace), workspace_bytes, P, F, H, W, max_rendered);
    if (!w.ok) return GVF_ENOSPC;
    // test-only diagnostic.  The copy rides on the CALLER's stream (no blocking hipMemcpy on the legacy stream: that is illegal while another
    // host thread captures a hipGraph, the hazard utils/in_flight.py documents), then that stream is waited for.
    if (hipMemcpyAsync(counts_host, w.cls, 2 * sizeof(uint32_t), hipMemcpyDeviceToHost, (hipStream_t)stream) != hipSuccess) return GVF_ELAUNCH;
    if (hipStreamSynchronize((hipStream_t)stream) != hipSuccess) return GVF_ELAUNCH;
    return GVF_OK;
}

extern "C" const char* gvf_version(void) { return "gvf_hip 0.1.0 gfx950"; }
