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
//                                        instance culling, SH -> RGB; writes one 64-byte splat record + an 8- or 16-byte bin record
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
// This file: argument checks, the host pipeline (run_pipeline: a sequence of stages over the call plan of rast_plan.h), the workspace
// layout, the stage profiler and the C entry points; it holds no kernel.  Front end (every kernel in front of the per-tile sort, and the
// two functions that launch them): rast_front.hip; per-tile sort: rast_sort.hip; blend: rast_blend.hip; backward (R7): rast_bwd.hip; what
// they share: rast_common.h.
//
// HBM layout (caller-owned workspace, carved below): per (frame, Gaussian) ONE 64-byte, 64-byte-aligned record
//   float4 {x, y, conic_a, conic_b} | float4 {conic_c, opacity, r, g} | float4 {b, depth, hx, hy} | 16 B unused
// so the blend's gather of a (splat, tile) instance touches exactly one cache line (three 40-B-total arrays cost
// three lines per instance: 5.7 GB of fabric reads per 24-frame step measured with FETCH_SIZE, vs 1.1 GB
// algorithmic); hx, hy = half extents of the region where alpha can reach 1/255 (instance and quadrant culling),
// computed once per visible Gaussian.  A bin record (bucket binning): 8 bytes {x0|y0<<8|x1<<16|y1<<24, depth bits} when the
// tile grid is at most 255 x 255 (images up to 4080 px either way), else 16 bytes {x0|y0<<16, x1|y1<<16, depth bits, 0}; the array
// is carved at 16 bytes per record either way.  Per (frame, tile) a range, a counter and a cursor; per instance one u64 key and
// one u32 ordered id (radix path: u64 key + u32 id, double buffered).
#include <atomic>
#include <cstdlib>
#include <vector>
#include "rast_common.h"
#include "gvf_sort.h"

namespace {

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
// the events of this call, or null: not timed
const hipEvent_t* prof_take_slot() {
    const int slot = g_prof.on ? g_prof.calls.fetch_add(1) : -1;
    return slot >= 0 && slot < PROF_MAX_CALLS ? g_prof.ev[slot] : nullptr;
}

std::atomic<long long> g_shared_calls{0};

// The environment switches, read per call: tests flip them inside one process.  "0" switches a path off (measurement / test aids).
bool switch_on(const char* name) {
    const char* v = getenv(name);
    return !(v && v[0] == '0');
}
RastSwitches switches_from_env() {
    RastSwitches sw;
    sw.shared_act = switch_on("GVF_RAST_SHARED_ACT");
    sw.slot_order = switch_on("GVF_RAST_SLOT_ORDER");
    sw.pre_wave_frames = switch_on("GVF_RAST_PRE_WAVE_FRAMES");   // 0: the bucket-binning fused launch on the 256-Gaussian mapping
    sw.blend_order = switch_on("GVF_RAST_BLEND_ORDER");
    sw.bin_rec8 = switch_on("GVF_RAST_BIN_REC8");                 // 0: 16-byte bin records on every grid
    return sw;
}

int check_shape(const GvfRastSettings& st, int F, int P, int64_t max_rendered) {
    if (st.image_height <= 0 || st.image_width <= 0 || P < 0 || F <= 0 || max_rendered < 0 || max_rendered > 0xFFFFFFFFll) return GVF_EINVAL;
    if (st.sh_degree < 0 || st.sh_degree > 3) return GVF_EINVAL;
    if (st.mode != GVF_RAST_MODE_MIP && st.mode != GVF_RAST_MODE_DILATE) return GVF_EINVAL;
    return GVF_OK;
}

// where the frames go: fp32 colour (+ alpha, depth, either may be null) or uint8 frames (gvf_rast_forward_batched_u8), exactly one of the two
struct RastOutputs { float* color; float* alpha; float* depth; unsigned char* u8; };

int check_call(const RastCall& c, const RastOutputs& out, const void* workspace) {
    const GvfRastSettings& st = *c.st;
    if (check_shape(st, c.F, c.P, c.max_rendered) != GVF_OK) return GVF_EINVAL;
    if ((out.color == nullptr) == (out.u8 == nullptr) || !c.out_num_rendered || !c.frames_host || !workspace) return GVF_EINVAL;
    if (c.P > 0 && c.colors_precomp == nullptr) {
        if (c.sh == nullptr || c.M < (st.sh_degree + 1) * (st.sh_degree + 1) || c.M > MAX_SH_COEFFS) return GVF_EINVAL;
    }
    if ((((uintptr_t)c.sh) & 15) != 0 || (((uintptr_t)workspace) & 255) != 0) return GVF_EINVAL;  // 16-B SH rows, 256-B workspace
    return GVF_OK;
}

PlanInputs plan_inputs(const RastCall& c) {
    PlanInputs in;
    in.F = c.F; in.P = c.P; in.M = c.M; in.fused = c.fused;
    in.has_sh = c.sh != nullptr; in.has_colors_precomp = c.colors_precomp != nullptr; in.has_cov3D_precomp = c.cov3D_precomp != nullptr;
    in.has_delta = c.delta != nullptr; in.has_subpixel_offset = c.subpixel_offset != nullptr;
    in.max_rendered = c.max_rendered;
    return in;
}

// validate -> carve -> plan -> upload -> front end -> per-tile sort -> blend; everything stream-ordered, no host sync
int run_pipeline(const RastCall& c, void* workspace, size_t workspace_bytes, const RastOutputs& out, hipStream_t stream) {
    int rc = check_call(c, out, workspace);
    if (rc != GVF_OK) return rc;
    // hipGetLastError() is process-wide: clear what other users of the runtime (e.g. an event query that
    // returned hipErrorNotReady) left behind, so GVF_CHECK_LAUNCH reports only this call's launches.
    (void)hipGetLastError();
    const GvfRastSettings& st = *c.st;
    const Workspace w = carve(workspace, workspace_bytes, c.P, c.F, st.image_height, st.image_width, c.max_rendered);
    if (!w.ok) return GVF_ENOSPC;
    const RastPlan plan = plan_call(st, c.frames_host, plan_inputs(c), switches_from_env());
    const hipEvent_t* marks = prof_take_slot();
    if ((rc = upload_frames(stream, c, plan, w)) != GVF_OK) return rc;

    if (c.P == 0) {
        // nothing to splat: background only
        if (hipMemsetAsync(c.out_num_rendered, 0, sizeof(uint32_t) * c.F, stream) != hipSuccess) return GVF_ELAUNCH;
    } else {
        uint64_t* keys = w.keys;          // the tile segments: (depth bits << 32 | id), unsorted inside a segment
        uint32_t* vals = nullptr;         // radix binning: the ids travel beside the keys
        if (plan.shared) g_shared_calls.fetch_add(1, std::memory_order_relaxed);
        rc = plan.bucket ? front_end_bucket(stream, c, plan, w, marks) : front_end_radix(stream, c, plan, w, marks, &keys, &vals);
        if (rc != GVF_OK) return rc;
        // per-tile on-chip sort by (depth, id)
        if (c.max_rendered > 0 &&
            (rc = launch_tile_sort(stream, w.ranges, keys, vals, w.ids, w.cls, (uint32_t)plan.nseg, plan.bucket ? 2 : 1)) != GVF_OK)
            return rc;
    }
    // slot order: the blend looks up where a Gaussian's record sits inside a frame (w.order_alt).  order_tiles: heaviest tiles first
    // (blend_order_kernel; the scatter pass is done with its cursors: their array takes the order)
    rc = launch_blend(stream, st, c.P, c.F, w.ranges, w.ids, w.splats, c.subpixel_offset, out.color, out.alpha, out.depth, out.u8,
                      plan.slot_mode ? w.order_alt : nullptr, plan.order_tiles ? w.cursor : nullptr, marks != nullptr ? marks[6] : nullptr);
    if (rc != GVF_OK) return rc;
    prof_mark(stream, marks, 7);
    return GVF_OK;
}

// the argument checks of the two batched forward entry points
int check_batched(const GvfRastSettings* st, const GvfRastFrame* frames_host, int F, const GvfGaussianActivation* act, int P,
                  const float* xyz_raw, const float* features_dc, const float* scaling_raw, const float* rotation_raw,
                  const float* opacity_raw, const float* delta, int n_delta) {
    if (!st || !frames_host || !act || F <= 0) return GVF_EINVAL;
    if (P > 0 && (!xyz_raw || !features_dc || !scaling_raw || !rotation_raw || !opacity_raw)) return GVF_EINVAL;
    if (act->scaling_activation != 0 && act->scaling_activation != 1) return GVF_EINVAL;
    for (int f = 0; f < F; ++f) {
        int di = frames_host[f].delta_index;
        if (di >= 0 && (delta == nullptr || di >= n_delta)) return GVF_EINVAL;
    }
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
    w.mhist = c.take<uint32_t>(MORTON_BINS);
    w.mm = c.take<uint32_t>(8);
    w.binrec = c.take<uint4>(FP);           // 16 bytes per record whichever form the call's plan takes (the layout does not depend on it)
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
    const RastCall c = {st, frame_host, 1, P, M, false, nullptr, means3D, scales, rotations, opacities, shs, colors_precomp, cov3D_precomp,
                        nullptr, 0, subpixel_offset, max_rendered, out_radii, out_num_rendered};
    return run_pipeline(c, workspace, workspace_bytes, {out_color, out_alpha, out_depth, nullptr}, (hipStream_t)stream);
}

extern "C" int gvf_rast_forward_batched(const GvfRastSettings* st, const GvfRastFrame* frames_host, int F,
                                        const GvfGaussianActivation* act, int P, int M, const float* xyz_raw,
                                        const float* features_dc, const float* scaling_raw,
                                        const float* rotation_raw, const float* opacity_raw, const float* delta,
                                        int n_delta, void* workspace, size_t workspace_bytes,
                                        int64_t max_rendered, float* out_color, float* out_alpha, float* out_depth,
                                        int32_t* out_radii, uint32_t* out_num_rendered, void* stream) {
    const int rc = check_batched(st, frames_host, F, act, P, xyz_raw, features_dc, scaling_raw, rotation_raw, opacity_raw, delta, n_delta);
    if (rc != GVF_OK) return rc;
    const RastCall c = {st, frames_host, F, P, M, true, act, xyz_raw, scaling_raw, rotation_raw, opacity_raw, features_dc, nullptr, nullptr,
                        delta, n_delta, nullptr, max_rendered, out_radii, out_num_rendered};
    return run_pipeline(c, workspace, workspace_bytes, {out_color, out_alpha, out_depth, nullptr}, (hipStream_t)stream);
}

// the batched call with the frames leaving as uint8 (the reference's post-process, utils/inference_utils.py:280-286, in the blend's epilogue)
extern "C" int gvf_rast_forward_batched_u8(const GvfRastSettings* st, const GvfRastFrame* frames_host, int F,
                                           const GvfGaussianActivation* act, int P, int M, const float* xyz_raw,
                                           const float* features_dc, const float* scaling_raw,
                                           const float* rotation_raw, const float* opacity_raw, const float* delta,
                                           int n_delta, void* workspace, size_t workspace_bytes,
                                           int64_t max_rendered, uint8_t* out_rgb_u8, uint32_t* out_num_rendered, void* stream) {
    if (!out_rgb_u8) return GVF_EINVAL;
    const int rc = check_batched(st, frames_host, F, act, P, xyz_raw, features_dc, scaling_raw, rotation_raw, opacity_raw, delta, n_delta);
    if (rc != GVF_OK) return rc;
    const RastCall c = {st, frames_host, F, P, M, true, act, xyz_raw, scaling_raw, rotation_raw, opacity_raw, features_dc, nullptr, nullptr,
                        delta, n_delta, nullptr, max_rendered, nullptr, out_num_rendered};
    return run_pipeline(c, workspace, workspace_bytes, {nullptr, nullptr, nullptr, out_rgb_u8}, (hipStream_t)stream);
}

// test-only diagnostic: the plan of a call with these arguments, through the forward's own plan_call and switches; no launch
extern "C" int gvf_rast_call_plan(const GvfRastSettings* st, const GvfRastFrame* frames_host, int F, int P, int M, int fused, int has_sh,
                                  int has_colors_precomp, int has_cov3D_precomp, int has_delta, int has_subpixel_offset,
                                  int64_t max_rendered, GvfRastPlan* out) {
    if (!st || !frames_host || !out || M < 0) return GVF_EINVAL;
    if (check_shape(*st, F, P, max_rendered) != GVF_OK) return GVF_EINVAL;
    PlanInputs in;
    in.F = F; in.P = P; in.M = M; in.fused = fused != 0;
    in.has_sh = has_sh != 0; in.has_colors_precomp = has_colors_precomp != 0; in.has_cov3D_precomp = has_cov3D_precomp != 0;
    in.has_delta = has_delta != 0; in.has_subpixel_offset = has_subpixel_offset != 0;
    in.max_rendered = max_rendered;
    *out = plan_call(*st, frames_host, in, switches_from_env());   // (the public part of the plan)
    return GVF_OK;
}

// test-only diagnostic: the bin-record form a call with these settings takes (the private part of the plan), through the forward's own
// plan_call and switches; the form does not depend on the Gaussians or the frames, so the plan is that of one frame without Gaussians
extern "C" int gvf_rast_bin_record_bytes(const GvfRastSettings* st, int* bytes) {
    if (!st || !bytes) return GVF_EINVAL;
    if (check_shape(*st, 1, 0, 0) != GVF_OK) return GVF_EINVAL;
    const GvfRastFrame frame = {};
    PlanInputs in = {};
    in.F = 1;
    *bytes = plan_call(*st, &frame, in, switches_from_env()).rec8 ? 8 : 16;
    return GVF_OK;
}

// test-only diagnostic: the slice grouping the plan and the batched backward share, as the backward's table
extern "C" int gvf_rast_slice_groups(const GvfRastFrame* frames_host, int F, int has_delta, int max_slices, int32_t* table_host,
                                     int* n_slices) {
    if (!frames_host || !table_host || !n_slices || F <= 0) return GVF_EINVAL;
    std::vector<int32_t> slices, frame_slice;
    if (!group_slices(frames_host, F, has_delta != 0, max_slices, slices, frame_slice)) return GVF_ENOSPC;
    const std::vector<int32_t> tab = slice_table(slices, frame_slice);
    for (size_t k = 0; k < tab.size(); ++k) table_host[k] = tab[k];
    *n_slices = (int)slices.size();
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
