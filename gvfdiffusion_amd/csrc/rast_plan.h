// rast_plan.h -- what a rasteriser call decides on the host before its first launch: the tile grid, the delta-slice table, the path flags,
// the record layout and the grids / dynamic-LDS sizes of the launches whose shape depends on the path.  Plain C++ (no HIP, no environment
// reads, no process state): plan_call is a pure function of its arguments, gvf_rast_call_plan hands its result to the host tests
// (tests/test_rast_plan_host.py pins the table below), run_pipeline (rast.hip) and the two front ends (rast_front.hip) launch from it.
#pragma once
#include <cstddef>
#include <cstdint>
#include <vector>
#include "../../include/gvf_rast.h"

namespace gvf_rast {

// ---- launch-shape constants the plan shares with the front-end kernels (rast_front.hip) ----
constexpr int TILE = GVF_TILE;
constexpr int WAVE = 64;
constexpr int PRE_THREADS = 256;
#ifndef GVF_PRE_FB                       // (a variant build passes it, and GVF_PRE_WAVE_FB, to rast.hip AND rast_front.hip)
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
constexpr int PRE_WAVES = PRE_THREADS / WAVE;
constexpr int PRE_WAVE_FB = GVF_PRE_WAVE_FB;
constexpr int ACT_MAX_SLICES = 16;       // delta slices of a shared-activation call (activate_cov_kernel takes their table as an argument)
constexpr int SCAN_CHUNK = 4096;         // counters per block of seg_sums_kernel / seg_scan_kernel
constexpr int BIN_SPT = 4;               // bin_kernel: slots per thread
constexpr int BIN_SLOTS = PRE_THREADS * BIN_SPT;
constexpr int BINX_TAB = 4096;           // bin_index_kernel: tiles of its whole-frame LDS table
constexpr int BINX_PER_WG = 8192;        //                   Gaussians per workgroup
constexpr int BIN_REC8_MAX_GRID = 255;   // 8-byte bin records: a rect coordinate lies in [0, gx] or [0, gy] and gets 8 bits
constexpr int MORTON_BINS = 1 << 15;
constexpr int ORDER_TILES_MIN_SEGS = 2048;   // heaviest-tiles-first blend: worth a launch when the frames' workgroups outnumber the chip's resident slots

// The record layout a forward call chose, kept in a workspace word (mm[LAYOUT_WORD], beside the bounding box) for the backward of that
// call, which reads it on the device: the plan's decision is not made a second time, and no host read is needed (capture-safe).
//   bit 0 (LAYOUT_SLOT_ORDER): splat records of a frame sit at the Gaussians' Morton slots, rec = order_alt[id] (blend_rec_of); else rec = id
constexpr int LAYOUT_WORD = 6;
constexpr uint32_t LAYOUT_SLOT_ORDER = 1u;

// ---- delta slices ----
// The frames' delta slices in order of first use: slices[k] = the k-th distinct delta index, frame_slice[f] = the k of frame f.  A frame
// without a delta (no delta tensor, or delta_index < 0) is slice -1.  cap > 0: at most that many distinct slices -- false at the first frame
// that needs one more (slices then holds the first `cap`, frame_slice is filled up to that frame); cap <= 0: no limit.
inline bool group_slices(const GvfRastFrame* frames_host, int F, bool has_delta, int cap, std::vector<int32_t>& slices,
                         std::vector<int32_t>& frame_slice) {
    slices.clear();
    frame_slice.assign((size_t)(F > 0 ? F : 0), 0);
    for (int f = 0; f < F; ++f) {
        const int32_t di = (has_delta && frames_host[f].delta_index >= 0) ? frames_host[f].delta_index : -1;
        size_t k = 0;
        while (k < slices.size() && slices[k] != di) ++k;
        if (k == slices.size()) {
            if (cap > 0 && (int)slices.size() == cap) return false;
            slices.push_back(di);
        }
        frame_slice[(size_t)f] = (int32_t)k;
    }
    return true;
}

// The grouping as the table the batched backward uploads: [F] frame indices grouped by slice (frames ascending inside a slice) |
// [ns + 1] group starts | [ns] the slices' delta indices.
inline std::vector<int32_t> slice_table(const std::vector<int32_t>& slices, const std::vector<int32_t>& frame_slice) {
    const size_t F = frame_slice.size(), ns = slices.size();
    std::vector<int32_t> tab, starts;
    tab.reserve(F + 2 * ns + 1);
    for (size_t k = 0; k < ns; ++k) {
        starts.push_back((int32_t)tab.size());
        for (size_t f = 0; f < F; ++f)
            if (frame_slice[f] == (int32_t)k) tab.push_back((int32_t)f);
    }
    starts.push_back((int32_t)tab.size());
    tab.insert(tab.end(), starts.begin(), starts.end());
    tab.insert(tab.end(), slices.begin(), slices.end());
    return tab;
}

// ---- the plan ----
// The environment switches of a call ("0" switches a path off; anything else, or unset, leaves it on).  plan_call does not read the
// environment: the caller does, once per call (tests flip the variables inside one process).
struct RastSwitches {
    bool shared_act = true;          // GVF_RAST_SHARED_ACT
    bool slot_order = true;          // GVF_RAST_SLOT_ORDER
    bool pre_wave_frames = true;     // GVF_RAST_PRE_WAVE_FRAMES
    bool blend_order = true;         // GVF_RAST_BLEND_ORDER
    bool bin_rec8 = true;            // GVF_RAST_BIN_REC8
};

// What of a call's arguments the plan depends on (pointers only as present / absent)
struct PlanInputs {
    int F, P, M;
    bool fused, has_sh, has_colors_precomp, has_cov3D_precomp, has_delta, has_subpixel_offset;
    int64_t max_rendered;
};

// The public part (flags, sizes, grids, LDS bytes: include/gvf_rast.h) + the slice table the front end and the upload launch need and the
// bin-record form (gvf_rast_bin_record_bytes shows it to the tests).
struct RastPlan : GvfRastPlan {
    int32_t di[ACT_MAX_SLICES];            // delta index of each slice (shared activation)
    std::vector<int32_t> frame_slice;      // [F]: the frame's slice; all zero unless `shared` (goes to the device copy's reserved[0])
    bool rec8;                             // bin records in the 8-byte form (BinRec8, rast_common.h) instead of the 16-byte one
};

inline int ceil_div(int a, int b) { return (a + b - 1) / b; }
inline int pre_lds_bytes(int rows, int M) { return (int)(((size_t)rows * M * 3 * sizeof(float) + 15) / 16 * 16 + 16); }   // SH rows + 4 wave sums

inline RastPlan plan_call(const GvfRastSettings& st, const GvfRastFrame* frames_host, const PlanInputs& in, const RastSwitches& sw) {
    RastPlan p = {};
    const int F = in.F, P = in.P;
    const size_t room = (size_t)(in.max_rendered > 0 ? in.max_rendered : 0) * 8u;   // bytes of keys_alt, which only the radix binning uses
    p.gx = ceil_div(st.image_width, TILE); p.gy = ceil_div(st.image_height, TILE); p.ntiles = p.gx * p.gy;
    p.nb = ceil_div(P, PRE_THREADS);
    p.nseg = (int32_t)((size_t)F * p.ntiles);
    p.bucket = st.bin_algo != GVF_RAST_BIN_RADIX;
    // per-pixel sub-pixel offsets move the sample positions: no box culling then (as in the blend)
    p.upstream_binning = st.upstream_binning != 0 || in.has_subpixel_offset;

    // shared activation (activate_cov_kernel): the call's distinct delta slices, if they are few, once per (slice, Gaussian) instead of once
    // per frame.  Worth it from two frames per slice on; the records (64 bytes each) must fit into keys_alt -- a sizing call with
    // max_rendered = 0 takes the fused path, whose outputs are the same bits.
    std::vector<int32_t> slices;
    const bool few = group_slices(frames_host, F, in.has_delta, ACT_MAX_SLICES, slices, p.frame_slice);
    p.n_slices = (int32_t)slices.size();
    for (size_t k = 0; k < slices.size(); ++k) p.di[k] = slices[k];
    const size_t rec_bytes = (size_t)p.n_slices * (size_t)P * 64u;
    p.shared = sw.shared_act && in.fused && !in.has_cov3D_precomp && p.bucket && P > 0 && F >= 2 && few && F >= 2 * p.n_slices &&
               rec_bytes <= room;
    if (!p.shared) p.frame_slice.assign((size_t)F, 0);

    // bucket binning without shared activation: bin_index_kernel takes the count pass when a frame's tiles fit its table
    p.index_count = p.bucket && !p.shared && p.ntiles <= BINX_TAB;
    // spatial (Morton) order of the Gaussians: bucket binning, several frames to amortise it over
    p.morton = p.bucket && F >= 4 && P >= 4096;
    // slot order of the shared-activation path (see activate_cov_kernel): needs the Morton order, SH input and room for the slot-ordered SH
    // copy behind the records
    const int M = in.has_colors_precomp ? 0 : in.M;
    p.slot_mode = p.shared && sw.slot_order && p.morton && p.nb > 0 && !in.has_colors_precomp && in.has_sh &&
                  rec_bytes + (size_t)P * (size_t)M * 3u * 4u <= room;
    p.layout = p.slot_mode ? LAYOUT_SLOT_ORDER : 0u;
    // preprocess_kernel<false> stores the bin records at the Gaussians' indices, bin_kernel gathers them in Morton order
    p.rec_gather = p.bucket && !p.shared && p.morton;
    p.wave_frames = !p.shared && p.bucket && sw.pre_wave_frames;
    // 8-byte bin records (half the bytes through preprocess's stores and both bin passes; a frame's records then fit one XCD's L2 in the
    // gather): every coordinate of a tile rect must fit 8 bits.  Larger grids (images beyond 4080 px) keep the 16-byte form.
    p.rec8 = p.bucket && sw.bin_rec8 && p.gx <= BIN_REC8_MAX_GRID && p.gy <= BIN_REC8_MAX_GRID;
    p.order_tiles = sw.blend_order && P > 0 && p.nb > 0 && in.max_rendered > 0 && (size_t)F * p.ntiles >= (size_t)ORDER_TILES_MIN_SEGS;

    p.pre_grid[0] = p.nb; p.pre_grid[1] = ceil_div(F, PRE_FB);
    p.wf_grid[0] = ceil_div(P, WAVE); p.wf_grid[1] = ceil_div(F, PRE_WAVES * PRE_WAVE_FB);
    p.pre_lds_bytes = pre_lds_bytes(PRE_THREADS, M);
    p.wf_lds_bytes = pre_lds_bytes(WAVE, M);
    // bin passes: (blocks of BIN_SLOTS slots, F), or 1-D with each XCD taking whole frames (groups of 8) under rec_gather
    const int bnb = ceil_div(P, BIN_SLOTS);
    p.bin_grid[0] = p.rec_gather ? ceil_div(F, 8) * 8 * bnb : bnb; p.bin_grid[1] = p.rec_gather ? 1 : F;
    p.binx_grid[0] = ceil_div(P, BINX_PER_WG); p.binx_grid[1] = F;
    p.scan_blocks = (int32_t)(((size_t)p.nseg + SCAN_CHUNK - 1) / SCAN_CHUNK);
    // the upload launch clears the tile ranges (2 words per segment), the tile counters and, for the Morton order, its histogram
    const size_t clear_words = 2 * (size_t)p.nseg + (size_t)p.nseg + (p.morton ? (size_t)MORTON_BINS : 0u);
    const size_t clear_blocks = (clear_words + 4095) / 4096;
    p.clear_blocks = (int32_t)(clear_blocks < 256 ? clear_blocks : 256);
    return p;
}

}  // namespace gvf_rast
