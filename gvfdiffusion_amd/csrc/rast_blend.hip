// rast_blend.hip -- the rasteriser's blend: the sorted tile segments composited into frames, and the uint8 post-process.  rast.hip has the
// pipeline around it.
#include "rast_common.h"

namespace {

// ---------------------------------------------------------------------------------------------
// R6: blend
// ---------------------------------------------------------------------------------------------
// One workgroup per 16x16 tile, as upstream's renderCUDA, but the 4 waves own the four 8x8 QUADRANTS of
// the tile and each wave only walks the splats that can reach its quadrant:
//   * the thread that stages splat j of a 256-splat batch into LDS also computes a 4-bit quadrant mask from
//     the axis-aligned bounding box of the region where alpha = opacity * exp(power) can reach 1/255
//     ( ca dx^2 + 2 cb dx dy + cc dy^2 <= 2 ln(255 opacity) ), inflated so that float noise can only keep
//     extra splats, never drop one: the list only decides WHICH (splat, quadrant) pairs are evaluated -- a culled pair
//     would have failed the alpha < 1/255 test at every pixel of the quadrant, so the image does not depend on it.
//     A kept splat is evaluated by splat_neg_exponent below, which is NOT upstream's expression since round 4:
//     upstream forms  power = -0.5 (A dx^2 + C dy^2) - B dx dy  from the pixel offsets and the conic, tests
//     power > 0, and takes  alpha = min(0.99, opacity * exp(power));  here the exponent comes from the Cholesky
//     factor of the scaled conic in tile-relative coordinates with log2(opacity) folded in,
//         alpha = min(0.99, exp2(lo - s1^2 - s2^2)),  s1 = c1 - l11 px - l12 py,  s2 = c2 - l22 py,
//     i.e. the same quadratic evaluated in another order (~1e-5 of the exponent apart: the cancellation in c - l p
//     over a tile's 16 pixels), with no `power > 0` case of its own (a sum of squares cannot come out positive;
//     upstream's test only fires on rounding noise at the centre of a valid splat) and with a conic that is not
//     positive definite dropped (opacity staged as 0) where upstream composites the indefinite form; the
//     transmittance update is  T - alpha T  (one fma) for upstream's  T (1 - alpha).  Every one of these stands
//     between this kernel and the published arithmetic only through oracle/rast_oracle.c, which keeps upstream's
//     forms: images agree to ~4e-7 except at pixels where a decision sits within that noise of its threshold
//     (flagged by the oracle);
//   * each wave compacts the batch into its own index list with wave64 ballots (order preserved = depth
//     order) and iterates over that list only.  A typical splat (3-sigma radius ~9 px) reaches ~40 % of the
//     quadrants of the tiles it was binned to, so ~60 % of upstream's (pixel, splat) evaluations disappear.
// Early termination is per wave (all 64 pixels saturated) and per workgroup (stop staging).

// Dispatch order of blend_kernel inside a frame: heaviest tiles first.  A workgroup's life is proportional to its tile's instance count
// (1 k .. 150 k cycles at the bench shape); in image order the heavy centre tiles of the LAST frame start late and the chip drains behind them:
// list scheduling of the measured workgroup durations on the 2048 resident slots puts the image order 5.7 % above sum / slots and
// heaviest-first 0.1-0.9 % above (scripts/blend_stamps.py, profiles/r05_blend_phase_stamps.txt).  One workgroup per frame: counting sort of the
// tiles by count class (64 classes of 32 instances, class 0 = 2016 and more; the order inside a class is whatever the atomics give -- tiles of a
// class are neighbours in the image anyway, so the splat records stay shared in L2).  Images do not depend on the order.
// Measured (profiles/r05_blend_order_ab.txt): the reference's live render job (512 x 512, tiles of up to 16 k instances beside empty ones) 167-176 ->
// 146-149 ms per sample; the bench shape (800 x 800, no tile above 2048) unchanged within noise -- there image order already mixes heavy (vector-pipe)
// and light (latency) workgroups on every CU.  So a frame is reordered only if it holds a tile of the top class.
__global__ __launch_bounds__(1024) void blend_order_kernel(const uint2* __restrict__ ranges, int ntiles, uint32_t* __restrict__ order) {
    __shared__ uint32_t hist[64];
    const int f = blockIdx.x, t = threadIdx.x;
    const uint2* r = ranges + (size_t)f * ntiles;
    if (t < 64) hist[t] = 0u;
    __syncthreads();
    for (int tile = t; tile < ntiles; tile += 1024) {
        const uint32_t n = r[tile].y - r[tile].x;
        atomicAdd(&hist[63u - min(63u, n >> 5)], 1u);
    }
    __syncthreads();
    const bool reorder = hist[0] != 0u;                // a tile in the top class (>= 2016 instances)?  Read by everyone BEFORE thread 0's scan overwrites it
    __syncthreads();
    if (!reorder) {                                    // image order
        for (int tile = t; tile < ntiles; tile += 1024) order[(size_t)f * ntiles + tile] = (uint32_t)tile;
        return;
    }
    if (t == 0) {
        uint32_t run = 0u;
        for (int c = 0; c < 64; ++c) { const uint32_t h = hist[c]; hist[c] = run; run += h; }
    }
    __syncthreads();
    for (int tile = t; tile < ntiles; tile += 1024) {
        const uint32_t n = r[tile].y - r[tile].x;
        order[(size_t)f * ntiles + atomicAdd(&hist[63u - min(63u, n >> 5)], 1u)] = (uint32_t)tile;
    }
}

#ifdef BLEND_TIMING
// timing builds only (scripts/blend_stamps.py, a variant library): wave-cycles per phase of blend_kernel, summed over every wave of a launch
//   [0] wait at the round's first barrier  [1] id load  [2] record gather  [3] Cholesky + quadrant mask + LDS writes  [4] wait at the second barrier
//   [5] list compaction  [6] compositing  [7] rounds  [8] list entries  [9] waves  [10] whole wave lifetime  [11] epilogue stores
__device__ unsigned long long* g_blend_buf;       // [waves of the launch][12], one row per wave (same-address atomics would serialise the launch)
__device__ unsigned long long g_blend_cap;
extern "C" int gvf_debug_blend_timing(unsigned long long* device_buf, unsigned long long rows) {
    if (hipMemcpyToSymbol(HIP_SYMBOL(g_blend_buf), &device_buf, sizeof(device_buf)) != hipSuccess) return 1;
    if (hipMemcpyToSymbol(HIP_SYMBOL(g_blend_cap), &rows, sizeof(rows)) != hipSuccess) return 1;
    return 0;
}
#define BT_DECL unsigned long long bt_acc[12] = {}; unsigned long long bt_last = __builtin_amdgcn_s_memtime(); const unsigned long long bt_first = bt_last;
#define BT(i) do { const unsigned long long n_ = __builtin_amdgcn_s_memtime(); bt_acc[i] += n_ - bt_last; bt_last = n_; } while (0)
#define BT_VMWAIT() asm volatile("s_waitcnt vmcnt(0)" ::: "memory")
#else
#define BT_DECL
#define BT(i) do { } while (0)
#define BT_VMWAIT() do { } while (0)
#endif

#ifdef BLEND_CONSUMED
// counting builds only (scripts/blend_consumed.py, a variant library): per size class of a (frame, tile) segment -- <= 2048 keys, <= 4096, <= 16384,
// more -- [segments, keys sorted, keys the compositing had staged when every pixel of the tile was saturated (whole 256-key rounds)]: how much of
// the per-tile sort's work the blend ever looks at
__device__ unsigned long long g_blend_cons[4][5];   // + [staged keys whose quadrant mask is 0, sum of the masks' bit counts]
extern "C" int gvf_debug_blend_consumed(unsigned long long* out12, int reset) {
    if (out12 && hipMemcpyFromSymbol(out12, HIP_SYMBOL(g_blend_cons), sizeof(g_blend_cons)) != hipSuccess) return 1;
    if (reset) { unsigned long long z[20] = {}; if (hipMemcpyToSymbol(HIP_SYMBOL(g_blend_cons), z, sizeof(z)) != hipSuccess) return 1; }
    return 0;
}
#endif

// The pixel's "done" flag of blend_kernel (outside the image, or saturated) lives as the wave's 64-bit LANE MASK done_m, and the predicates of
// the compositing step are scalar operations on lane masks (ballot / inverse ballot); all 64 lanes are active, workgroups are whole.  A per-lane
// bool costs one scalar instruction more per list entry and a vector rebuild of the flag per __all(): 41.4 against 38.9 ticks per list entry per
// SIMD in the loop alone (profiles/r06_ubench_blend_step.txt, r06_blend_lane_masks_ab.txt), bit-identical images.  The fence between the two
// pairs of a trip keeps the second pair's LDS reads behind the first pair's arithmetic: without it the scheduler requests all four entries'
// records at once -- 68 vector registers, seven waves per SIMD instead of eight.

// DEPTH: accumulate the depth channel (diff_gauss outputs; one fma per evaluated splat that the mip path does not pay)
template <bool DEPTH>
__global__ __launch_bounds__(BLEND_THREADS) void blend_kernel(
    int P, int H, int W, int gx, int gy, float bg0, float bg1, float bg2, const uint2* __restrict__ ranges,
    const uint32_t* __restrict__ point_list, const float4* __restrict__ splats,
    const float* __restrict__ subpixel_offset, float* __restrict__ out_color,
    float* __restrict__ out_alpha, float* __restrict__ out_depth,
    const uint32_t* __restrict__ tile_order /* [F][tiles]: workgroup blockIdx.x of frame f takes tile tile_order[f][blockIdx.x]; null = identity */,
    const uint32_t* __restrict__ rec_of /* Gaussian id -> index of its splat record inside a frame (slot order); null = the id itself */,
    unsigned char* __restrict__ out_u8 /* non-null: the frames leave as uint8 [F][3][H][W] = clamp(rgb, 0, 1) * 255 truncated (C1's post-process,
                                          rgb_to_u8_kernel's arithmetic on the same float) and out_color is not written */) {
    __shared__ float4 sA[BLEND_THREADS];
    __shared__ float4 sB[BLEND_THREADS];
    __shared__ float4 sC[BLEND_THREADS];                  // {b, depth, -, -}: 16-byte stride like sA / sB, one index shift per splat
    __shared__ unsigned char sMask[BLEND_THREADS];
    // per-wave compacted list of the batch: the BYTE OFFSET (16 x index) of each kept splat's records, one dword each -- four entries are one
    // ds_read_b128 whose registers ARE the addresses of the record reads (as byte indices they cost an extract-and-shift per compositing step)
    __shared__ unsigned sList[4][BLEND_THREADS];

    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int f = blockIdx.y;
    const int tile = tile_order != nullptr ? (int)tile_order[(size_t)f * gridDim.x + blockIdx.x] : (int)blockIdx.x;
    const int tx = tile % gx, ty = tile / gx;
    const int px = tx * TILE + (wave & 1) * 8 + (lane & 7), py = ty * TILE + (wave >> 1) * 8 + (lane >> 3);
    const bool inside = px < W && py < H;
    const size_t pid = (size_t)py * W + px;
    float pxf = (float)px, pyf = (float)py;
    if (subpixel_offset != nullptr && inside) { pxf += subpixel_offset[2 * pid]; pyf += subpixel_offset[2 * pid + 1]; }

    const uint2 rng = ranges[(size_t)f * gx * gy + tile];
    const size_t gbase = (size_t)f * P;
    const int rounds = (int)((rng.y - rng.x + BLEND_THREADS - 1) / BLEND_THREADS);
    int todo = (int)(rng.y - rng.x);
    const uint64_t lt_mask = (1ull << lane) - 1ull;

    const float pxr = pxf - (float)(tx * TILE), pyr = pyf - (float)(ty * TILE);      // tile-relative (exact: small integers + the sub-pixel offset)
    unsigned long long done_m = __builtin_amdgcn_ballot_w64(!inside);
    float T = 1.0f, C0 = 0.f, C1 = 0.f, C2 = 0.f, Dacc = 0.f;

    BT_DECL
#ifdef BLEND_CONSUMED
    int rounds_done = rounds;
#endif
    for (int r = 0; r < rounds; ++r, todo -= BLEND_THREADS) {
        BT(6);
        // (r > 0: before the first round no pixel inside the image is saturated and nothing in LDS has to be protected from a previous round;
        //  the reduction's LDS round trip and barriers are ~1 % of a wave's life at 1.17 rounds per tile, profiles/r06_blend_lane_masks_ab.txt)
#ifdef BLEND_CONSUMED
        if (r > 0 && __syncthreads_and(done_m == ~0ull)) { rounds_done = r; break; }
#else
        if (r > 0 && __syncthreads_and(done_m == ~0ull)) break;
#endif
        BT(0);
#ifdef BLEND_TIMING
        uint32_t id_ = 0;
        if (t < todo) id_ = point_list[rng.x + (uint32_t)r * BLEND_THREADS + t];
        if (t < todo && rec_of != nullptr) id_ = rec_of[id_];
        BT_VMWAIT(); BT(1);
        float4 a_ = {}, b_ = {}, c_ = {};
        if (t < todo) { const float4* rec = splats + 4 * (gbase + id_); a_ = rec[0]; c_ = rec[2]; b_ = rec[1]; }
        BT_VMWAIT(); BT(2);
        bt_acc[7] += 1;
#endif
        if (t < todo) {
#ifdef BLEND_TIMING
            const float4 a = a_, b = b_, c = c_;
#else
            uint32_t id = point_list[rng.x + (uint32_t)r * BLEND_THREADS + t];
            if (rec_of != nullptr) id = rec_of[id];          // (a 1 MB table, L2-resident; the sorted lists keep Gaussian ids: ties break by index)
            const float4* rec = splats + 4 * (gbase + id);
            const float4 a = rec[0];
            const float4 c = rec[2];
            const float4 b = rec[1];
#endif
            const SplatChol ch = splat_cholesky(a.x, a.y, a.z, a.w, b.x, (float)(tx * TILE), (float)(ty * TILE));
            sA[t] = make_float4(ch.l11, ch.l12, ch.l22, ch.c1);
            sB[t] = make_float4(ch.c2, ch.ok ? __builtin_amdgcn_logf(b.y) : -__builtin_inff(), b.z, b.w);       // log2(opacity)
            sC[t] = make_float4(c.x, c.y, 0.f, 0.f);
            sMask[t] = (unsigned char)quadrant_mask(a.x, a.y, a.z, a.w, b.x, b.y, c.z, (float)(tx * TILE), (float)(ty * TILE), subpixel_offset != nullptr);
#ifdef BLEND_CONSUMED
            {
                const unsigned n_ = rng.y - rng.x;
                const int cls_ = n_ <= 2048u ? 0 : n_ <= 4096u ? 1 : n_ <= 16384u ? 2 : 3;
                if (sMask[t] == 0) atomicAdd(&g_blend_cons[cls_][3], 1ull);
                atomicAdd(&g_blend_cons[cls_][4], (unsigned long long)__popc((unsigned)sMask[t]));
            }
#endif
        }
        BT(3);
        __syncthreads();
        BT(4);
        const int cnt = min(BLEND_THREADS, todo);
        if (done_m == ~0ull) continue;                    // this quadrant is saturated (wave-uniform)
        // compact the batch into this wave's list (ascending index = depth order)
        int n_w = 0;
#pragma unroll
        for (int k = 0; k < BLEND_THREADS / GVF_WAVE; ++k) {
            const int idx = k * GVF_WAVE + lane;
            const bool hit = idx < cnt && ((sMask[idx] >> wave) & 1u);
            const uint64_t bal = __ballot(hit);
            if (hit) sList[wave][n_w + __popcll(bal & lt_mask)] = (unsigned)idx * 16u;
            n_w += __popcll(bal);
        }
        __builtin_amdgcn_wave_barrier();
        BT(5);
#ifdef BLEND_TIMING
        bt_acc[8] += n_w;
#endif
        // Branch-free compositing step (upstream's `continue`s become predicates: a skipped splat gets weight 0,
        // which leaves C and T bit-identical), two splats per trip so that the second one's LDS reads and alpha
        // arithmetic overlap the first one's serial T update.
#define GVF_BLEND_STEP(J)                                                                              \
        {                                                                                              \
            const float4 a = *reinterpret_cast<const float4*>(reinterpret_cast<const unsigned char*>(sA) + (J));          \
            const float4 b = *reinterpret_cast<const float4*>(reinterpret_cast<const unsigned char*>(sB) + (J));          \
            const float4 c4_ = *reinterpret_cast<const float4*>(reinterpret_cast<const unsigned char*>(sC) + (J));        \
            const float2 c = DEPTH ? make_float2(c4_.x, c4_.y) : make_float2(c4_.x, 0.f);              \
            const float nlog = splat_neg_exponent(a.x, a.y, a.z, a.w, b.x, pxr, pyr, b.y);   /* -log2(opacity * G) */ \
            const float alpha = fminf(0.99f, __builtin_amdgcn_exp2f(-nlog));                           \
            const float w_raw = alpha * T;                                                             \
            const float test_T = T - w_raw;        /* = T (1 - alpha) up to one rounding; one op less */ \
            /* ok = !done && !(alpha < 1/255); stop = ok && test_T < 1e-4; done |= stop; acc = ok && !stop */                  \
            const unsigned long long ok_m = __builtin_amdgcn_ballot_w64(!(alpha < 1.0f / 255.0f)) & ~done_m;   \
            const unsigned long long stop_m = ok_m & __builtin_amdgcn_ballot_w64(test_T < 0.0001f);    \
            done_m |= stop_m;                                                                          \
            const bool acc = __builtin_amdgcn_inverse_ballot_w64(ok_m ^ stop_m);                       \
            const float wgt = acc ? w_raw : 0.0f;                                                      \
            C0 = __builtin_fmaf(b.z, wgt, C0);                                                         \
            C1 = __builtin_fmaf(b.w, wgt, C1);                                                         \
            C2 = __builtin_fmaf(c.x, wgt, C2);                                                         \
            if (DEPTH) Dacc = __builtin_fmaf(c.y, wgt, Dacc);                                          \
            T = acc ? test_T : T;                                                                      \
        }
        int jj = 0;
        for (; jj + 3 < n_w; jj += 4) {
            if (done_m == ~0ull) break;
            const unsigned j0 = sList[wave][jj], j1 = sList[wave][jj + 1], j2 = sList[wave][jj + 2], j3 = sList[wave][jj + 3];
            GVF_BLEND_STEP(j0)
            GVF_BLEND_STEP(j1)
            __builtin_amdgcn_sched_barrier(0);
            GVF_BLEND_STEP(j2)
            GVF_BLEND_STEP(j3)
        }
        for (; jj < n_w; ++jj) {
            if (done_m == ~0ull) break;
            const unsigned j0 = sList[wave][jj];
            GVF_BLEND_STEP(j0)
        }
#undef GVF_BLEND_STEP
    }
#ifdef BLEND_CONSUMED
    if (t == 0) {
        const unsigned n = rng.y - rng.x, used = min(n, (unsigned)rounds_done * BLEND_THREADS);
        const int cls = n <= 2048u ? 0 : n <= 4096u ? 1 : n <= 16384u ? 2 : 3;
        atomicAdd(&g_blend_cons[cls][0], 1ull); atomicAdd(&g_blend_cons[cls][1], (unsigned long long)n); atomicAdd(&g_blend_cons[cls][2], (unsigned long long)used);
    }
#endif
    if (inside) {
        const size_t hw = (size_t)H * W;
        const float r0 = __builtin_fmaf(T, bg0, C0), r1 = __builtin_fmaf(T, bg1, C1), r2 = __builtin_fmaf(T, bg2, C2);
        if (out_u8 != nullptr) {                   // (uniform) no fp32 frame in HBM at all when the caller wants the uint8 one
            unsigned char* ob = out_u8 + (size_t)f * 3 * hw;
            ob[0 * hw + pid] = (unsigned char)(fminf(fmaxf(r0, 0.f), 1.f) * 255.0f);
            ob[1 * hw + pid] = (unsigned char)(fminf(fmaxf(r1, 0.f), 1.f) * 255.0f);
            ob[2 * hw + pid] = (unsigned char)(fminf(fmaxf(r2, 0.f), 1.f) * 255.0f);
        } else {
            float* oc = out_color + (size_t)f * 3 * hw;
            oc[0 * hw + pid] = r0;
            oc[1 * hw + pid] = r1;
            oc[2 * hw + pid] = r2;
        }
        if (out_alpha != nullptr) out_alpha[(size_t)f * hw + pid] = 1.0f - T;
        if (out_depth != nullptr) out_depth[(size_t)f * hw + pid] = Dacc;
    }
#ifdef BLEND_TIMING
    BT(6);
    BT_VMWAIT(); BT(11);
    bt_acc[9] = 1; bt_acc[10] = bt_last - bt_first;
    const unsigned long long wid = ((unsigned long long)f * gridDim.x + tile) * 4 + wave;
    if (lane == 0 && g_blend_buf != nullptr && wid < g_blend_cap)
        for (int i = 0; i < 12; ++i) g_blend_buf[wid * 12 + i] = bt_acc[i];
#endif
}

// (Round 5 measured two more variants of the compositing step and dropped both: the two predicates as EXEC masks (if / else instead of v_cndmask:
// one vector instruction less, blend 0.82 ms against 0.70) and the colour accumulation on the idle matrix pipe (one v_mfma_f32_4x4x1_16b_f32 per
// splat and wave -- weights as A, channel (lane & 3) of {r, g, b, depth} as B -- instead of three v_fma_f32: 14 vector instructions + 1 MFMA per step
// against 16, blend 0.74 ms against 0.69).  profiles/r05_blend_branchy_ab.txt, r05_blend_mfma_accumulate_ab.txt; git history has both.)
// (Round 4 measured a matrix-pipe variant of this kernel -- the exponents of 32 splats x 64 pixels from v_mfma_f32_32x32x2_f32 on the expanded
// quadratic form, or from ONE v_mfma_f32_32x32x16_f16 with hi / lo split coefficients, software-pipelined under the compositing steps;
// 22.3 -> 14.4 vector instructions per step, images within 1e-6 of this kernel's -- and dropped it: 0.92 ms (fp16 split) / 1.03 ms (f32)
// against 0.80 ms.  profiles/r04_blend_matrix_pipe.txt has the numbers, git history (round 4) the kernel.)
// C1 post-process: rgb float -> uint8 exactly as utils/inference_utils.py:280-286 does on the host
// (clamp(0,1) * 255, truncating cast), so frames leave the device at 1 byte per channel.
__global__ __launch_bounds__(256) void rgb_to_u8_kernel(const float4* __restrict__ src, uchar4* __restrict__ dst,
                                                        long long n4, const float* __restrict__ tail_src,
                                                        unsigned char* __restrict__ tail_dst, int tail) {
    for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < n4; i += (long long)gridDim.x * blockDim.x) {
        const float4 v = src[i];
        uchar4 o;
        o.x = (unsigned char)(fminf(fmaxf(v.x, 0.f), 1.f) * 255.0f);
        o.y = (unsigned char)(fminf(fmaxf(v.y, 0.f), 1.f) * 255.0f);
        o.z = (unsigned char)(fminf(fmaxf(v.z, 0.f), 1.f) * 255.0f);
        o.w = (unsigned char)(fminf(fmaxf(v.w, 0.f), 1.f) * 255.0f);
        dst[i] = o;
    }
    if (blockIdx.x == 0 && (int)threadIdx.x < tail)
        tail_dst[threadIdx.x] = (unsigned char)(fminf(fmaxf(tail_src[threadIdx.x], 0.f), 1.f) * 255.0f);
}

}  // namespace

int gvf_rast::launch_blend(hipStream_t stream, const GvfRastSettings& st, int P, int F, const uint2* ranges, const uint32_t* point_list,
                           const float4* splats, const float* subpixel_offset, float* out_color, float* out_alpha, float* out_depth,
                           unsigned char* out_u8, const uint32_t* rec_of, uint32_t* tile_order, hipEvent_t ordered) {
    const int H = st.image_height, W = st.image_width;
    const int gx = (W + TILE - 1) / TILE, gy = (H + TILE - 1) / TILE, ntiles = gx * gy;
    if (tile_order != nullptr) hipLaunchKernelGGL(blend_order_kernel, dim3(F), dim3(1024), 0, stream, ranges, ntiles, tile_order);
    if (ordered != nullptr) (void)hipEventRecord(ordered, stream);
    hipLaunchKernelGGL(out_depth != nullptr ? blend_kernel<true> : blend_kernel<false>, dim3(ntiles, F), dim3(BLEND_THREADS), 0, stream, P, H, W,
                       gx, gy, st.bg[0], st.bg[1], st.bg[2], ranges, point_list, splats, subpixel_offset, out_color, out_alpha, out_depth,
                       tile_order, rec_of, out_u8);
    GVF_CHECK_LAUNCH();
    return GVF_OK;
}

extern "C" int gvf_rgb_to_u8(const float* rgb, uint8_t* out, int64_t n, void* stream) {
    if (n < 0) return GVF_EINVAL;
    if (n == 0) return GVF_OK;
    if (!rgb || !out || (((uintptr_t)rgb) & 15) || (((uintptr_t)out) & 3)) return GVF_EINVAL;
    (void)hipGetLastError();
    const long long n4 = n / 4;
    long long blocks = (n4 + 255) / 256;
    if (blocks < 1) blocks = 1;
    if (blocks > 8192) blocks = 8192;
    hipLaunchKernelGGL(rgb_to_u8_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream,
                       reinterpret_cast<const float4*>(rgb), reinterpret_cast<uchar4*>(out), n4, rgb + n4 * 4,
                       out + n4 * 4, (int)(n - n4 * 4));
    GVF_CHECK_LAUNCH();
    return GVF_OK;
}
