// vit.hip -- the front and the back of the DINOv2 ViT image encoder on gfx950 (MI355X): patch embedding with the token assembly, and the
// read-out of the token stream.  C ABI, layouts and formulas: include/gvf_vit.h.  The blocks in between are launches of gemm.hip / attn.hip.
//
// Patch embedding = the 14 x 14 stride-14 convolution 3 -> D as an implicit GEMM on v_mfma_f32_16x16x32_{f16,bf16}:
//   acc[patch][d] = sum_k r16((img - mean) / std)[patch][k] * W16[d][k],   k = c * 196 + dy * 14 + dx  (588, zero-padded to 608 = 19 k-steps)
// A workgroup owns 32 patches x 128 channels.  Its 32 patches -- 3 x 14 runs of 14 contiguous floats each -- are gathered from the fp32 image
// ONCE, z-scored in fp32, rounded once and laid down in LDS as 32 rows of 608 16-bit values (38.5 KiB); neighbouring patches of one patch
// row are neighbours in memory, so a (channel, dy) line of the tile is read as one contiguous piece.  The four waves (2 x 2: 16 patches x 64
// channels each) then run the 19 k-steps with the A fragment from LDS and the four B fragments straight from the packed weight (D x 1216
// bytes: it lives in L2).  The epilogue adds bias and position and stores the fp32 token rows, plus the (sum, sum of squares) of the wave's
// 64 columns of every row -- the partial LayerNorm statistics gvf_gemm_ln wants.  The cls / register rows are written by a few extra
// workgroups of the same launch.
//
// LDS banking: rows are 616 elements apart (1232 bytes = 308 dwords, 308 mod 64 = 52): the 16 rows of an A-fragment read start at bank
// offsets 52 r mod 64 = sixteen distinct multiples of 4, so the ds_read_b128 of a 16-lane group covers all 64 banks once.
//
// The image is re-gathered by each of the D / 128 column tiles of a patch tile (8 for ViT-L): 0.2 % of the encoder's FLOPs sit here,
// and the repeats are L2 hits; a wider tile would trade them for accumulator registers the kernel does not need to spend.
#include "gvf_common.h"
#include "gvf_lp.h"
#include "gvf_rowops.h"
#include "../../include/gvf_rast.h"
#include "../../include/gvf_dit.h"
#include "../../include/gvf_vit.h"

namespace {

constexpr int NT = 256;
constexpr int PS = GVF_VIT_PATCH;            // 14
constexpr int KP = GVF_VIT_PATCH_K;          // 588
constexpr int KPAD = GVF_VIT_PATCH_KPAD;     // 608
constexpr int BM = 32, BN = 128;             // patches x channels per workgroup
constexpr int LDA = 616;                     // 16-bit elements between staged patch rows (see the banking note above)
constexpr int LINES = 3 * PS;                // (channel, dy) lines of a patch: 42

struct PatchArgs {
    const float* img; int B, H, W, gw, n;
    float m0, m1, m2, s0, s1, s2;
    const unsigned short* w; const float* bias; const float* cls; const float* reg; int R; const float* pos; int D;
    float* x; float* stats; int tiles_m;
};

template <int DT>
__global__ __launch_bounds__(NT) void pack_patch_weight_kernel(const float* __restrict__ w, unsigned short* __restrict__ out, int D) {
    const long long total = (long long)D * KPAD;
    for (long long i = blockIdx.x * (long long)NT + threadIdx.x; i < total; i += (long long)gridDim.x * NT) {
        const long long d = i / KPAD;
        const int k = (int)(i - d * KPAD);
        out[i] = GvfLp<DT>::to16(k < KP ? w[d * KP + k] : 0.0f);
    }
}

template <int DT>
__global__ __launch_bounds__(NT) void patch_embed_kernel(PatchArgs a) {
    typedef GvfLp<DT> LP;
    typedef typename LP::x8 x8;
    __shared__ uint4 sA4[BM * LDA / 8];                                   // 39 424 bytes
    unsigned* sA = reinterpret_cast<unsigned*>(sA4);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int n0 = blockIdx.y * BN;
    const int T = 1 + a.R + a.n;
    const int parts = a.D / 64;

    if ((int)blockIdx.x >= a.tiles_m) {
        // ---- the cls / register rows: a wave per (row, 64-column slice) of this workgroup's 128 columns
        const int u = ((int)blockIdx.x - a.tiles_m) * 4 + wave;
        const int sr = u >> 1, slice = u & 1;
        if (sr >= a.B * (1 + a.R)) return;
        const int b = sr / (1 + a.R), t = sr - b * (1 + a.R);
        const int col = n0 + slice * 64 + lane;
        const float v = t == 0 ? a.cls[col] + a.pos[col] : a.reg[(size_t)(t - 1) * a.D + col];
        const size_t row = (size_t)b * T + t;
        a.x[row * a.D + col] = v;
        if (a.stats != nullptr) {
            const float s = gvf_wave_sum_xor(v), q = gvf_wave_sum_xor(v * v);
            if (lane == 0) *reinterpret_cast<float2*>(a.stats + (row * parts + (n0 >> 6) + slice) * 2) = make_float2(s, q);
        }
        return;
    }

    const int total = a.B * a.n;
    const int p0 = blockIdx.x * BM;
    // ---- gather: item = (line, patch, float2 of the run); rows past the last patch repeat it (their results are dropped)
    constexpr int ITEMS = LINES * BM * (PS / 2);                           // 9408
#pragma unroll 4
    for (int it = threadIdx.x; it < ITEMS; it += NT) {
        const int j = it % (PS / 2), t2 = it / (PS / 2);
        const int pl = t2 % BM, cr = t2 / BM;
        const int c = cr / PS, dy = cr - c * PS;
        int pg = p0 + pl;
        pg = pg < total ? pg : total - 1;
        const int b = pg / a.n, i = pg - b * a.n;
        const int py = i / a.gw, px = i - py * a.gw;
        const float2 v = *reinterpret_cast<const float2*>(a.img + (((size_t)b * 3 + c) * a.H + (py * PS + dy)) * a.W + px * PS + 2 * j);
        const float m = c == 0 ? a.m0 : (c == 1 ? a.m1 : a.m2), s = c == 0 ? a.s0 : (c == 1 ? a.s1 : a.s2);
        sA[(pl * LDA + cr * PS + 2 * j) >> 1] = LP::pack((v.x - m) / s, (v.y - m) / s);
    }
    for (int it = threadIdx.x; it < BM * ((KPAD - KP) / 2); it += NT) {   // the zero padding k = 588 .. 607
        const int pl = it / ((KPAD - KP) / 2), q = it - pl * ((KPAD - KP) / 2);
        sA[((pl * LDA + KP) >> 1) + q] = 0u;
    }
    __syncthreads();

    const int wm = wave >> 1, wn = wave & 1;
    const int fi = lane & 15, fq = lane >> 4;
    gvf_f32x4 acc[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[j] = gvf_f32x4{0.f, 0.f, 0.f, 0.f};
    const unsigned short* arow = reinterpret_cast<const unsigned short*>(sA4) + (wm * 16 + fi) * LDA + fq * 8;
    const unsigned short* wrow[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) wrow[j] = a.w + (size_t)(n0 + wn * 64 + j * 16 + fi) * KPAD + fq * 8;
#pragma unroll 1
    for (int ks = 0; ks < KPAD / 32; ++ks) {
        uint4 bv[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) bv[j] = *reinterpret_cast<const uint4*>(wrow[j] + ks * 32);
        const uint4 av = *reinterpret_cast<const uint4*>(arow + ks * 32);
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[j] = LP::mfma16(__builtin_bit_cast(x8, av), __builtin_bit_cast(x8, bv[j]), acc[j]);
    }

    // ---- epilogue: accumulator register r of fragment j = patch wm * 16 + fq * 4 + r, channel n0 + wn * 64 + j * 16 + fi
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int pg = p0 + wm * 16 + fq * 4 + r;
        const bool ok = pg < total;
        const int pgc = ok ? pg : total - 1;
        const int b = pgc / a.n, i = pgc - b * a.n;
        const size_t row = (size_t)b * T + 1 + a.R + i;
        float v[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int col = n0 + wn * 64 + j * 16 + fi;
            v[j] = (acc[j][r] + (a.bias != nullptr ? a.bias[col] : 0.0f)) + a.pos[(size_t)(1 + i) * a.D + col];
            if (ok) a.x[row * a.D + col] = v[j];
        }
        if (a.stats != nullptr) {                                        // this wave's 64 columns of the row: two adds in the lane, four shuffles
            float s = (v[0] + v[1]) + (v[2] + v[3]);
            float q = (v[0] * v[0] + v[1] * v[1]) + (v[2] * v[2] + v[3] * v[3]);
#pragma unroll
            for (int d = 1; d < 16; d <<= 1) { s += __shfl_xor(s, d, 64); q += __shfl_xor(q, d, 64); }
            if (ok && fi == 0) *reinterpret_cast<float2*>(a.stats + (row * parts + (n0 >> 6) + wn) * 2) = make_float2(s, q);
        }
    }
}

template <bool F16>
__global__ __launch_bounds__(NT) void tokens_out_kernel(const float* __restrict__ x, void* __restrict__ out, int B, int R, int n, int D, int mode,
                                                        float eps, const float* __restrict__ ln_w, const float* __restrict__ ln_b, int order) {
    const int lane = threadIdx.x & 63;
    const long long orow = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    const int T = 1 + R + n, To = order == GVF_VIT_ORDER_STORED ? T : n + 1;
    if (orow >= (long long)B * To) return;
    const int b = (int)(orow / To), j = (int)(orow - (long long)b * To);
    const int t = order == GVF_VIT_ORDER_STORED ? j : (j < n ? 1 + R + j : 0);
    const float4* xr = reinterpret_cast<const float4*>(x + ((size_t)b * T + t) * D);
    const int nv = D >> 2;
    float4 v[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) v[i] = lane + 64 * i < nv ? xr[lane + 64 * i] : make_float4(0.f, 0.f, 0.f, 0.f);
    if (mode != GVF_VIT_OUT_COPY) {
        float s = 0.f;
#pragma unroll
        for (int i = 0; i < 4; ++i) s += (v[i].x + v[i].y) + (v[i].z + v[i].w);
        const float mean = gvf_wave_sum_dpp(s) / (float)D;
        float q = 0.f;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            if (lane + 64 * i < nv) {
                const float a0 = v[i].x - mean, a1 = v[i].y - mean, a2 = v[i].z - mean, a3 = v[i].w - mean;
                q += (a0 * a0 + a1 * a1) + (a2 * a2 + a3 * a3);
            }
        }
        const float rstd = rsqrtf(gvf_wave_sum_dpp(q) / (float)D + eps);
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            v[i].x = (v[i].x - mean) * rstd; v[i].y = (v[i].y - mean) * rstd; v[i].z = (v[i].z - mean) * rstd; v[i].w = (v[i].w - mean) * rstd;
            if (mode == GVF_VIT_OUT_LN_AFFINE && lane + 64 * i < nv) {
                const float4 w4 = *reinterpret_cast<const float4*>(ln_w + (lane + 64 * i) * 4);
                const float4 b4 = *reinterpret_cast<const float4*>(ln_b + (lane + 64 * i) * 4);
                v[i].x = v[i].x * w4.x + b4.x; v[i].y = v[i].y * w4.y + b4.y; v[i].z = v[i].z * w4.z + b4.z; v[i].w = v[i].w * w4.w + b4.w;
            }
        }
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        if (lane + 64 * i >= nv) continue;
        const size_t o = (size_t)orow * D + (size_t)(lane + 64 * i) * 4;
        if (F16) {
            uint2 w2;
            w2.x = GvfLp<GVF_DT_F16>::pack(v[i].x, v[i].y); w2.y = GvfLp<GVF_DT_F16>::pack(v[i].z, v[i].w);
            *reinterpret_cast<uint2*>(reinterpret_cast<unsigned short*>(out) + o) = w2;
        } else {
            *reinterpret_cast<float4*>(reinterpret_cast<float*>(out) + o) = v[i];
        }
    }
}

}  // namespace

extern "C" int gvf_vit_pack_patch_weight(int dtype, const float* w, int D, void* packed, void* stream_) {
    if (!gvf_lp_ok(dtype) || D <= 0 || !w || !packed || gvf_mis(packed, 15)) return GVF_EINVAL;
    (void)hipGetLastError();
    const long long total = (long long)D * KPAD;
    const int blocks = (int)(gvf_cdiv(total, NT) < 4096 ? gvf_cdiv(total, NT) : 4096);
    GVF_LP_DISPATCH(dtype, pack_patch_weight_kernel<DT><<<dim3(blocks), dim3(NT), 0, (hipStream_t)stream_>>>(w, (unsigned short*)packed, D));
    GVF_CHECK_LAUNCH();
    return GVF_OK;
}

extern "C" int gvf_vit_patch_embed(int dtype, const float* img, int B, int H, int W, const float* mean, const float* std, const void* w_packed,
                                   const float* bias, const float* cls, const float* reg, int R, const float* pos, int n_patches, int D,
                                   float* x, float* stats, void* stream_) {
    if (!gvf_lp_ok(dtype) || B < 0 || H <= 0 || W <= 0 || (H % PS) != 0 || (W % PS) != 0 || D <= 0 || (D % BN) != 0 || R < 0 || n_patches <= 0)
        return GVF_EINVAL;
    if ((long long)(H / PS) * (W / PS) != n_patches) return GVF_EINVAL;            // the grid the position embedding was stored for, nothing else
    if (B == 0) return GVF_OK;
    if (!img || !mean || !std || !w_packed || !cls || !pos || !x || (R > 0 && !reg)) return GVF_EINVAL;
    if (gvf_mis(img, 7) || gvf_mis(w_packed, 15) || gvf_mis(x, 3) || gvf_mis(stats, 7)) return GVF_EINVAL;
    if (!(std[0] != 0.0f) || !(std[1] != 0.0f) || !(std[2] != 0.0f)) return GVF_EINVAL;
    const long long total = (long long)B * n_patches, special = (long long)B * (1 + R);
    if (total > 0x3fffffffLL || special > 0x3fffffffLL) return GVF_EINVAL;
    PatchArgs a;
    a.img = img; a.B = B; a.H = H; a.W = W; a.gw = W / PS; a.n = n_patches;
    a.m0 = mean[0]; a.m1 = mean[1]; a.m2 = mean[2]; a.s0 = std[0]; a.s1 = std[1]; a.s2 = std[2];
    a.w = (const unsigned short*)w_packed; a.bias = bias; a.cls = cls; a.reg = reg; a.R = R; a.pos = pos; a.D = D;
    a.x = x; a.stats = stats; a.tiles_m = (int)gvf_cdiv(total, BM);
    const long long gx = a.tiles_m + gvf_cdiv(special * 2, 4);
    if (gx > 0x7fffffffLL || D / BN > 65535) return GVF_EINVAL;
    (void)hipGetLastError();
    const dim3 grid((unsigned)gx, (unsigned)(D / BN));
    GVF_LP_DISPATCH(dtype, patch_embed_kernel<DT><<<grid, dim3(NT), 0, (hipStream_t)stream_>>>(a));
    GVF_CHECK_LAUNCH();
    return GVF_OK;
}

extern "C" int gvf_vit_tokens_out(const float* x, int B, int R, int n_patches, int D, int mode, float eps, const float* ln_w, const float* ln_b,
                                  int order, int out_f16, void* out, void* stream_) {
    if (B < 0 || R < 0 || n_patches <= 0 || D <= 0 || (D % 4) != 0 || D > 1024) return GVF_EINVAL;
    if (mode != GVF_VIT_OUT_COPY && mode != GVF_VIT_OUT_LN_AFFINE && mode != GVF_VIT_OUT_LN) return GVF_EINVAL;
    if (order != GVF_VIT_ORDER_STORED && order != GVF_VIT_ORDER_PATCHES_CLS) return GVF_EINVAL;
    if (mode != GVF_VIT_OUT_COPY && !(eps > 0.0f)) return GVF_EINVAL;
    if (B == 0) return GVF_OK;
    if (!x || !out || gvf_mis(x, 15) || gvf_mis(out, 15)) return GVF_EINVAL;
    if (mode == GVF_VIT_OUT_LN_AFFINE && (!ln_w || !ln_b || gvf_mis(ln_w, 15) || gvf_mis(ln_b, 15))) return GVF_EINVAL;
    const long long rows = (long long)B * (order == GVF_VIT_ORDER_STORED ? 1 + R + n_patches : n_patches + 1);
    if (gvf_cdiv(rows, 4) > 0x7fffffffLL) return GVF_EINVAL;
    (void)hipGetLastError();
    const dim3 grid((unsigned)gvf_cdiv(rows, 4)), block(NT);
    if (out_f16) tokens_out_kernel<true><<<grid, block, 0, (hipStream_t)stream_>>>(x, out, B, R, n_patches, D, mode, eps, ln_w, ln_b, order);
    else tokens_out_kernel<false><<<grid, block, 0, (hipStream_t)stream_>>>(x, out, B, R, n_patches, D, mode, eps, ln_w, ln_b, order);
    GVF_CHECK_LAUNCH();
    return GVF_OK;
}
