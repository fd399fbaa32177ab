// clip.hip -- the front and the back of CLIP's ViT-B/32 image tower on gfx950 (MI355X): the 32 x 32 patch convolution with the token assembly,
// ln_pre, and the read-out ln_post(cls) @ proj -> unit vector -> cosine.  C ABI, layouts and formulas: include/gvf_clip.h.  The blocks in
// between are launches of gemm.hip / attn.hip.
//
// Patch embedding = the 32 x 32 stride-32 convolution 3 -> D as an implicit GEMM on v_mfma_f32_16x16x32_{f16,bf16}:
//   acc[patch][d] = sum_k A16[patch][k] * W16[d][k],   k = c * 1024 + dy * 32 + dx  (3072 = 96 k-steps)
// A workgroup owns 32 patches x 128 channels, its four waves 2 x 2 (16 patches x 64 channels each), as in vit.hip.  32 whole patch rows would be
// 192 KiB, more than a CU's LDS, so K is staged in six chunks of 512 = 16 image lines of one channel: 32 rows of 512 16-bit values (32.5 KiB with
// the pitch below), gathered once per chunk -- a (channel, dy) line of neighbouring patches is one contiguous piece of the image -- and
// converted on the way in: a uint8 pixel through the 256-entry operand table of its channel (staged in LDS), an fp32 pixel by one rounding.
// Every accumulator runs ONE chain over the 96 k-steps in ascending k (chunks in order, 16 steps each), whatever the batch or the tile a patch
// falls in, so a token's bits depend on its pixels and the weights only.  The B fragments come straight from the packed weight (D x 6 KiB:
// it lives in L2).  The epilogue adds the position row and stores the fp32 token; a few extra workgroups of the same launch write cls + pos[0].
//
// LDS banking: rows are 520 elements apart (1040 bytes = 260 dwords, 260 mod 64 = 4): the 16 rows of an A-fragment read start at bank offsets
// 4 r mod 64 = sixteen distinct multiples of 4, so the ds_read_b128 of a 16-lane group covers all 64 banks once (the argument of vit.hip's 616).
//
// ln_pre is a second launch (gvf_clip_ln_rows): an in-place fp32 row LayerNorm that also writes the partial statistics gvf_gemm_ln reads.
#include "gvf_common.h"
#include "gvf_lp.h"
#include "gvf_rowops.h"
#include "../../include/gvf_rast.h"
#include "../../include/gvf_dit.h"
#include "../../include/gvf_clip.h"

namespace {

constexpr int NT = 256;
constexpr int PS = GVF_CLIP_PATCH;           // 32
constexpr int KP = GVF_CLIP_PATCH_K;         // 3072
constexpr int BM = 32, BN = 128;             // patches x channels per workgroup
constexpr int KC = 512;                      // k per staged chunk: 16 lines of 32 pixels of one channel
constexpr int NCH = KP / KC;                 // 6 chunks, two per channel
constexpr int LDA = 520;                     // 16-bit elements between staged patch rows (see the banking note above)
constexpr int MAXD = 1024, MAXE = 1024;

struct PatchArgs {
    const void* img; const unsigned short* lut; int B, S, g, n;
    const unsigned short* w; const float* cls; const float* pos; int D;
    float* x; int tiles_m;
};

template <int DT>
__global__ __launch_bounds__(NT) void clip_pack_patch_weight_kernel(const float* __restrict__ w, unsigned short* __restrict__ out, long long total) {
    for (long long i = blockIdx.x * (long long)NT + threadIdx.x; i < total; i += (long long)gridDim.x * NT) out[i] = GvfLp<DT>::to16(w[i]);
}

template <int DT, int KIND>
__global__ __launch_bounds__(NT) void clip_patch_embed_kernel(PatchArgs a) {
    typedef GvfLp<DT> LP;
    typedef typename LP::x8 x8;
    __shared__ uint4 sA4[BM * LDA / 8];                                   // 33 280 bytes
    __shared__ unsigned short sLut[256];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int n0 = blockIdx.y * BN;
    const int T = 1 + a.n;

    if ((int)blockIdx.x >= a.tiles_m) {
        // ---- the cls rows: a wave per (image, 64-column slice) of this workgroup's 128 columns
        const int u = ((int)blockIdx.x - a.tiles_m) * 4 + wave;
        const int b = u >> 1, slice = u & 1;
        if (b >= a.B) return;
        const int col = n0 + slice * 64 + lane;
        a.x[(size_t)b * T * a.D + col] = a.cls[col] + a.pos[col];
        return;
    }

    const int total = a.B * a.n;
    const int p0 = blockIdx.x * BM;
    const int wm = wave >> 1, wn = wave & 1;
    const int fi = lane & 15, fq = lane >> 4;
    gvf_f32x4 acc[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[j] = gvf_f32x4{0.f, 0.f, 0.f, 0.f};
    const unsigned short* arow = reinterpret_cast<const unsigned short*>(sA4) + (wm * 16 + fi) * LDA + fq * 8;
    const unsigned short* wrow[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) wrow[j] = a.w + (size_t)(n0 + wn * 64 + j * 16 + fi) * KP + fq * 8;

#pragma unroll 1
    for (int ch = 0; ch < NCH; ++ch) {
        const int c = ch >> 1, half = ch & 1;
        if (KIND == GVF_CLIP_IN_U8 && half == 0) sLut[threadIdx.x] = a.lut[c * 256 + threadIdx.x];      // (its readers passed the barrier below)
        __syncthreads();                                                  // the previous chunk's fragments are read; the table is in place
        // ---- gather: item = (line, patch, 8 pixels of the run); rows past the last patch repeat it (their results are dropped)
#pragma unroll 2
        for (int it = threadIdx.x; it < (KC / PS) * BM * (PS / 8); it += NT) {
            const int j = it & 3, pl = (it >> 2) & (BM - 1), dyl = it >> 7;
            int pg = p0 + pl;
            pg = pg < total ? pg : total - 1;
            const int b = pg / a.n, i = pg - b * a.n;
            const int py = i / a.g, px = i - py * a.g;
            const size_t at = (((size_t)b * 3 + c) * a.S + (py * PS + half * 16 + dyl)) * a.S + px * PS + 8 * j;
            uint4 q;
            if (KIND == GVF_CLIP_IN_U8) {
                const uint2 v = *reinterpret_cast<const uint2*>(reinterpret_cast<const unsigned char*>(a.img) + at);
                q.x = (unsigned)sLut[v.x & 255u] | ((unsigned)sLut[(v.x >> 8) & 255u] << 16);
                q.y = (unsigned)sLut[(v.x >> 16) & 255u] | ((unsigned)sLut[v.x >> 24] << 16);
                q.z = (unsigned)sLut[v.y & 255u] | ((unsigned)sLut[(v.y >> 8) & 255u] << 16);
                q.w = (unsigned)sLut[(v.y >> 16) & 255u] | ((unsigned)sLut[v.y >> 24] << 16);
            } else {
                const float* src = reinterpret_cast<const float*>(a.img) + at;
                const float4 v0 = *reinterpret_cast<const float4*>(src), v1 = *reinterpret_cast<const float4*>(src + 4);
                q.x = LP::pack(v0.x, v0.y); q.y = LP::pack(v0.z, v0.w); q.z = LP::pack(v1.x, v1.y); q.w = LP::pack(v1.z, v1.w);
            }
            sA4[pl * (LDA / 8) + dyl * (PS / 8) + j] = q;
        }
        __syncthreads();
#pragma unroll 4
        for (int ks = 0; ks < KC / 32; ++ks) {
            uint4 bv[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) bv[j] = *reinterpret_cast<const uint4*>(wrow[j] + ch * KC + ks * 32);
            const uint4 av = *reinterpret_cast<const uint4*>(arow + ks * 32);
#pragma unroll
            for (int j = 0; j < 4; ++j) acc[j] = LP::mfma16(__builtin_bit_cast(x8, av), __builtin_bit_cast(x8, bv[j]), acc[j]);
        }
    }

    // ---- epilogue: accumulator register r of fragment j = patch wm * 16 + fq * 4 + r, channel n0 + wn * 64 + j * 16 + fi
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int pg = p0 + wm * 16 + fq * 4 + r;
        if (pg >= total) continue;
        const int b = pg / a.n, i = pg - b * a.n;
        const size_t row = (size_t)b * T + 1 + i;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int col = n0 + wn * 64 + j * 16 + fi;
            a.x[row * a.D + col] = acc[j][r] + a.pos[(size_t)(1 + i) * a.D + col];
        }
    }
}

// One row per wave, the row in registers: lane l holds the float4s l, l + 64, ... of the row (D <= 1024: at most four).
struct RowLn {
    float4 v[4];
    __device__ __forceinline__ void load_normalise(const float* __restrict__ xr, int D, float eps, const float* __restrict__ ln_w,
                                                   const float* __restrict__ ln_b, int lane) {
        const int nv = D >> 2;
        const float4* x4 = reinterpret_cast<const float4*>(xr);
#pragma unroll
        for (int i = 0; i < 4; ++i) v[i] = lane + 64 * i < nv ? x4[lane + 64 * i] : make_float4(0.f, 0.f, 0.f, 0.f);
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
            if (lane + 64 * i < nv) {
                const float4 w4 = *reinterpret_cast<const float4*>(ln_w + (lane + 64 * i) * 4);
                const float4 b4 = *reinterpret_cast<const float4*>(ln_b + (lane + 64 * i) * 4);
                v[i].x = (v[i].x - mean) * rstd * w4.x + b4.x; v[i].y = (v[i].y - mean) * rstd * w4.y + b4.y;
                v[i].z = (v[i].z - mean) * rstd * w4.z + b4.z; v[i].w = (v[i].w - mean) * rstd * w4.w + b4.w;
            } else {
                v[i] = make_float4(0.f, 0.f, 0.f, 0.f);
            }
        }
    }
};

__global__ __launch_bounds__(NT) void clip_ln_rows_kernel(float* __restrict__ x, long long rows, int D, float eps, const float* __restrict__ ln_w,
                                                          const float* __restrict__ ln_b, float* __restrict__ stats) {
    const int lane = threadIdx.x & 63;
    const long long row = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= rows) return;
    float* xr = x + (size_t)row * D;
    RowLn r;
    r.load_normalise(xr, D, eps, ln_w, ln_b, lane);
    const int nv = D >> 2, parts = D >> 6;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const bool on = lane + 64 * i < nv;                              // nv is a multiple of 32: a 16-lane group is all on or all off
        if (on) reinterpret_cast<float4*>(xr)[lane + 64 * i] = r.v[i];
        if (stats != nullptr) {                                          // the 64-column slice 4 i + lane / 16 of the row as written
            const float4 y = r.v[i];
            const float s = gvf_row16_sum_xor((y.x + y.y) + (y.z + y.w));
            const float q = gvf_row16_sum_xor((y.x * y.x + y.y * y.y) + (y.z * y.z + y.w * y.w));
            if (on && (lane & 15) == 0) *reinterpret_cast<float2*>(stats + ((size_t)row * parts + i * 4 + (lane >> 4)) * 2) = make_float2(s, q);
        }
    }
}

// the four waves' totals added in wave order; every thread gets the sum
__device__ __forceinline__ float head_block_sum(float v, float* red) {
    v = gvf_wave_sum_dpp(v);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    return ((red[0] + red[1]) + red[2]) + red[3];
}

template <int DT>
__global__ __launch_bounds__(NT) void clip_head_kernel(const float* __restrict__ x, int L, int D, float eps, const float* __restrict__ ln_w,
                                                       const float* __restrict__ ln_b, const unsigned* __restrict__ proj, int E,
                                                       const float* __restrict__ g, float* __restrict__ feat, float* __restrict__ unit,
                                                       float* __restrict__ sim) {
    typedef GvfLp<DT> LP;
    __shared__ float sh[MAXD];
    __shared__ float red[4];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int b = blockIdx.x;
    if (wave == 0) {                                                      // h = r16(ln_post(x0)), as fp32
        RowLn r;
        r.load_normalise(x + (size_t)b * L * D, D, eps, ln_w, ln_b, lane);
        const int nv = D >> 2;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            if (lane + 64 * i < nv) {
                const unsigned lo = LP::pack(r.v[i].x, r.v[i].y), hi = LP::pack(r.v[i].z, r.v[i].w);
                *reinterpret_cast<float4*>(&sh[(lane + 64 * i) * 4]) = make_float4(LP::lo(lo), LP::hi(lo), LP::lo(hi), LP::hi(hi));
            }
        }
    }
    __syncthreads();
    // f: a thread owns the column pairs t and t + 256 (E <= 1024); one fma chain per column over ascending d
    // (a pair past the end reads the last pair instead and is dropped below: a load under a per-element condition would be waited for one by one)
    const int npair = E >> 1;
    float a0[2] = {0.f, 0.f}, a1[2] = {0.f, 0.f};
    const unsigned* pcol[2];
#pragma unroll
    for (int u = 0; u < 2; ++u) pcol[u] = proj + ((int)threadIdx.x + NT * u < npair ? (int)threadIdx.x + NT * u : npair - 1);
#pragma unroll 8
    for (int d = 0; d < D; ++d) {
        const float hd = sh[d];
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            const unsigned w = pcol[u][(size_t)d * npair];
            a0[u] = fmaf(hd, LP::lo(w), a0[u]);
            a1[u] = fmaf(hd, LP::hi(w), a1[u]);
        }
    }
    float f0[2], f1[2], ss = 0.f;
#pragma unroll
    for (int u = 0; u < 2; ++u) {
        const unsigned w = LP::pack(a0[u], a1[u]);
        f0[u] = LP::lo(w); f1[u] = LP::hi(w);
        if ((int)threadIdx.x + NT * u >= npair) { f0[u] = 0.f; f1[u] = 0.f; }
        ss += f0[u] * f0[u] + f1[u] * f1[u];
    }
    const float nrm = sqrtf(head_block_sum(ss, red));
    float dot = 0.f;
#pragma unroll
    for (int u = 0; u < 2; ++u) {
        const int q = (int)threadIdx.x + NT * u;
        if (q < npair) {
            const float u0 = f0[u] / nrm, u1 = f1[u] / nrm;
            const size_t o = (size_t)b * E + 2 * q;
            *reinterpret_cast<float2*>(feat + o) = make_float2(f0[u], f1[u]);
            *reinterpret_cast<float2*>(unit + o) = make_float2(u0, u1);
            if (g != nullptr) {
                const float2 g2 = *reinterpret_cast<const float2*>(g + 2 * q);
                dot += u0 * g2.x + u1 * g2.y;
            }
        }
    }
    if (g != nullptr) {
        const float s = head_block_sum(dot, red);
        if (threadIdx.x == 0) sim[b] = s;
    }
}

}  // namespace

extern "C" int gvf_clip_pack_patch_weight(int dtype, const float* w, int D, void* packed, void* stream_) {
    if (!gvf_lp_ok(dtype) || D <= 0 || !w || !packed || gvf_mis(packed, 15)) return GVF_EINVAL;
    (void)hipGetLastError();
    const long long total = (long long)D * KP;
    const int blocks = (int)(gvf_cdiv(total, NT) < 4096 ? gvf_cdiv(total, NT) : 4096);
    GVF_LP_DISPATCH(dtype, clip_pack_patch_weight_kernel<DT><<<dim3(blocks), dim3(NT), 0, (hipStream_t)stream_>>>(w, (unsigned short*)packed, total));
    GVF_CHECK_LAUNCH();
    return GVF_OK;
}

extern "C" int gvf_clip_patch_embed(int dtype, int in_kind, const void* img, const void* lut, int B, int S, const void* w_packed, const float* cls,
                                    const float* pos, int n_patches, int D, float* x, void* stream_) {
    if (!gvf_lp_ok(dtype) || (in_kind != GVF_CLIP_IN_U8 && in_kind != GVF_CLIP_IN_F32) || B < 0 || S <= 0 || (S % PS) != 0 || D <= 0 ||
        (D % BN) != 0 || n_patches <= 0)
        return GVF_EINVAL;
    if ((long long)(S / PS) * (S / PS) != n_patches) return GVF_EINVAL;            // the grid the position embedding was stored for, nothing else
    if (B == 0) return GVF_OK;
    if (!img || !w_packed || !cls || !pos || !x || (in_kind == GVF_CLIP_IN_U8 && !lut)) return GVF_EINVAL;
    if (gvf_mis(img, 15) || gvf_mis(w_packed, 15) || gvf_mis(x, 3) || gvf_mis(lut, 1)) return GVF_EINVAL;
    const long long total = (long long)B * n_patches;
    if (total > 0x3fffffffLL || (long long)B * 3 * S * S > 0x7fffffffffLL) return GVF_EINVAL;
    PatchArgs a;
    a.img = img; a.lut = (const unsigned short*)lut; a.B = B; a.S = S; a.g = S / PS; a.n = n_patches;
    a.w = (const unsigned short*)w_packed; a.cls = cls; a.pos = pos; a.D = D;
    a.x = x; a.tiles_m = (int)gvf_cdiv(total, BM);
    const long long gx = a.tiles_m + gvf_cdiv((long long)B * 2, 4);
    if (gx > 0x7fffffffLL || D / BN > 65535) return GVF_EINVAL;
    (void)hipGetLastError();
    const dim3 grid((unsigned)gx, (unsigned)(D / BN));
    if (in_kind == GVF_CLIP_IN_U8) {
        GVF_LP_DISPATCH(dtype, clip_patch_embed_kernel<DT, GVF_CLIP_IN_U8><<<grid, dim3(NT), 0, (hipStream_t)stream_>>>(a));
    } else {
        GVF_LP_DISPATCH(dtype, clip_patch_embed_kernel<DT, GVF_CLIP_IN_F32><<<grid, dim3(NT), 0, (hipStream_t)stream_>>>(a));
    }
    GVF_CHECK_LAUNCH();
    return GVF_OK;
}

extern "C" int gvf_clip_ln_rows(float* x, long long rows, int D, float eps, const float* ln_w, const float* ln_b, float* stats, void* stream_) {
    if (rows < 0 || D <= 0 || (D % 128) != 0 || D > MAXD || !(eps > 0.0f)) return GVF_EINVAL;
    if (rows == 0) return GVF_OK;
    if (!x || !ln_w || !ln_b || gvf_mis(x, 15) || gvf_mis(ln_w, 15) || gvf_mis(ln_b, 15) || gvf_mis(stats, 7)) return GVF_EINVAL;
    if (gvf_cdiv(rows, 4) > 0x7fffffffLL) return GVF_EINVAL;
    (void)hipGetLastError();
    clip_ln_rows_kernel<<<dim3((unsigned)gvf_cdiv(rows, 4)), dim3(NT), 0, (hipStream_t)stream_>>>(x, rows, D, eps, ln_w, ln_b, stats);
    GVF_CHECK_LAUNCH();
    return GVF_OK;
}

extern "C" int gvf_clip_head(int dtype, const float* x, int B, int L, int D, float eps, const float* ln_w, const float* ln_b, const void* proj, int E,
                             const float* g, float* feat, float* unit, float* sim, void* stream_) {
    if (!gvf_lp_ok(dtype) || B < 0 || L <= 0 || D <= 0 || (D % 128) != 0 || D > MAXD || E <= 0 || (E % 64) != 0 || E > MAXE || !(eps > 0.0f))
        return GVF_EINVAL;
    if (B == 0) return GVF_OK;
    if (!x || !ln_w || !ln_b || !proj || !feat || !unit || (g != nullptr && !sim)) return GVF_EINVAL;
    if (gvf_mis(x, 15) || gvf_mis(ln_w, 15) || gvf_mis(ln_b, 15) || gvf_mis(proj, 3) || gvf_mis(g, 7) || gvf_mis(feat, 7) || gvf_mis(unit, 7) ||
        gvf_mis(sim, 3))
        return GVF_EINVAL;
    (void)hipGetLastError();
    GVF_LP_DISPATCH(dtype, clip_head_kernel<DT><<<dim3((unsigned)B), dim3(NT), 0, (hipStream_t)stream_>>>(
                               x, L, D, eps, ln_w, ln_b, (const unsigned*)proj, E, g, feat, unit, sim));
    GVF_CHECK_LAUNCH();
    return GVF_OK;
}
