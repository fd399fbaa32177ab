// conv3x3.hip -- implicit-GEMM 3x3 convolution (stride 1, zero padding 1) on v_mfma_f32_16x16x32_{f16,bf16}, gfx950, and the two
// first-layer kernels of the LPIPS trunk.  C ABI, layouts and formulas: include/gvf_lpips.h.
//
// GEMM view: D[co][pixel] = sum_{tap, ci} Wimg[co][tap, ci] * patch[pixel + tap][ci].  The WEIGHTS are the MFMA's A operand (rows = output
// channels) and the pixels its B operand (columns), so that accumulator register r of lane l is output channel 4 (l / 16) + r of pixel
// l % 16: a lane owns four consecutive channels of one pixel and stores them with one 8-byte NHWC store.
//
// Tiling: one 256-thread workgroup per 16 x 16 pixel tile and 64 output channels; wave w owns tile rows 4w .. 4w + 3 (four 16-pixel B
// fragments) and all four 16-channel A fragments: 16 accumulators.  The input channels go in chunks of 32 (one k-step): the 18 x 18 halo
// patch of a chunk (64 bytes per pixel, zeros outside the image) is staged in LDS once and read nine times with shifted pixel addresses.
// The weight image is in fragment order (gvf_conv3x3_pack), so a wave's A fragment is one coalesced 1 KiB load that the L2 serves.
//
// LDS banking (MI355X: ds_read_b128 is serviced in four groups of 16 lanes -- {0-3, 12-15, 20-27}, ... -- over 64 banks): a B-fragment
// read takes 16 consecutive patch pixels p, lane quarter q reading 16-byte piece q of its pixel.  With a plain 64-byte pixel stride the
// bank is 16 (p % 4) + 4 q and a group's lanes collide four ways.  Piece q of pixel p is therefore stored at position q ^ (2 * ((p >> 2) & 1)):
// of the four pixels of one residue class p % 4 in a read, the first and the last are in the group with quarter q0 and the middle two
// with q0 ^ 1, and {f(t), f(t + 3), f(t + 1) ^ 1, f(t + 2) ^ 1} covers all four positions for f = (0, 2, 0, 2) at every start t.
#include "gvf_common.h"
#include "gvf_lp.h"
#include "../../include/gvf_rast.h"
#include "../../include/gvf_dit.h"
#include "../../include/gvf_lpips.h"

namespace {

constexpr int NT = 256;
constexpr int TS = 16;                  // tile side (pixels)
constexpr int PS = TS + 2;              // patch side
constexpr int PP = PS * PS;             // patch pixels: 324
constexpr int KC = 32;                  // input channels per chunk = one MFMA k-step
constexpr int CO_T = 64;                // output channels per workgroup

__device__ __forceinline__ int swz(int pp) { return ((pp >> 2) & 1) << 1; }

__device__ __forceinline__ bool positive16(unsigned short h) { return h != 0 && !(h & 0x8000u); }     // > 0 for fp16 and bf16 alike (no NaNs stored)

struct Tile {
    int n, y0, x0;
};
__device__ __forceinline__ Tile tile_of(int tiles_x, int tiles_y) {
    const int b = blockIdx.x;
    const int tx = b % tiles_x, t = b / tiles_x;
    return {t / tiles_y, (t % tiles_y) * TS, tx * TS};
}

// epilogue of one lane's four channels co .. co + 3 of pixel (y, x): bias, addend, ReLU, mask, 8-byte store
template <int DT>
__device__ __forceinline__ void store4(gvf_f32x4 v, const float* __restrict__ bias, const unsigned short* __restrict__ addend,
                                       const unsigned short* __restrict__ mask_src, unsigned short* __restrict__ out, int64_t o, int co,
                                       bool relu) {
    typedef GvfLp<DT> L;
    float f[4] = {v[0], v[1], v[2], v[3]};
    if (bias) {
#pragma unroll
        for (int r = 0; r < 4; ++r) f[r] += bias[co + r];
    }
    if (addend) {
        const uint2 a = *(const uint2*)(addend + o);
        f[0] += L::lo(a.x); f[1] += L::hi(a.x); f[2] += L::lo(a.y); f[3] += L::hi(a.y);
    }
    if (relu) {
#pragma unroll
        for (int r = 0; r < 4; ++r) f[r] = fmaxf(f[r], 0.f);
    }
    if (mask_src) {
        const uint2 m = *(const uint2*)(mask_src + o);
        if (!positive16((unsigned short)(m.x & 0xffffu))) f[0] = 0.f;
        if (!positive16((unsigned short)(m.x >> 16))) f[1] = 0.f;
        if (!positive16((unsigned short)(m.y & 0xffffu))) f[2] = 0.f;
        if (!positive16((unsigned short)(m.y >> 16))) f[3] = 0.f;
    }
    uint2 w;
    w.x = L::pack(f[0], f[1]);
    w.y = L::pack(f[2], f[3]);
    *(uint2*)(out + o) = w;
}

template <int DT>
__global__ __launch_bounds__(NT) void conv3x3_kernel(const unsigned short* __restrict__ in, const uint4* __restrict__ wimg,
                                                     const float* __restrict__ bias, const unsigned short* __restrict__ addend,
                                                     const unsigned short* __restrict__ mask_src, unsigned short* __restrict__ out, int H,
                                                     int W, int cin, int cout, int tiles_x, int tiles_y, int relu) {
    typedef GvfLp<DT> L;
    typedef typename L::x8 x8;
    __shared__ uint4 s_patch[PP * 4];       // 20.25 KiB
    const Tile t = tile_of(tiles_x, tiles_y);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int fi = lane & 15, fq = lane >> 4;
    const int nchunk = cin / KC;
    const int cb0 = blockIdx.y * (CO_T / 16);
    const int64_t img = (int64_t)t.n * H * W;

    gvf_f32x4 acc[4][4];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = gvf_f32x4{0.f, 0.f, 0.f, 0.f};

    for (int ch = 0; ch < nchunk; ++ch) {
        if (ch) __syncthreads();
        // stage: every load of the thread is issued before its first LDS store
        constexpr int IT = (PP * 4 + NT - 1) / NT;      // 6
        uint4 v[IT];
#pragma unroll
        for (int it = 0; it < IT; ++it) {
            const int idx = threadIdx.x + it * NT;
            const int pp = idx >> 2, q = idx & 3;
            const int r = pp / PS, c = pp - r * PS;
            const int y = t.y0 - 1 + r, x = t.x0 - 1 + c;
            v[it] = uint4{0u, 0u, 0u, 0u};
            if (idx < PP * 4 && y >= 0 && y < H && x >= 0 && x < W)
                v[it] = *(const uint4*)(in + (img + (int64_t)y * W + x) * cin + ch * KC + q * 8);
        }
#pragma unroll
        for (int it = 0; it < IT; ++it) {
            const int idx = threadIdx.x + it * NT;
            const int pp = idx >> 2, q = idx & 3;
            if (idx < PP * 4) s_patch[pp * 4 + (q ^ swz(pp))] = v[it];
        }
        __syncthreads();
#pragma unroll
        for (int tap = 0; tap < 9; ++tap) {
            const int dy = tap / 3, dx = tap % 3;
            x8 a[4], b[4];
#pragma unroll
            for (int i = 0; i < 4; ++i)
                a[i] = __builtin_bit_cast(x8, wimg[(((int64_t)(cb0 + i) * nchunk + ch) * 9 + tap) * 64 + lane]);
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int pp = (wave * 4 + j + dy) * PS + fi + dx;
                b[j] = __builtin_bit_cast(x8, s_patch[pp * 4 + (fq ^ swz(pp))]);
            }
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int j = 0; j < 4; ++j) acc[i][j] = L::mfma16(a[i], b[j], acc[i][j]);
        }
    }

    const int x = t.x0 + fi;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int y = t.y0 + wave * 4 + j;
        if (y >= H || x >= W) continue;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int co = blockIdx.y * CO_T + 16 * i + 4 * fq;
            const int64_t o = (img + (int64_t)y * W + x) * cout + co;
            store4<DT>(acc[i][j], bias, addend, mask_src, out, o, co, relu != 0);
        }
    }
}

// ---- weight images ---------------------------------------------------------------------------------------------------------------------
// element e = (((cb * nchunk + ch) * 9 + tap) * 64 + lane) * 8 + j: row = 16 cb + lane % 16, k = 32 ch + 8 (lane / 16) + j
template <int DT>
__global__ __launch_bounds__(NT) void pack_kernel(const float* __restrict__ w, int cout, int cin, int dgrad, unsigned short* __restrict__ out,
                                                  int64_t total) {
    const int nchunk = (dgrad ? cout : cin) / KC;
    for (int64_t e = (int64_t)blockIdx.x * NT + threadIdx.x; e < total; e += (int64_t)gridDim.x * NT) {
        const int j = (int)(e & 7), lane = (int)((e >> 3) & 63);
        int64_t r = e >> 9;
        const int tap = (int)(r % 9);
        r /= 9;
        const int ch = (int)(r % nchunk), cb = (int)(r / nchunk);
        const int row = 16 * cb + (lane & 15), k = KC * ch + 8 * (lane >> 4) + j;
        const float v = dgrad ? w[((int64_t)k * cin + row) * 9 + (8 - tap)] : w[((int64_t)row * cin + k) * 9 + tap];
        out[e] = GvfLp<DT>::to16(v);
    }
}

// first layer: [4 cb][64 lanes][8]; k = 3 tap + ci for k < 27, zero above
template <int DT>
__global__ __launch_bounds__(NT) void pack_first_kernel(const float* __restrict__ w, unsigned short* __restrict__ out) {
    for (int e = threadIdx.x; e < 4 * 64 * 8; e += NT) {
        const int j = e & 7, lane = (e >> 3) & 63, cb = e >> 9;
        const int row = 16 * cb + (lane & 15), k = 8 * (lane >> 4) + j;
        out[e] = GvfLp<DT>::to16(k < 27 ? w[(row * 3 + k % 3) * 9 + k / 3] : 0.f);
    }
}

// ---- first layer, forward: fp32 NCHW image, z-score fused, K = 27 in one k-step ------------------------------------------------------------
template <int DT>
__global__ __launch_bounds__(NT) void first_fwd_kernel(const float* __restrict__ xin, const uint4* __restrict__ wimg, const float* __restrict__ bias,
                                                       const float* __restrict__ mean, const float* __restrict__ std_,
                                                       unsigned short* __restrict__ out, int H, int W, int tiles_x, int tiles_y) {
    typedef GvfLp<DT> L;
    typedef typename L::x8 x8;
    __shared__ unsigned short s_p[3 * PP];
    const Tile t = tile_of(tiles_x, tiles_y);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int fi = lane & 15, fq = lane >> 4;
    const int64_t hw = (int64_t)H * W;
    for (int i = threadIdx.x; i < 3 * PP; i += NT) {
        const int c = i / PP, pp = i - c * PP;
        const int r = pp / PS, cc = pp - r * PS;
        const int y = t.y0 - 1 + r, x = t.x0 - 1 + cc;
        float v = 0.f;                                    // the padding is zero AFTER the z-score
        if (y >= 0 && y < H && x >= 0 && x < W) v = (xin[((int64_t)t.n * 3 + c) * hw + (int64_t)y * W + x] - mean[c]) / std_[c];
        s_p[i] = L::to16(v);
    }
    int off[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const int k = 8 * fq + j, tap = k / 3;
        off[j] = k < 27 ? (k % 3) * PP + (tap / 3) * PS + tap % 3 + fi : -1;
    }
    x8 a[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) a[i] = __builtin_bit_cast(x8, wimg[i * 64 + lane]);
    __syncthreads();
    const int x = t.x0 + fi;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int rr = wave * 4 + j, y = t.y0 + rr;
        unsigned short e[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) e[k] = off[k] >= 0 ? s_p[off[k] + rr * PS] : (unsigned short)0;
        uint4 bw;
        bw.x = e[0] | ((unsigned)e[1] << 16); bw.y = e[2] | ((unsigned)e[3] << 16);
        bw.z = e[4] | ((unsigned)e[5] << 16); bw.w = e[6] | ((unsigned)e[7] << 16);
        const x8 b = __builtin_bit_cast(x8, bw);
        gvf_f32x4 acc4[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) acc4[i] = L::mfma16(a[i], b, gvf_f32x4{0.f, 0.f, 0.f, 0.f});     // every lane takes part in the MFMAs
        if (y >= H || x >= W) continue;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const gvf_f32x4 acc = acc4[i];
            const int co = 16 * i + 4 * fq;
            const int64_t o = ((int64_t)t.n * hw + (int64_t)y * W + x) * 64 + co;
            store4<DT>(acc, bias, nullptr, nullptr, out, o, co, true);
        }
    }
}

// ---- first layer, input gradient: 64 -> 3 channels, direct; one thread per pixel ------------------------------------------------------------
__global__ __launch_bounds__(NT) void first_bwd_kernel(const unsigned short* __restrict__ z, const float* __restrict__ w, const float* __restrict__ std_,
                                                       float* __restrict__ dx, int H, int W, int tiles_x, int tiles_y) {
    typedef GvfLp<0> L;
    __shared__ float s_w[9][64][3];         // [tap][co][ci]
    for (int i = threadIdx.x; i < 9 * 64 * 3; i += NT) {
        const int ci = i % 3, co = (i / 3) % 64, tap = i / 192;
        s_w[tap][co][ci] = w[(co * 3 + ci) * 9 + tap];
    }
    __syncthreads();
    const Tile t = tile_of(tiles_x, tiles_y);
    const int y = t.y0 + (int)(threadIdx.x >> 4), x = t.x0 + (int)(threadIdx.x & 15);
    if (y >= H || x >= W) return;
    const int64_t hw = (int64_t)H * W;
    float a0 = 0.f, a1 = 0.f, a2 = 0.f;
    for (int tap = 0; tap < 9; ++tap) {
        const int yy = y + 1 - tap / 3, xx = x + 1 - tap % 3;
        if (yy < 0 || yy >= H || xx < 0 || xx >= W) continue;
        const uint4* p = (const uint4*)(z + ((int64_t)t.n * hw + (int64_t)yy * W + xx) * 64);
#pragma unroll
        for (int g = 0; g < 8; ++g) {
            const uint4 v = p[g];
            const unsigned wd[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
            for (int h = 0; h < 4; ++h) {
                const float lo = L::lo(wd[h]), hi = L::hi(wd[h]);
                const float* w0 = s_w[tap][8 * g + 2 * h];
                a0 = fmaf(lo, w0[0], a0); a1 = fmaf(lo, w0[1], a1); a2 = fmaf(lo, w0[2], a2);
                a0 = fmaf(hi, w0[3], a0); a1 = fmaf(hi, w0[4], a1); a2 = fmaf(hi, w0[5], a2);
            }
        }
    }
    const int64_t o = (int64_t)t.n * 3 * hw + (int64_t)y * W + x;
    dx[o] = a0 / std_[0];
    dx[o + hw] = a1 / std_[1];
    dx[o + 2 * hw] = a2 / std_[2];
}

bool chan_ok(int c) { return c == 64 || c == 128 || c == 256 || c == 512; }
bool dtype_ok(int dt) { return dt == GVF_DT_BF16 || dt == GVF_DT_F16; }
bool aligned16(const void* p) { return ((uintptr_t)p & 15u) == 0; }

// N, H, W >= 1, N H W 512 < 2^40, and the tile grid fits blockIdx.x
bool geom_ok(int N, int H, int W, int& tiles_x, int& tiles_y, unsigned& blocks) {
    if (N <= 0 || H <= 0 || W <= 0) return false;
    if ((int64_t)N * H * W > ((int64_t)1 << 31)) return false;
    tiles_x = (W + TS - 1) / TS;
    tiles_y = (H + TS - 1) / TS;
    const int64_t b = (int64_t)N * tiles_x * tiles_y;
    if (b > 0x7fffffff) return false;
    blocks = (unsigned)b;
    return true;
}

bool packed_size(int cout, int cin, int mode, size_t& bytes) {
    if (mode != GVF_CONV_PACK_FWD && mode != GVF_CONV_PACK_DGRAD) return false;
    if (cin == 3) {
        if (mode != GVF_CONV_PACK_FWD || cout != 64) return false;
        bytes = (size_t)64 * KC * 2;
        return true;
    }
    if (!chan_ok(cout) || !chan_ok(cin)) return false;
    bytes = (size_t)cout * cin * 9 * 2;
    return true;
}

}  // namespace

extern "C" int gvf_conv3x3_packed_bytes(int cout, int cin, int mode, size_t* out) {
    size_t b;
    if (!out || !packed_size(cout, cin, mode, b)) return GVF_EINVAL;
    *out = b;
    return GVF_OK;
}

extern "C" int gvf_conv3x3_pack(const float* w, int cout, int cin, int mode, int dtype, void* out, size_t out_bytes, void* stream) {
    size_t b;
    if (!w || !out || !dtype_ok(dtype) || !packed_size(cout, cin, mode, b) || !aligned16(out)) return GVF_EINVAL;
    if (out_bytes < b) return GVF_ENOSPC;
    hipStream_t s = (hipStream_t)stream;
    if (cin == 3) {
        GVF_LP_DISPATCH(dtype, (pack_first_kernel<DT><<<1, NT, 0, s>>>(w, (unsigned short*)out)));
    } else {
        const int64_t total = (int64_t)(b / 2);
        const unsigned blocks = (unsigned)((total + NT - 1) / NT < 4096 ? (total + NT - 1) / NT : 4096);
        GVF_LP_DISPATCH(dtype, (pack_kernel<DT><<<blocks, NT, 0, s>>>(w, cout, cin, mode == GVF_CONV_PACK_DGRAD, (unsigned short*)out, total)));
    }
    GVF_CHECK_LAUNCH();
    return GVF_OK;
}

extern "C" int gvf_conv3x3(const void* in, const void* wimg, const float* bias, const void* addend, const void* mask_src, void* out,
                           int N, int H, int W, int cin, int cout, int flags, int dtype, void* stream) {
    int tx, ty;
    unsigned blocks;
    if (!in || !wimg || !out || !dtype_ok(dtype) || !chan_ok(cin) || !chan_ok(cout) || (flags & ~GVF_CONV_RELU) ||
        !geom_ok(N, H, W, tx, ty, blocks))
        return GVF_EINVAL;
    if (!aligned16(in) || !aligned16(wimg) || !aligned16(out) || !aligned16(addend) || !aligned16(mask_src)) return GVF_EINVAL;
    hipStream_t s = (hipStream_t)stream;
    const dim3 grid(blocks, (unsigned)(cout / CO_T));
    GVF_LP_DISPATCH(dtype, (conv3x3_kernel<DT><<<grid, NT, 0, s>>>((const unsigned short*)in, (const uint4*)wimg, bias,
                                                                   (const unsigned short*)addend, (const unsigned short*)mask_src,
                                                                   (unsigned short*)out, H, W, cin, cout, tx, ty, flags & GVF_CONV_RELU)));
    GVF_CHECK_LAUNCH();
    return GVF_OK;
}

extern "C" int gvf_lpips_first_forward(const float* x, const void* wimg, const float* bias, const float* mean, const float* std_, void* out,
                                       int N, int H, int W, int dtype, void* stream) {
    int tx, ty;
    unsigned blocks;
    if (!x || !wimg || !bias || !mean || !std_ || !out || !dtype_ok(dtype) || !geom_ok(N, H, W, tx, ty, blocks)) return GVF_EINVAL;
    if (!aligned16(wimg) || !aligned16(out)) return GVF_EINVAL;
    hipStream_t s = (hipStream_t)stream;
    GVF_LP_DISPATCH(dtype, (first_fwd_kernel<DT><<<blocks, NT, 0, s>>>(x, (const uint4*)wimg, bias, mean, std_, (unsigned short*)out, H, W, tx, ty)));
    GVF_CHECK_LAUNCH();
    return GVF_OK;
}

extern "C" int gvf_lpips_first_backward(const void* z, const float* w, const float* std_, float* dx, int N, int H, int W, void* stream) {
    int tx, ty;
    unsigned blocks;
    if (!z || !w || !std_ || !dx || !geom_ok(N, H, W, tx, ty, blocks) || !aligned16(z)) return GVF_EINVAL;
    first_bwd_kernel<<<blocks, NT, 0, (hipStream_t)stream>>>((const unsigned short*)z, w, std_, dx, H, W, tx, ty);
    GVF_CHECK_LAUNCH();
    return GVF_OK;
}
