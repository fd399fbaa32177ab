// spconv.hip -- submanifold sparse 3x3x3 convolution on v_mfma_f32_16x16x32_{f16,bf16}, its neighbour map and weight image, and the
// LayerNorm + activation link in front of it, gfx950.  C ABI, definition and layouts: include/gvf_spconv.h.
//
// GEMM view: D[co][row] = sum_{tap, ci} Wimg[co][tap, ci] * in[nbr[row][tap]][ci].  As in conv3x3.hip the WEIGHTS are the MFMA's A operand
// (rows = output channels) and the voxel rows its B operand (columns): accumulator register r of lane l is output channel 4 (l / 16) + r of
// row l % 16, so a lane owns four consecutive channels of one output row (one 16- or 8-byte store), and output row n depends on column n
// of B alone -- a NaN in a gathered row stays in the outputs that gathered it.
//
// Tiling: one 256-thread workgroup per 64 output rows and 64 AF output channels (AF = 4, 2, 1 by the divisibility of Cout); wave w owns
// the AF 16-channel A fragments 16 AF w ... and all four 16-row B fragments: 4 AF accumulators.  The walk is tap-major: for every tap
// that has a neighbour somewhere in the tile (a wave-uniform mask, built once from the tile's 64 x 27 map entries), the input channels
// go in stages of 64 (two k-steps): the stage's 64 x 128 B of gathered rows are loaded with 16-byte loads, eight lanes per row, into
// registers while the previous stage is multiplied, and written to the other of two LDS buffers (one barrier per stage).  An absent
// neighbour's piece is a zero written to LDS, never a load.  The weight image is in fragment order, so an A fragment is one coalesced
// 1 KiB load; the workgroups of one weight slice are neighbours in launch order and share it in L2.
//
// LDS banking (ds_read_b128 is served in four groups of 16 lanes -- {0-3, 12-15, 20-27}, ... -- over 64 banks): a row is 128 B, so with a
// plain layout the 16-byte unit of piece p of row r is 8 (r % 2) + p and rows of equal parity collide.  Piece p of row r is stored at
// position p ^ ((r / 2) % 8): in a group the eight rows of one parity are r / 2 = {0, 1, 6, 7} with piece P and {2, 3, 4, 5} with piece
// P ^ 1 (or the mirror image), whose positions P ^ {0, 1, 6, 7, 3, 2, 5, 4} are all different.
#include "gvf_common.h"
#include "gvf_lp.h"
#include "gvf_rowops.h"
#include "../../include/gvf_rast.h"
#include "../../include/gvf_dit.h"
#include "../../include/gvf_spconv.h"

namespace {

constexpr int NT = 256;
constexpr int TR = 64;                  // output rows per workgroup
constexpr int KS = 64;                  // input channels per stage (two MFMA k-steps)
constexpr int NTAP = 27;
constexpr int CMAX = 2048;
constexpr unsigned long long EMPTY = ~0ull;

// ---- neighbour map -----------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ bool in_grid(int v) { return (unsigned)v < 1024u; }
__device__ __forceinline__ unsigned long long pack_key(int b, int x, int y, int z) {
    return ((unsigned long long)(unsigned)b << 30) | ((unsigned long long)x << 20) | ((unsigned long long)y << 10) | (unsigned long long)z;
}
__device__ __forceinline__ unsigned slot_of(unsigned long long key, unsigned mask) {
    return (unsigned)((key * 0x9E3779B97F4A7C15ull) >> 32) & mask;
}

__global__ __launch_bounds__(NT) void map_insert_kernel(const int4* __restrict__ coords, int T, unsigned long long* __restrict__ keys,
                                                        int* __restrict__ vals, unsigned mask) {
    const int i = blockIdx.x * NT + threadIdx.x;
    if (i >= T) return;
    const int4 c = coords[i];
    if (c.x < 0 || !in_grid(c.y) || !in_grid(c.z) || !in_grid(c.w)) return;
    const unsigned long long key = pack_key(c.x, c.y, c.z, c.w);
    unsigned s = slot_of(key, mask);
    for (unsigned n = 0; n <= mask; ++n, s = (s + 1) & mask) {
        const unsigned long long old = atomicCAS(keys + s, EMPTY, key);
        if (old == EMPTY || old == key) {
            vals[s] = i;
            return;
        }
    }
}

__global__ __launch_bounds__(NT) void map_lookup_kernel(const int4* __restrict__ coords, int T, const unsigned long long* __restrict__ keys,
                                                        const int* __restrict__ vals, unsigned mask, int* __restrict__ nbr) {
    const int e = blockIdx.x * NT + threadIdx.x;           // 27 T < 2^31
    if (e >= T * NTAP) return;
    const int i = e / NTAP, k = e - i * NTAP;
    const int4 c = coords[i];
    const int x = c.y + k / 9 - 1, y = c.z + (k / 3) % 3 - 1, z = c.w + k % 3 - 1;
    int j = -1;
    if (c.x >= 0 && in_grid(c.y) && in_grid(c.z) && in_grid(c.w) && in_grid(x) && in_grid(y) && in_grid(z)) {
        const unsigned long long key = pack_key(c.x, x, y, z);
        unsigned s = slot_of(key, mask);
        for (unsigned n = 0; n <= mask; ++n, s = (s + 1) & mask) {
            const unsigned long long have = keys[s];
            if (have == key) { j = vals[s]; break; }
            if (have == EMPTY) break;
        }
    }
    nbr[e] = j;
}

// table slots: the power of two >= 2 T (load <= 1/2), at least 64
bool map_slots(int T, size_t& slots) {
    if (T < 1 || (int64_t)T * NTAP > 0x7fffffffll) return false;
    size_t s = 64;
    while (s < (size_t)2 * (size_t)T) s <<= 1;
    slots = s;
    return true;
}

// ---- weight image ------------------------------------------------------------------------------------------------------------------------
template <int DT>
__global__ __launch_bounds__(NT) void pack_kernel(const float* __restrict__ w, int cin, unsigned short* __restrict__ out, int64_t total) {
    const int nch = cin / 32;
    for (int64_t e = (int64_t)blockIdx.x * NT + threadIdx.x; e < total; e += (int64_t)gridDim.x * NT) {
        const int j = (int)(e & 7), lane = (int)((e >> 3) & 63);
        int64_t r = e >> 9;
        const int ch = (int)(r % nch);
        r /= nch;
        const int tap = (int)(r % NTAP), cb = (int)(r / NTAP);
        const int row = 16 * cb + (lane & 15), k = 32 * ch + 8 * (lane >> 4) + j;
        out[e] = GvfLp<DT>::to16(w[((int64_t)row * NTAP + tap) * cin + k]);
    }
}

// ---- the convolution ---------------------------------------------------------------------------------------------------------------------
template <int DT, int AF, bool OUT32>
__global__ __launch_bounds__(NT) void spconv3_kernel(const unsigned short* __restrict__ in, int ld_in, const int* __restrict__ nbr,
                                                     const uint4* __restrict__ wimg, const float* __restrict__ bias,
                                                     const float* __restrict__ addend, void* __restrict__ out_, int T, int cin, int cout) {
    typedef GvfLp<DT> L;
    typedef typename L::x8 x8;
    __shared__ uint4 s_b[2][TR * 8];        // 16 KiB
    __shared__ int s_nbr[NTAP][TR];         // 6.75 KiB
    __shared__ unsigned s_any[NTAP];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int fi = lane & 15, fq = lane >> 4;
    const int tile0 = blockIdx.x * TR;
    const int nch = cin / 32, nks = cin / KS;
    const int cb0 = (blockIdx.y * 4 + wave) * AF;

    for (int idx = threadIdx.x; idx < TR * NTAP; idx += NT) {
        const int r = idx / NTAP, k = idx - r * NTAP;
        int j = -1;
        if (tile0 + r < T) {
            j = nbr[(int64_t)(tile0 + r) * NTAP + k];
            if ((unsigned)j >= (unsigned)T) j = -1;        // a map that is not this tensor's must not send a load out of the rows
        }
        s_nbr[k][r] = j;
    }
    __syncthreads();
    for (int k = wave; k < NTAP; k += 4) {
        const unsigned long long any = __ballot(s_nbr[k][lane] >= 0);
        if (lane == 0) s_any[k] = any != 0ull;
    }
    __syncthreads();
    unsigned m = 0;
#pragma unroll
    for (int k = 0; k < NTAP; ++k) m |= s_any[k] << k;
    unsigned todo = __builtin_amdgcn_readfirstlane(m);      // taps still to walk, ascending

    gvf_f32x4 acc[AF][4];
#pragma unroll
    for (int i = 0; i < AF; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = gvf_f32x4{0.f, 0.f, 0.f, 0.f};

    // the thread's two 16-byte pieces of a stage: rows r0 and r0 + 32, piece p of the stage's 128 B
    const int r0 = threadIdx.x >> 3, p = threadIdx.x & 7;
    auto gather = [&](int tap, int ks, uint4 (&v)[2]) {
#pragma unroll
        for (int it = 0; it < 2; ++it) {
            const int j = s_nbr[tap][r0 + 32 * it];
            v[it] = uint4{0u, 0u, 0u, 0u};
            if (j >= 0) v[it] = *(const uint4*)(in + (int64_t)j * ld_in + ks * KS + p * 8);
        }
    };
    auto stash = [&](int buf, const uint4 (&v)[2]) {
#pragma unroll
        for (int it = 0; it < 2; ++it) {
            const int r = r0 + 32 * it;
            s_b[buf][r * 8 + (p ^ ((r >> 1) & 7))] = v[it];
        }
    };

    uint4 v[2];
    int tap = 0, ks = 0, buf = 0;
    if (todo) {
        tap = __builtin_ctz(todo);
        gather(tap, 0, v);
        stash(0, v);
    }
    __syncthreads();
    while (todo) {
        // the stage after this one
        int ntap = tap, nk = ks + 1;
        unsigned rest = todo;
        if (nk == nks) {
            nk = 0;
            rest = todo & (todo - 1);
            ntap = rest ? __builtin_ctz(rest) : 0;
        }
        if (rest) gather(ntap, nk, v);
#pragma unroll
        for (int s = 0; s < 2; ++s) {
            x8 a[AF], b[4];
#pragma unroll
            for (int i = 0; i < AF; ++i)
                a[i] = __builtin_bit_cast(x8, wimg[(((int64_t)(cb0 + i) * NTAP + tap) * nch + ks * 2 + s) * 64 + lane]);
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int r = 16 * j + fi;
                b[j] = __builtin_bit_cast(x8, s_b[buf][r * 8 + ((4 * s + fq) ^ ((r >> 1) & 7))]);
            }
#pragma unroll
            for (int i = 0; i < AF; ++i)
#pragma unroll
                for (int j = 0; j < 4; ++j) acc[i][j] = L::mfma16(a[i], b[j], acc[i][j]);
        }
        if (rest) stash(buf ^ 1, v);
        __syncthreads();
        buf ^= 1;
        todo = rest;
        tap = ntap;
        ks = nk;
    }

#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int row = tile0 + 16 * j + fi;
        if (row >= T) continue;
#pragma unroll
        for (int i = 0; i < AF; ++i) {
            const int co = 16 * (cb0 + i) + 4 * fq;
            const int64_t o = (int64_t)row * cout + co;
            float f[4] = {acc[i][j][0], acc[i][j][1], acc[i][j][2], acc[i][j][3]};
            if (bias) {
                const float4 b4 = *(const float4*)(bias + co);
                f[0] += b4.x; f[1] += b4.y; f[2] += b4.z; f[3] += b4.w;
            }
            if (addend) {
                const float4 a4 = *(const float4*)(addend + o);
                f[0] += a4.x; f[1] += a4.y; f[2] += a4.z; f[3] += a4.w;
            }
            if (OUT32) {
                *(float4*)((float*)out_ + o) = float4{f[0], f[1], f[2], f[3]};
            } else {
                uint2 w2;
                w2.x = L::pack(f[0], f[1]);
                w2.y = L::pack(f[2], f[3]);
                *(uint2*)((unsigned short*)out_ + o) = w2;
            }
        }
    }
}

// ---- LayerNorm + activation ----------------------------------------------------------------------------------------------------------------
// one wave per row; the row stays in registers: VPL float4 per lane, C <= 256 VPL.  The arithmetic is that of elem.hip's ln_mod_kernel
// (the same rounding counts), with the activation on top.
template <int VPL, int DT>
__global__ __launch_bounds__(NT) void ln_act_kernel(const float* __restrict__ x, unsigned short* __restrict__ out, int rows, int C, float eps,
                                                    const float* __restrict__ ln_w, const float* __restrict__ ln_b,
                                                    const float* __restrict__ shift, const float* __restrict__ scale, int act) {
    const int lane = threadIdx.x & 63;
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= rows) return;
    const float4* xr = reinterpret_cast<const float4*>(x + (size_t)row * C);
    const int nv = C >> 2;
    float4 v[VPL];
    float s = 0.f;
#pragma unroll
    for (int i = 0; i < VPL; ++i) {
        v[i] = float4{0.f, 0.f, 0.f, 0.f};
        if (lane + 64 * i < nv) {
            v[i] = xr[lane + 64 * i];
            s += (v[i].x + v[i].y) + (v[i].z + v[i].w);
        }
    }
    const float mean = gvf_wave_sum_dpp(s) / (float)C;
    float q = 0.f;
#pragma unroll
    for (int i = 0; i < VPL; ++i) {
        if (lane + 64 * i < nv) {
            const float a = v[i].x - mean, b = v[i].y - mean, c = v[i].z - mean, d = v[i].w - mean;
            q += (a * a + b * b) + (c * c + d * d);
        }
    }
    const float rstd = rsqrtf(gvf_wave_sum_dpp(q) / (float)C + eps);
#pragma unroll
    for (int i = 0; i < VPL; ++i) {
        if (lane + 64 * i >= nv) continue;
        const int c0 = (lane + 64 * i) * 4;
        float y[4] = {(v[i].x - mean) * rstd, (v[i].y - mean) * rstd, (v[i].z - mean) * rstd, (v[i].w - mean) * rstd};
        if (ln_w != nullptr) {
            const float4 w4 = *reinterpret_cast<const float4*>(ln_w + c0);
            const float4 b4 = *reinterpret_cast<const float4*>(ln_b + c0);
            y[0] = y[0] * w4.x + b4.x; y[1] = y[1] * w4.y + b4.y; y[2] = y[2] * w4.z + b4.z; y[3] = y[3] * w4.w + b4.w;
        }
        if (scale != nullptr) {
            const float4 sc = *reinterpret_cast<const float4*>(scale + c0);
            const float4 sh = *reinterpret_cast<const float4*>(shift + c0);
            y[0] = y[0] * (1.0f + sc.x) + sh.x; y[1] = y[1] * (1.0f + sc.y) + sh.y;
            y[2] = y[2] * (1.0f + sc.z) + sh.z; y[3] = y[3] * (1.0f + sc.w) + sh.w;
        }
        if (act == GVF_ACT_SILU) {
#pragma unroll
            for (int e = 0; e < 4; ++e) y[e] = y[e] / (1.0f + __expf(-y[e]));
        }
        uint2 o;
        o.x = GvfLp<DT>::pack(y[0], y[1]);
        o.y = GvfLp<DT>::pack(y[2], y[3]);
        *reinterpret_cast<uint2*>(out + (size_t)row * C + c0) = o;
    }
}

bool chan_ok(int c) { return c >= 64 && c <= CMAX && c % 64 == 0; }
bool dtype_ok(int dt) { return dt == GVF_DT_BF16 || dt == GVF_DT_F16; }
bool aligned(const void* p, uintptr_t a) { return ((uintptr_t)p & (a - 1)) == 0; }
bool rows_ok(int T) { return T >= 1 && (int64_t)T * NTAP <= 0x7fffffffll; }

}  // namespace

extern "C" int gvf_spconv_map_workspace_bytes(int T, size_t* out) {
    size_t slots;
    if (!out || !map_slots(T, slots)) return GVF_EINVAL;
    *out = slots * (sizeof(unsigned long long) + sizeof(int));
    return GVF_OK;
}

extern "C" int gvf_spconv_neighbor_map(const int32_t* coords, int T, int32_t* nbr, void* workspace, size_t workspace_bytes, void* stream) {
    size_t slots;
    if (!coords || !nbr || !workspace || !map_slots(T, slots)) return GVF_EINVAL;
    if (!aligned(coords, 16) || !aligned(nbr, 4) || !aligned(workspace, 256)) return GVF_EINVAL;
    if (workspace_bytes < slots * (sizeof(unsigned long long) + sizeof(int))) return GVF_ENOSPC;
    hipStream_t s = (hipStream_t)stream;
    unsigned long long* keys = (unsigned long long*)workspace;
    int* vals = (int*)(keys + slots);
    (void)hipGetLastError();
    if (hipMemsetAsync(keys, 0xff, slots * sizeof(unsigned long long), s) != hipSuccess) {
        (void)hipGetLastError();
        return GVF_ELAUNCH;
    }
    const unsigned mask = (unsigned)(slots - 1);
    map_insert_kernel<<<(unsigned)((T + NT - 1) / NT), NT, 0, s>>>((const int4*)coords, T, keys, vals, mask);
    GVF_CHECK_LAUNCH();
    const int64_t total = (int64_t)T * NTAP;
    map_lookup_kernel<<<(unsigned)((total + NT - 1) / NT), NT, 0, s>>>((const int4*)coords, T, keys, vals, mask, nbr);
    GVF_CHECK_LAUNCH();
    return GVF_OK;
}

extern "C" int gvf_spconv_packed_bytes(int cout, int cin, size_t* out) {
    if (!out || !chan_ok(cout) || !chan_ok(cin)) return GVF_EINVAL;
    *out = (size_t)cout * cin * NTAP * 2;
    return GVF_OK;
}

extern "C" int gvf_spconv_pack(const float* w, int cout, int cin, int dtype, void* out, size_t out_bytes, void* stream) {
    if (!w || !out || !dtype_ok(dtype) || !chan_ok(cout) || !chan_ok(cin) || !aligned(w, 4) || !aligned(out, 16)) return GVF_EINVAL;
    const size_t b = (size_t)cout * cin * NTAP * 2;
    if (out_bytes < b) return GVF_ENOSPC;
    const int64_t total = (int64_t)(b / 2);
    const int64_t want = (total + NT - 1) / NT;
    const unsigned blocks = (unsigned)(want < 8192 ? want : 8192);
    (void)hipGetLastError();
    GVF_LP_DISPATCH(dtype, (pack_kernel<DT><<<blocks, NT, 0, (hipStream_t)stream>>>(w, cin, (unsigned short*)out, total)));
    GVF_CHECK_LAUNCH();
    return GVF_OK;
}

namespace {
template <int DT, int AF>
void launch_conv(bool out32, dim3 grid, hipStream_t s, const void* in, int ld_in, const int32_t* nbr, const void* wimg, const float* bias,
                 const float* addend, void* out, int T, int cin, int cout) {
    if (out32)
        spconv3_kernel<DT, AF, true><<<grid, NT, 0, s>>>((const unsigned short*)in, ld_in, nbr, (const uint4*)wimg, bias, addend, out, T, cin, cout);
    else
        spconv3_kernel<DT, AF, false><<<grid, NT, 0, s>>>((const unsigned short*)in, ld_in, nbr, (const uint4*)wimg, bias, addend, out, T, cin, cout);
}
}  // namespace

extern "C" int gvf_spconv3(const void* in, int ld_in, const int32_t* nbr, const void* wimg, const float* bias, const float* addend, void* out,
                           int out_f32, int T, int cin, int cout, int dtype, void* stream) {
    if (!in || !nbr || !wimg || !out || !dtype_ok(dtype) || !chan_ok(cin) || !chan_ok(cout) || !rows_ok(T)) return GVF_EINVAL;
    if (ld_in < cin || ld_in % 8 != 0) return GVF_EINVAL;
    if (!aligned(in, 16) || !aligned(nbr, 4) || !aligned(wimg, 16) || !aligned(out, 16) || !aligned(bias, 16) || !aligned(addend, 16))
        return GVF_EINVAL;
    hipStream_t s = (hipStream_t)stream;
    const int af = cout % 256 == 0 ? 4 : (cout % 128 == 0 ? 2 : 1);
    const dim3 grid((unsigned)((T + TR - 1) / TR), (unsigned)(cout / (64 * af)));
    (void)hipGetLastError();
    GVF_LP_DISPATCH(dtype, {
        if (af == 4) launch_conv<DT, 4>(out_f32 != 0, grid, s, in, ld_in, nbr, wimg, bias, addend, out, T, cin, cout);
        else if (af == 2) launch_conv<DT, 2>(out_f32 != 0, grid, s, in, ld_in, nbr, wimg, bias, addend, out, T, cin, cout);
        else launch_conv<DT, 1>(out_f32 != 0, grid, s, in, ld_in, nbr, wimg, bias, addend, out, T, cin, cout);
    });
    GVF_CHECK_LAUNCH();
    return GVF_OK;
}

extern "C" int gvf_ln_act_rows(int dtype, const float* x, void* out16, int rows, int C, float eps, const float* ln_w, const float* ln_b,
                               const float* shift, const float* scale, int act, void* stream) {
    if (!x || !out16 || !dtype_ok(dtype) || rows < 1 || C < 4 || C > CMAX || C % 4 != 0 || !(eps >= 0.f)) return GVF_EINVAL;
    if ((ln_w == nullptr) != (ln_b == nullptr) || (shift == nullptr) != (scale == nullptr)) return GVF_EINVAL;
    if (act != GVF_ACT_NONE && act != GVF_ACT_SILU) return GVF_EINVAL;
    if (!aligned(x, 16) || !aligned(out16, 8) || !aligned(ln_w, 16) || !aligned(ln_b, 16) || !aligned(shift, 16) || !aligned(scale, 16))
        return GVF_EINVAL;
    hipStream_t s = (hipStream_t)stream;
    const dim3 grid((unsigned)((rows + 3) / 4));
    unsigned short* o = (unsigned short*)out16;
    (void)hipGetLastError();
    GVF_LP_DISPATCH(dtype, {
        if (C <= 256) ln_act_kernel<1, DT><<<grid, NT, 0, s>>>(x, o, rows, C, eps, ln_w, ln_b, shift, scale, act);
        else if (C <= 512) ln_act_kernel<2, DT><<<grid, NT, 0, s>>>(x, o, rows, C, eps, ln_w, ln_b, shift, scale, act);
        else if (C <= 1024) ln_act_kernel<4, DT><<<grid, NT, 0, s>>>(x, o, rows, C, eps, ln_w, ln_b, shift, scale, act);
        else ln_act_kernel<8, DT><<<grid, NT, 0, s>>>(x, o, rows, C, eps, ln_w, ln_b, shift, scale, act);
    });
    GVF_CHECK_LAUNCH();
    return GVF_OK;
}
