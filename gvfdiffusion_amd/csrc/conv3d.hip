// conv3d.hip -- dense 3x3x3 convolution (zero padding 1) on v_mfma_f32_16x16x32_{f16,bf16} with the pixel-shuffle of the sparse-structure
// decoder in its store, its weight image, and the occupancy read-out of the decoder's logits, gfx950.  C ABI, definition and layouts:
// include/gvf_conv3d.h.
//
// GEMM view, as spconv.hip: D[co][voxel] = sum_{ch, tap, ci} Wimg[co][ch, tap, ci] * halo[voxel + tap][32 ch + ci].  The WEIGHTS are the
// MFMA's A operand (rows = output channels), the voxels its B operand (columns): accumulator register r of lane l is output channel
// 4 (l / 16) + r of voxel l % 16, and output voxel n depends on column n of B alone -- a NaN stays in the outputs whose halo holds it.
//
// Tiling: a 256-thread workgroup owns a 4 x 4 x 4 brick of output voxels -- four B fragments, fragment j = the x-slice j, lane % 16 =
// 4 y + z inside it -- and a tile of output channels.  VF = 4 (wide Cout): wave w owns CF 16-channel A fragments and all four B fragments
// (a 64 CF channel tile per workgroup).  VF = 1 (Cout <= 32: the 64^3 layers, which are memory-bound): wave w owns B fragment w and all
// CF <= 2 A fragments, so no MFMA is spent beyond the padding of Cout to 16.  The walk is chunk-major: per 32-channel chunk the brick's
// 6 x 6 x 6 halo (216 cells x 64 B = 13.5 KiB) is loaded with 16-byte loads, four lanes per cell, into registers while the previous chunk
// is multiplied, and written to the other of two LDS buffers (one barrier per chunk); the 27 taps then read it with shifted addresses.  A
// halo cell outside the grid is a zero written to LDS, never a load.  The weight image is in fragment order (chunk-major, tap-minor), so
// an A fragment is one coalesced 1 KiB load and a wave walks its slice of the image front to back.
//
// LDS banking (ds_read_b128 is served in four groups of 16 lanes -- {0-3, 12-15, 20-27}, {4-11, 16-19, 28-31}, ... -- over 64 banks = 16
// slots of 16 B): a cell is 64 B, so piece p of cell c sits in slot 4 (c % 4) + p.  A group holds the lanes y in {0, 3} of piece P and
// y in {1, 2} of piece P ^ 1.  For one y the four z are four consecutive cells: all four values of c % 4.  So the four (y, piece) sets of
// a group each cover every c % 4, and the layout is conflict-free exactly when their four stored positions differ.  Piece p of halo cell
// (hx, hy, hz) is stored at position p ^ 2 (hy % 2): y in {0, 3} have different hy parity -> positions P and P ^ 2; y in {1, 2} likewise
// -> P ^ 1 and P ^ 3.  All four differ, for every tap.
#include "gvf_common.h"
#include "gvf_lp.h"
#include "../../include/gvf_rast.h"
#include "../../include/gvf_dit.h"
#include "../../include/gvf_conv3d.h"

namespace {

constexpr int NT = 256;
constexpr int NTAP = 27;
constexpr int CMAX = 2048;
constexpr int BR = 4;                   // brick edge
constexpr int HE = BR + 2;              // halo edge
constexpr int NCELL = HE * HE * HE;     // 216
constexpr int NPIECE = NCELL * 4;       // 864 16-byte pieces per chunk
constexpr int NIT = (NPIECE + NT - 1) / NT;
constexpr int OCC_ITEMS = 8;
constexpr int OCC_SPAN = NT * OCC_ITEMS;        // cells per workgroup of the occupancy kernels

// ---- weight image ------------------------------------------------------------------------------------------------------------------------
template <int DT>
__global__ __launch_bounds__(NT) void pack3d_kernel(const float* __restrict__ w, int cout, int cin, unsigned short* __restrict__ out,
                                                    int64_t total) {
    const int nch = (cin + 31) / 32;
    for (int64_t e = (int64_t)blockIdx.x * NT + threadIdx.x; e < total; e += (int64_t)gridDim.x * NT) {
        const int j = (int)(e & 7), lane = (int)((e >> 3) & 63);
        int64_t r = e >> 9;
        const int tap = (int)(r % NTAP);
        r /= NTAP;
        const int ch = (int)(r % nch), cb = (int)(r / nch);
        const int row = 16 * cb + (lane & 15), k = 32 * ch + 8 * (lane >> 4) + j;
        float v = 0.f;
        if (row < cout && k < cin) v = w[((int64_t)row * cin + k) * NTAP + tap];
        out[e] = GvfLp<DT>::to16(v);
    }
}

// ---- the convolution ---------------------------------------------------------------------------------------------------------------------
template <int DT, int CF, int VF>
__global__ __launch_bounds__(NT) void conv3d3_kernel(const unsigned short* __restrict__ in, int ld_in, const uint4* __restrict__ wimg,
                                                     const float* __restrict__ bias, const float* __restrict__ addend, void* __restrict__ out_,
                                                     int out32, int shuffle, int X, int Y, int Z, int nbx, int nby, int nbz, int nch, int ncb,
                                                     int cout) {
    typedef GvfLp<DT> L;
    typedef typename L::x8 x8;
    __shared__ uint4 s_h[2][NPIECE];        // 27 KiB
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int fi = lane & 15, fq = lane >> 4;
    const int vy = fi >> 2, vz = fi & 3;

    unsigned bid = blockIdx.x;
    const int iz = (int)(bid % (unsigned)nbz);
    bid /= (unsigned)nbz;
    const int iy = (int)(bid % (unsigned)nby);
    bid /= (unsigned)nby;
    const int ix = (int)(bid % (unsigned)nbx);
    const int b = (int)(bid / (unsigned)nbx);
    const int x0 = ix * BR, y0 = iy * BR, z0 = iz * BR;

    // the thread's pieces of a chunk: where they come from (-1: outside the grid, a zero) and where they go
    int64_t src[NIT];
    int dst[NIT];
#pragma unroll
    for (int it = 0; it < NIT; ++it) {
        const int idx = threadIdx.x + NT * it;
        src[it] = -1;
        dst[it] = -1;
        if (idx < NPIECE) {
            const int cell = idx >> 2, p = idx & 3;
            const int hx = cell / (HE * HE), hy = (cell / HE) % HE, hz = cell % HE;
            const int gx = x0 + hx - 1, gy = y0 + hy - 1, gz = z0 + hz - 1;
            dst[it] = cell * 4 + (p ^ ((hy & 1) << 1));
            if ((unsigned)gx < (unsigned)X && (unsigned)gy < (unsigned)Y && (unsigned)gz < (unsigned)Z)
                src[it] = ((((int64_t)b * X + gx) * Y + gy) * Z + gz) * ld_in + p * 8;
        }
    }
    auto gather = [&](int ch, uint4 (&v)[NIT]) {
#pragma unroll
        for (int it = 0; it < NIT; ++it) {
            v[it] = uint4{0u, 0u, 0u, 0u};
            if (src[it] >= 0) v[it] = *(const uint4*)(in + src[it] + ch * 32);
        }
    };
    auto stash = [&](int buf, const uint4 (&v)[NIT]) {
#pragma unroll
        for (int it = 0; it < NIT; ++it)
            if (dst[it] >= 0) s_h[buf][dst[it]] = v[it];
    };

    // VF = 4: the wave's CF channel fragments, every x-slice.  VF = 1: every channel fragment of the tile, the wave's x-slice.
    const int cb0 = VF == 4 ? (blockIdx.y * 4 + wave) * CF : blockIdx.y * CF;
    const bool active = cb0 < ncb && (VF == 4 || x0 + wave < X);
    int cbs[CF];
#pragma unroll
    for (int i = 0; i < CF; ++i) cbs[i] = cb0 + i < ncb ? cb0 + i : ncb - 1;      // a fragment beyond Cout: a valid address, never stored

    gvf_f32x4 acc[CF][VF];
#pragma unroll
    for (int i = 0; i < CF; ++i)
#pragma unroll
        for (int j = 0; j < VF; ++j) acc[i][j] = gvf_f32x4{0.f, 0.f, 0.f, 0.f};

    // B fragment address of tap (kx, ky, kz), x-slice vx: cell ((vx + kx) HE + vy + ky) HE + vz + kz, position fq ^ 2 ((vy + ky) % 2)
    const int cell0 = (vy * HE + vz) * 4;
    const int pos_even = fq ^ ((vy & 1) << 1), pos_odd = pos_even ^ 2;

    uint4 v[NIT];
    gather(0, v);
    stash(0, v);
    __syncthreads();
    int buf = 0;
    for (int ch = 0; ch < nch; ++ch) {
        const bool more = ch + 1 < nch;
        if (more) gather(ch + 1, v);
        if (active) {
#pragma unroll
            for (int tap = 0; tap < NTAP; ++tap) {
                const int kx = tap / 9, ky = (tap / 3) % 3, kz = tap % 3;
                x8 a[CF], bf[VF];
#pragma unroll
                for (int i = 0; i < CF; ++i) a[i] = __builtin_bit_cast(x8, wimg[(((int64_t)cbs[i] * nch + ch) * NTAP + tap) * 64 + lane]);
#pragma unroll
                for (int j = 0; j < VF; ++j) {
                    const int vx = VF == 4 ? j : wave;
                    const int u = cell0 + (((vx + kx) * HE + ky) * HE + kz) * 4 + ((ky & 1) ? pos_odd : pos_even);
                    bf[j] = __builtin_bit_cast(x8, s_h[buf][u]);
                }
#pragma unroll
                for (int i = 0; i < CF; ++i)
#pragma unroll
                    for (int j = 0; j < VF; ++j) acc[i][j] = L::mfma16(a[i], bf[j], acc[i][j]);
            }
        }
        if (more) stash(buf ^ 1, v);
        __syncthreads();
        buf ^= 1;
    }
    if (!active) return;

    const int gy = y0 + vy, gz = z0 + vz;
    if (gy >= Y || gz >= Z) return;
    const bool vec = !shuffle && (cout & 3) == 0;
    const int cq = cout >> 3;
#pragma unroll
    for (int j = 0; j < VF; ++j) {
        const int gx = x0 + (VF == 4 ? j : wave);
        if (gx >= X) continue;
        const int64_t row = (((int64_t)b * X + gx) * Y + gy) * Z + gz;
#pragma unroll
        for (int i = 0; i < CF; ++i) {
            if (cb0 + i >= ncb) continue;
            const int co = 16 * (cb0 + i) + 4 * fq;
            if (co >= cout) continue;
            float f[4] = {acc[i][j][0], acc[i][j][1], acc[i][j][2], acc[i][j][3]};
            if (vec) {
                const int64_t o = row * cout + co;
                if (bias) {
                    const float4 b4 = *(const float4*)(bias + co);
                    f[0] += b4.x; f[1] += b4.y; f[2] += b4.z; f[3] += b4.w;
                }
                if (addend) {
                    const float4 a4 = *(const float4*)(addend + o);
                    f[0] += a4.x; f[1] += a4.y; f[2] += a4.z; f[3] += a4.w;
                }
                if (out32) {
                    *(float4*)((float*)out_ + o) = float4{f[0], f[1], f[2], f[3]};
                } else {
                    uint2 w2;
                    w2.x = L::pack(f[0], f[1]);
                    w2.y = L::pack(f[2], f[3]);
                    *(uint2*)((unsigned short*)out_ + o) = w2;
                }
                continue;
            }
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int c = co + r;
                if (c >= cout) continue;
                int64_t o = row * cout + c;
                if (shuffle)        // channel c = ((c' 2 + i) 2 + j) 2 + k -> channel c' of voxel (2x + i, 2y + j, 2z + k)
                    o = ((((int64_t)b * (2 * X) + 2 * gx + ((c >> 2) & 1)) * (2 * Y) + 2 * gy + ((c >> 1) & 1)) * (2 * Z) + 2 * gz + (c & 1)) * cq + (c >> 3);
                float t = f[r];
                if (bias) t += bias[c];
                if (addend) t += addend[o];
                if (out32) ((float*)out_)[o] = t;
                else ((unsigned short*)out_)[o] = L::to16(t);
            }
        }
    }
}

// ---- occupancy ---------------------------------------------------------------------------------------------------------------------------
// three launches: per-workgroup counts, one exclusive scan of them, ordered writes.  A workgroup spans OCC_SPAN consecutive cells, taken in
// OCC_ITEMS passes of 256 so that thread order is row order inside a pass.
__device__ __forceinline__ bool occupied(const float* __restrict__ logits, int64_t i, int64_t cells) { return i < cells && logits[i] > 0.f; }

__global__ __launch_bounds__(NT) void occ_count_kernel(const float* __restrict__ logits, int64_t cells, int* __restrict__ counts) {
    __shared__ int s_n[NT / 64];
    const int64_t base = (int64_t)blockIdx.x * OCC_SPAN;
    int n = 0;
#pragma unroll
    for (int it = 0; it < OCC_ITEMS; ++it) n += __popcll(__ballot(occupied(logits, base + it * NT + threadIdx.x, cells)));
    if ((threadIdx.x & 63) == 0) s_n[threadIdx.x >> 6] = n;
    __syncthreads();
    if (threadIdx.x == 0) counts[blockIdx.x] = s_n[0] + s_n[1] + s_n[2] + s_n[3];
}

// one workgroup: thread t sums its contiguous segment, thread 0 scans the 256 sums, every thread rewrites its segment as offsets
__global__ __launch_bounds__(NT) void occ_scan_kernel(int* __restrict__ counts, int nblk, int* __restrict__ total) {
    __shared__ int s_part[NT];
    const int seg = (nblk + NT - 1) / NT;
    const int lo = min((int)threadIdx.x * seg, nblk), hi = min(lo + seg, nblk);
    int s = 0;
    for (int i = lo; i < hi; ++i) s += counts[i];
    s_part[threadIdx.x] = s;
    __syncthreads();
    if (threadIdx.x == 0) {
        int run = 0;
        for (int i = 0; i < NT; ++i) {
            const int c = s_part[i];
            s_part[i] = run;
            run += c;
        }
        *total = run;
    }
    __syncthreads();
    int run = s_part[threadIdx.x];
    for (int i = lo; i < hi; ++i) {
        const int c = counts[i];
        counts[i] = run;
        run += c;
    }
}

__global__ __launch_bounds__(NT) void occ_write_kernel(const float* __restrict__ logits, int64_t cells, int X, int Y, int Z,
                                                       const int* __restrict__ offsets, int4* __restrict__ coords) {
    __shared__ int s_n[2][NT / 64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t base = (int64_t)blockIdx.x * OCC_SPAN;
    int run = offsets[blockIdx.x];
#pragma unroll
    for (int it = 0; it < OCC_ITEMS; ++it) {
        const int64_t i = base + it * NT + threadIdx.x;
        const bool occ = occupied(logits, i, cells);
        const unsigned long long m = __ballot(occ);
        if (lane == 0) s_n[it & 1][wave] = __popcll(m);
        __syncthreads();                    // the other half of s_n was last read before the previous pass's barrier
        int before = 0, all = 0;
#pragma unroll
        for (int w = 0; w < NT / 64; ++w) {
            const int c = s_n[it & 1][w];
            before += w < wave ? c : 0;
            all += c;
        }
        if (occ) {
            const int at = run + before + __popcll(m & ((1ull << lane) - 1ull));
            int64_t r = i;
            const int z = (int)(r % Z);
            r /= Z;
            const int y = (int)(r % Y);
            r /= Y;
            coords[at] = int4{(int)(r / X), (int)(r % X), y, z};
        }
        run += all;
    }
}

bool chan_ok(int c) { return c >= 1 && c <= CMAX; }
bool dtype_ok(int dt) { return dt == GVF_DT_BF16 || dt == GVF_DT_F16; }
bool aligned(const void* p, uintptr_t a) { return ((uintptr_t)p & (a - 1)) == 0; }
// B X Y Z (times `mul`) with 27 x it below 2^31; 0 when the sizes are bad
int64_t grid_rows(int B, int X, int Y, int Z, int mul) {
    if (B < 1 || X < 1 || Y < 1 || Z < 1) return 0;
    const int64_t lim = 0x7fffffffll / NTAP;
    int64_t n = mul;
    for (int d : {B, X, Y, Z}) {
        n *= d;
        if (n > lim) return 0;
    }
    return n;
}
size_t image_bytes(int cout, int cin) { return (size_t)((cout + 15) / 16 * 16) * (size_t)((cin + 31) / 32 * 32) * NTAP * 2; }

template <int DT, int CF, int VF>
void launch_conv(dim3 grid, hipStream_t s, const void* in, int ld_in, const void* wimg, const float* bias, const float* addend, void* out,
                 int out32, int shuffle, int X, int Y, int Z, int nbx, int nby, int nbz, int nch, int ncb, int cout) {
    conv3d3_kernel<DT, CF, VF><<<grid, NT, 0, s>>>((const unsigned short*)in, ld_in, (const uint4*)wimg, bias, addend, out, out32, shuffle, X, Y,
                                                   Z, nbx, nby, nbz, nch, ncb, cout);
}

}  // namespace

extern "C" int gvf_conv3d3_packed_bytes(int cout, int cin, size_t* out) {
    if (!out || !chan_ok(cout) || !chan_ok(cin)) return GVF_EINVAL;
    *out = image_bytes(cout, cin);
    return GVF_OK;
}

extern "C" int gvf_conv3d3_pack(const float* w, int cout, int cin, int dtype, void* out, size_t out_bytes, void* stream) {
    if (!w || !out || !dtype_ok(dtype) || !chan_ok(cout) || !chan_ok(cin) || !aligned(w, 4) || !aligned(out, 16)) return GVF_EINVAL;
    const size_t b = image_bytes(cout, cin);
    if (out_bytes < b) return GVF_ENOSPC;
    const int64_t total = (int64_t)(b / 2);
    const int64_t want = (total + NT - 1) / NT;
    const unsigned blocks = (unsigned)(want < 8192 ? want : 8192);
    (void)hipGetLastError();
    GVF_LP_DISPATCH(dtype, (pack3d_kernel<DT><<<blocks, NT, 0, (hipStream_t)stream>>>(w, cout, cin, (unsigned short*)out, total)));
    GVF_CHECK_LAUNCH();
    return GVF_OK;
}

extern "C" int gvf_conv3d3(const void* in, int ld_in, const void* wimg, const float* bias, const float* addend, void* out, int out_f32,
                           int store, int B, int X, int Y, int Z, int cin, int cout, int dtype, void* stream) {
    if (!in || !wimg || !out || !dtype_ok(dtype) || !chan_ok(cin) || !chan_ok(cout)) return GVF_EINVAL;
    if (store != GVF_CONV3D_STORE_ROWS && store != GVF_CONV3D_STORE_SHUFFLE2) return GVF_EINVAL;
    const int shuffle = store == GVF_CONV3D_STORE_SHUFFLE2;
    if (shuffle && cout % 8 != 0) return GVF_EINVAL;
    if (grid_rows(B, X, Y, Z, shuffle ? 8 : 1) == 0) return GVF_EINVAL;
    const int nch = (cin + 31) / 32, ncb = (cout + 15) / 16;
    if (ld_in < nch * 32 || ld_in % 8 != 0) return GVF_EINVAL;
    if (!aligned(in, 16) || !aligned(wimg, 16) || !aligned(out, 16) || !aligned(bias, 16) || !aligned(addend, 16)) return GVF_EINVAL;
    const int nbx = (X + BR - 1) / BR, nby = (Y + BR - 1) / BR, nbz = (Z + BR - 1) / BR;
    const int64_t bricks = (int64_t)B * nbx * nby * nbz;
    // channel fragments per wave: as many as keep 256 workgroups in the launch (the card's compute units), the narrow layers by x-slice
    int cf, vf = 4;
    if (ncb <= 2) {
        cf = ncb;
        vf = 1;
    } else {
        cf = ncb <= 4 ? 1 : (ncb <= 8 ? 2 : 4);
        while (cf > 1 && bricks * ((ncb + 4 * cf - 1) / (4 * cf)) < 256) cf >>= 1;
    }
    const dim3 grid((unsigned)bricks, (unsigned)(vf == 1 ? 1 : (ncb + 4 * cf - 1) / (4 * cf)));
    hipStream_t s = (hipStream_t)stream;
    (void)hipGetLastError();
#define GVF_CONV3D_GO(CF_, VF_) \
    launch_conv<DT, CF_, VF_>(grid, s, in, ld_in, wimg, bias, addend, out, out_f32 != 0, shuffle, X, Y, Z, nbx, nby, nbz, nch, ncb, cout)
    GVF_LP_DISPATCH(dtype, {
        if (vf == 1 && cf == 1) GVF_CONV3D_GO(1, 1);
        else if (vf == 1) GVF_CONV3D_GO(2, 1);
        else if (cf == 1) GVF_CONV3D_GO(1, 4);
        else if (cf == 2) GVF_CONV3D_GO(2, 4);
        else GVF_CONV3D_GO(4, 4);
    });
#undef GVF_CONV3D_GO
    GVF_CHECK_LAUNCH();
    return GVF_OK;
}

extern "C" int gvf_occupancy_workspace_bytes(int64_t cells, size_t* out) {
    if (!out || cells < 1 || cells > 0x7fffffffll / NTAP) return GVF_EINVAL;
    *out = (size_t)((cells + OCC_SPAN - 1) / OCC_SPAN) * sizeof(int);
    return GVF_OK;
}

extern "C" int gvf_occupancy_coords(const float* logits, int B, int X, int Y, int Z, int32_t* coords, int64_t capacity, int32_t* count,
                                    void* workspace, size_t workspace_bytes, void* stream) {
    const int64_t cells = grid_rows(B, X, Y, Z, 1);
    if (!logits || !coords || !count || !workspace || cells == 0) return GVF_EINVAL;
    if (!aligned(logits, 4) || !aligned(coords, 16) || !aligned(count, 4) || !aligned(workspace, 256)) return GVF_EINVAL;
    const int nblk = (int)((cells + OCC_SPAN - 1) / OCC_SPAN);
    if (capacity < cells || workspace_bytes < (size_t)nblk * sizeof(int)) return GVF_ENOSPC;
    hipStream_t s = (hipStream_t)stream;
    int* counts = (int*)workspace;
    (void)hipGetLastError();
    occ_count_kernel<<<(unsigned)nblk, NT, 0, s>>>(logits, cells, counts);
    GVF_CHECK_LAUNCH();
    occ_scan_kernel<<<1, NT, 0, s>>>(counts, nblk, count);
    GVF_CHECK_LAUNCH();
    occ_write_kernel<<<(unsigned)nblk, NT, 0, s>>>(logits, cells, X, Y, Z, counts, (int4*)coords);
    GVF_CHECK_LAUNCH();
    return GVF_OK;
}
