// linear_grad.hip -- a projection's backward: the weight gradient dW = dY^T X (+ db = column sums of dY) and the transposing cast of the fp32
// master weight (include/gvf_linear_grad.h).  The forward and the input gradient are gvf_gemm (gemm.hip) on the two images the cast writes.
//
// Weight gradient: both operands have the contraction index m as their slow axis.  A workgroup (4 waves as 2 x 2, each 64 x 64 of a 128 x 128 tile
// of dW, 4 x 4 accumulators of the 16x16x32 MFMA) stages BM = 64 rows of dY [m][n0 .. n0 + 128) and of X [m][k0 .. k0 + 128) ROW-MAJOR into LDS
// -- 16 bytes per lane, 16 lanes per 256-byte row, the next stage's loads in flight in registers while this one is multiplied -- and reads the
// fragments column-wise with ds_read_b64_tr_b16: per 16-lane group a block of 4 rows x 16 columns, lane i of the group receiving column i.
// MFMA slot 8 g + e of lane group g holds row 4 g + e (e < 4) and row 16 + 4 g + (e - 4) of the k-step's 32 rows, in BOTH operands (the order
// in which m fills the contraction slots is free as long as the operands agree), so that the two groups of a 32-lane half read 8 CONSECUTIVE
// rows of the same 16 columns.  LDS rows are LD = 144 elements = 288 bytes = 72 banks apart: row r starts at bank 8 r (mod 64), a lane covers
// 2 banks, the 4 lanes of a row 8, the 8 rows of a half all 64 -- conflict-free by the bank rule of the transposed read ((address / 4) % 64 per
// 32-lane half).  Every lane always reads inside the tile (EXEC all ones); what lies past M, N or K is zero in the tile and never loaded
// (the load's address is clamped into the operand, its value replaced by zero).
//
// Split over m and the reduction: see the header.  One k-step = one MFMA per accumulator = one fp32 rounding of the running sum.
#include "gvf_common.h"
#include "gvf_lp.h"
#include "gvf_rowops.h"
#include "../../include/gvf_rast.h"
#include "../../include/gvf_dit.h"
#include "../../include/gvf_linear_grad.h"

namespace {

constexpr int BT = 128;          // edge of the output tile (n and k)
constexpr int BM = 64;           // rows of m per stage: two 32-row k-steps
constexpr int LD = 144;          // LDS row stride in 16-bit elements (288 bytes)
constexpr int KSTEP = 32;        // rows of one MFMA k-step
constexpr int WGRAD_CUS = 256;   // the MI355X's CU count: the automatic split aims at two workgroups per CU (3 fit: 158 VGPRs, 36 KiB of LDS) ...
constexpr int WGRAD_MAX_AUTO = 16;   // ... over at most 16 slots (beyond, the reducer's traffic costs more than the occupancy returns: measured) ...
constexpr int WGRAD_MIN_STEPS = 8;   // ... of at least 8 k-steps each
constexpr int WGRAD_MAX_SPLITS = 65535;

typedef __attribute__((ext_vector_type(4))) short s16x4;
typedef __attribute__((address_space(3))) s16x4 lds_s16x4;

// The fragment of the k-step whose first row is at `p` (this lane's block address: row 4 g + q, columns 4 p .. 4 p + 3)
template <int DT>
__device__ __forceinline__ typename GvfLp<DT>::x8 tr_fragment(const unsigned short* p) {
    const s16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4*)p);
    const s16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4*)(p + 16 * LD));
    return __builtin_bit_cast(typename GvfLp<DT>::x8, __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7));
}

// 16 bytes of row `row`, columns col .. col + 7 of a [rows][cols] operand, zeros outside it (extent a multiple of 8: a chunk is inside or outside)
__device__ __forceinline__ uint4 load_chunk(const unsigned short* __restrict__ base, int ld, int row, int row_end, int col, int cols) {
    const bool ok = row < row_end && col < cols;
    const uint4 v = *reinterpret_cast<const uint4*>(base + (size_t)(ok ? row : row_end - 1) * ld + (ok ? col : 0));
    return ok ? v : make_uint4(0u, 0u, 0u, 0u);
}

template <int DT>
__global__ __launch_bounds__(256) void wgrad_partial_kernel(const unsigned short* __restrict__ dY, int ldy, const unsigned short* __restrict__ X,
                                                            int ldx, int M, int N, int K, int steps_per_group, float* __restrict__ ws,
                                                            long long slot_stride, int want_db) {
    using L = GvfLp<DT>;
    using x8 = typename L::x8;
    __shared__ __attribute__((aligned(16))) unsigned short lds[2 * BM * LD];
    unsigned short* const sY = lds;
    unsigned short* const sX = lds + BM * LD;

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wr = wave >> 1, wc = wave & 1;
    const int k0 = blockIdx.x * BT, n0 = blockIdx.y * BT;
    const long long mb = (long long)blockIdx.z * steps_per_group * KSTEP;
    const int m_begin = mb < M ? (int)mb : M;
    const int m_end = mb + (long long)steps_per_group * KSTEP < M ? (int)(mb + (long long)steps_per_group * KSTEP) : M;
    const bool do_db = want_db != 0 && blockIdx.x == 0 && wc == 0;

    // staging: 16 lanes per row, rows srow + 16 i
    const int schunk = (tid & 15) * 8, srow = tid >> 4;
    uint4 py[4], px[4];
    auto fetch = [&](int m) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            py[i] = load_chunk(dY, ldy, m + srow + 16 * i, m_end, n0 + schunk, N);
            px[i] = load_chunk(X, ldx, m + srow + 16 * i, m_end, k0 + schunk, K);
        }
    };

    gvf_f32x4 acc[4][4];
    gvf_f32x4 dbacc[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        dbacc[i] = gvf_f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = gvf_f32x4{0.f, 0.f, 0.f, 0.f};
    }
    const x8 ones = __builtin_bit_cast(x8, make_uint4(L::ONE2, L::ONE2, L::ONE2, L::ONE2));

    // this lane's block address inside a k-step: row 4 g + q, columns 4 p .. 4 p + 3 (g = lane / 16, q = (lane / 4) % 4, p = lane % 4)
    const int frag_off = (4 * (lane >> 4) + ((lane >> 2) & 3)) * LD + 4 * (lane & 3);
    const unsigned short* const fY = sY + frag_off + wr * 64;
    const unsigned short* const fX = sX + frag_off + wc * 64;

    if (m_begin < m_end) fetch(m_begin);
    for (int m = m_begin; m < m_end; m += BM) {
        __syncthreads();                                      // the previous stage's fragment reads are done
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            *reinterpret_cast<uint4*>(sY + (srow + 16 * i) * LD + schunk) = py[i];
            *reinterpret_cast<uint4*>(sX + (srow + 16 * i) * LD + schunk) = px[i];
        }
        __syncthreads();
        if (m + BM < m_end) fetch(m + BM);                    // in flight while this stage is multiplied
#pragma unroll
        for (int s = 0; s < BM / KSTEP; ++s) {
            if (m + s * KSTEP >= m_end) break;                // (uniform: a stage's second k-step past the group's rows is all zeros)
            x8 a[4], b[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) a[i] = tr_fragment<DT>(fY + s * KSTEP * LD + 16 * i);
#pragma unroll
            for (int j = 0; j < 4; ++j) b[j] = tr_fragment<DT>(fX + s * KSTEP * LD + 16 * j);
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int j = 0; j < 4; ++j) acc[i][j] = L::mfma16(a[i], b[j], acc[i][j]);
            if (do_db) {
#pragma unroll
                for (int i = 0; i < 4; ++i) dbacc[i] = L::mfma16(a[i], ones, dbacc[i]);
            }
        }
    }

    // the partial tile into this group's slot: accumulator register r of lane l is row 4 (l / 16) + r, column l % 16 of its 16 x 16 block
    float* const slot = ws + (size_t)blockIdx.z * (size_t)slot_stride;
    const int fr = lane & 15, fq = lane >> 4;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int n = n0 + wr * 64 + 16 * i + 4 * fq + r;
            if (n >= N) continue;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int k = k0 + wc * 64 + 16 * j + fr;
                if (k < K) slot[(size_t)n * K + k] = acc[i][j][r];
            }
            if (do_db && fr == 0) slot[(size_t)N * K + n] = dbacc[i][r];      // (every column of the product with ones is the row sum)
        }
    }
}

// dW (and db) = the slots added in ascending order; four consecutive elements per thread (K % 4 == 0: they never straddle a row of dW)
__global__ __launch_bounds__(256) void wgrad_reduce_kernel(const float* __restrict__ ws, long long slot_stride, int splits, float* __restrict__ dW,
                                                           int lddw, float* __restrict__ db, int N, int K) {
    const long long nk = (long long)N * K;
    const long long total = nk + (db != nullptr ? N : 0);
    const long long e = ((long long)blockIdx.x * 256 + threadIdx.x) * 4;
    if (e >= total) return;
    float4 s = *reinterpret_cast<const float4*>(ws + e);
    for (int g = 1; g < splits; ++g) {
        const float4 v = *reinterpret_cast<const float4*>(ws + (size_t)g * (size_t)slot_stride + e);
        s.x += v.x;
        s.y += v.y;
        s.z += v.z;
        s.w += v.w;
    }
    if (e < nk) {
        const long long n = e / K;
        *reinterpret_cast<float4*>(dW + n * lddw + (e - n * K)) = s;
    } else {
        *reinterpret_cast<float4*>(db + (e - nk)) = s;
    }
}

// One 64 x 64 tile of the master per workgroup: rounded once, stored row-major as it is read and, through LDS, transposed.  Lane pairs of columns:
// every global store is 4 bytes per lane, 128 contiguous bytes per 32 lanes.  Tile rows are 65 elements apart: the transposed read of rows 2 c,
// 2 c + 1 (c = 0 .. 31) at one column lands on 32 distinct banks.
template <int DT>
__global__ __launch_bounds__(256) void cast_transpose_kernel(const float* __restrict__ W, long long ldw, unsigned short* __restrict__ W16,
                                                             long long ld_k, unsigned short* __restrict__ W16T, long long ld_n, int N, int K) {
    using L = GvfLp<DT>;
    __shared__ unsigned short tile[64][65];
    const int n0 = blockIdx.y * 64, k0 = blockIdx.x * 64;
    const int c2 = threadIdx.x & 31, r = threadIdx.x >> 5;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        const int row = r + 8 * i, n = n0 + row, k = k0 + 2 * c2;
        float v0 = 0.f, v1 = 0.f;
        if (n < N) {
            if (k < K) v0 = W[n * ldw + k];
            if (k + 1 < K) v1 = W[n * ldw + k + 1];
        }
        const unsigned pk = L::pack(v0, v1);
        tile[row][2 * c2] = (unsigned short)(pk & 0xffffu);
        tile[row][2 * c2 + 1] = (unsigned short)(pk >> 16);
        if (n < N && k < ld_k) *reinterpret_cast<unsigned*>(W16 + n * ld_k + k) = pk;       // (k and ld_k even: the pair is inside or outside)
    }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        const int kk = r + 8 * i, k = k0 + kk, n = n0 + 2 * c2;
        const unsigned pk = (unsigned)tile[2 * c2][kk] | ((unsigned)tile[2 * c2 + 1][kk] << 16);
        if (k < K && n < ld_n) *reinterpret_cast<unsigned*>(W16T + k * ld_n + n) = pk;
    }
}


inline long long slot_floats(int N, int K) { return (long long)N * K + N; }

}  // namespace

extern "C" int gvf_cast_transpose(int dtype, const float* W, int ldw, void* W16, int ld_k, void* W16T, int ld_n, int N, int K, void* stream_) {
    if (!gvf_lp_ok(dtype)) return GVF_EINVAL;
    if (N <= 0 || K <= 0 || ldw < K || ld_k < K || ld_n < N || (ld_k % 8) != 0 || (ld_n % 8) != 0) return GVF_EINVAL;
    if (!W || !W16 || !W16T) return GVF_EINVAL;
    if (gvf_mis(W, 3) || gvf_mis(W16, 3) || gvf_mis(W16T, 3)) return GVF_EINVAL;
    (void)hipGetLastError();
    const dim3 grid((unsigned)gvf_cdiv(ld_k, 64), (unsigned)gvf_cdiv(ld_n, 64));
    if (grid.y > 65535u) return GVF_EINVAL;
    GVF_LP_DISPATCH(dtype, hipLaunchKernelGGL(cast_transpose_kernel<DT>, grid, dim3(256), 0, (hipStream_t)stream_, W, (long long)ldw,
                                              (unsigned short*)W16, (long long)ld_k, (unsigned short*)W16T, (long long)ld_n, N, K));
    GVF_CHECK_LAUNCH();
    return GVF_OK;
}

extern "C" int gvf_gemm_wgrad_splits(int M, int N, int K) {
    if (M < 0 || N <= 0 || K <= 0) return GVF_EINVAL;
    const long long tiles = gvf_cdiv(N, BT) * gvf_cdiv(K, BT);
    const long long steps = gvf_cdiv(M, KSTEP);
    long long s = 2 * WGRAD_CUS / tiles;
    if (s > WGRAD_MAX_AUTO) s = WGRAD_MAX_AUTO;
    if (s > steps / WGRAD_MIN_STEPS) s = steps / WGRAD_MIN_STEPS;
    return s < 1 ? 1 : (int)s;
}

extern "C" int gvf_gemm_wgrad_workspace_bytes(int M, int N, int K, int splits, size_t* out) {
    if (!out || M < 0 || N <= 0 || K <= 0 || splits < 0 || splits > WGRAD_MAX_SPLITS) return GVF_EINVAL;
    if (splits == 0) splits = gvf_gemm_wgrad_splits(M, N, K);
    *out = gvf_align_up((size_t)splits * (size_t)slot_floats(N, K) * sizeof(float), 256);
    return GVF_OK;
}

extern "C" int gvf_gemm_wgrad(int dtype, const void* dY, int ldy, const void* X, int ldx, int M, int N, int K, float* dW, int lddw, float* db,
                              void* workspace, size_t workspace_bytes, int splits, void* stream_) {
    if (!gvf_lp_ok(dtype)) return GVF_EINVAL;
    if (M < 0 || N <= 0 || K <= 0 || (N % 8) != 0 || (K % 8) != 0) return GVF_EINVAL;
    if (ldy < N || ldx < K || lddw < K || (ldy % 8) != 0 || (ldx % 8) != 0 || (lddw % 8) != 0) return GVF_EINVAL;
    if (splits < 0 || splits > WGRAD_MAX_SPLITS) return GVF_EINVAL;
    if (!dY || !X || !dW || !workspace) return GVF_EINVAL;
    if (gvf_mis(dY, 15) || gvf_mis(X, 15) || gvf_mis(dW, 15) || gvf_mis(db, 15) || gvf_mis(workspace, 15)) return GVF_EINVAL;
    if (splits == 0) splits = gvf_gemm_wgrad_splits(M, N, K);
    size_t need = 0;
    if (gvf_gemm_wgrad_workspace_bytes(M, N, K, splits, &need) != GVF_OK || workspace_bytes < need) return GVF_EINVAL;
    const long long tiles_n = gvf_cdiv(N, BT), tiles_k = gvf_cdiv(K, BT);
    if (tiles_n > 65535) return GVF_EINVAL;
    const int steps_per_group = (int)gvf_cdiv(gvf_cdiv(M, KSTEP), splits);
    hipStream_t stream = (hipStream_t)stream_;
    (void)hipGetLastError();
    float* ws = (float*)workspace;
    GVF_LP_DISPATCH(dtype, hipLaunchKernelGGL(wgrad_partial_kernel<DT>, dim3((unsigned)tiles_k, (unsigned)tiles_n, (unsigned)splits), dim3(256), 0,
                                              stream, (const unsigned short*)dY, ldy, (const unsigned short*)X, ldx, M, N, K, steps_per_group, ws,
                                              slot_floats(N, K), db != nullptr ? 1 : 0));
    GVF_CHECK_LAUNCH();
    const long long total4 = (slot_floats(N, K) - (db != nullptr ? 0 : N)) / 4;
    hipLaunchKernelGGL(wgrad_reduce_kernel, dim3((unsigned)gvf_cdiv(total4, 256)), dim3(256), 0, stream, ws, slot_floats(N, K), splits, dW, lddw, db, N,
                       K);
    GVF_CHECK_LAUNCH();
    return GVF_OK;
}
