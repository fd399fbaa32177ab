// attn_bwd.hip -- flash attention backward (dQ, dK, dV of softmax(q k^T * scale) v), head_dim 32 or 64, fp16 / bf16 operands, gfx950.
//
// The gradient of the operator seam model/attention/full_attn.py (ops/attention_grad.py).  csrc/attn.hip keeps neither the scores nor
// the row statistics, so the backward starts with a statistics pass of its own and recomputes P from Q, K and a per-row log-sum-exp:
//
//   stats  : per query row  lse2 = log2 sum_k exp2(c s_k)  (c = scale * log2 e, online maximum over 32-key tiles) and
//            delta = sum_d dO_d O_d  (O: the forward's rounded output), both fp32 (N, H, Lq) in the caller's workspace.
//   sweep K: a workgroup owns 128 keys (a wave 32) and sweeps the queries in 32-row tiles; dK^T and dV^T stay in accumulators.
//            With few key blocks and many queries the query range is split over several workgroups per key block (a function of
//            the shape alone), whose fp32 partials one more kernel sums in chunk order.
//   sweep Q: a workgroup owns 128 queries and sweeps the keys in 32-row tiles; dQ^T stays in accumulators.
//
// Both sweeps are ONE kernel template.  The owned rows x sit on the MFMA lane (their fragments live in registers as B operands),
// the streamed rows y are staged through LDS and arrive as A operands, so a 32x32 accumulator holds [y in the 16 registers][x on
// the lane]:   S = Y1 X1^T, dP = Y2 X2^T  with (X1, X2, Y1, Y2) = (K, V, Q, dO) in sweep K and (Q, dO, K, V) in sweep Q.
// The accumulators start at -lse2 / c and -delta of their query (a per-register row constant in sweep K, a per-lane one in sweep
// Q), so p = exp2(c S') and dS = p dP' scale need no subtraction.  P and dS, rounded to the operand type, are already the B operands
// of the products that sum over y:  dV^T += dO^T P,  dK^T += Q^T dS  (sweep K),  dQ^T += K^T dS^T  (sweep Q); their A operands are
// read from a transposed LDS image of the same staged tile, contraction slots permuted to the accumulator's row order.
//
// Rounding points (flash-attn's): scores and dP fp32 from 16-bit operands; p fp32, rounded to 16 bit where it feeds dV; dS rounded
// to 16 bit where it feeds dQ and dK; fp32 accumulation; gradients stored in the operand type.
// Determinism: every gradient element is summed by one wave in tile order; no atomics, no workgroup waits on another.
// Short sequences (Lq, Lk <= 32, head_dim 32: the DiT's temporal attention): one wave per (sequence, head) problem, everything in
// registers and a per-wave LDS slab, no workspace.
// Ragged form (gvf_attn_varlen_bwd: packed [T, H, C] tensors, device cu_seqlens, the sparse seam sparse/attention/full_attn.py): the same
// three kernels, instantiated with VARLEN.  Only the problem decode differs (problem_of): a workgroup reads its sequence's row base and
// lengths from cu_seqlens, the grids are sized from the longest lengths, and a workgroup whose owned block lies past its sequence
// leaves before the first barrier.  No length crosses to the host; the split rule sees the host-known arguments only.
#include <cstdlib>
#include "gvf_common.h"
#include "gvf_lp.h"
#include "../../include/gvf_rast.h"
#include "../../include/gvf_dit.h"
#include "../../include/gvf_attn_bwd.h"

namespace {

typedef gvf_f32x16 f32x16;

constexpr int XB = 128;          // owned rows per workgroup (32 per wave)
constexpr int YT = 32;           // streamed rows per staged tile
constexpr int THREADS = 256;
constexpr int TLD = YT + 4;      // row stride (16-bit elements) of a transposed tile [d][y]: rows stay 8-byte aligned
constexpr int SM_LD = 36;        // row stride of the short-sequence kernel's staged rows

struct BwdParams {
    const unsigned short *q, *k, *v, *o, *dout;
    unsigned short *dq, *dk, *dv;
    float *lse2, *delta;
    float* part;                     // key sweep split over the queries: fp32 partial dK, dV [2][n_split][N H][Lk][D]
    int n_outer, n_inner, Lq, Lk, H, x_blocks, n_split;    // ragged: n_outer sequences, n_inner 1, Lq / Lk the longest (they size the grids)
    const int32_t *cu_q, *cu_k;      // ragged: sequence `outer` owns token rows [cu[outer], cu[outer + 1]) of the packed tensors
    long long total_q, total_k;      // ragged: rows of the packed tensors; statistics are [H][total_q], partials [2][n_split][H][total_k][D]
    long long q_s[4], k_s[4], v_s[4], o_s[4], do_s[4], dq_s[4], dk_s[4], dv_s[4];     // {outer, inner, seq, head} in elements
    float scale, scale_log2e, inv_scale_log2e;
};

template <int D>
struct Cfg {
    static constexpr int NS = D / 16;        // MFMA steps of a d contraction
    static constexpr int ND = D / 32;        // 32-row tiles of a transposed gradient accumulator
    static constexpr int KC = D / 8;         // 16-byte chunks per row
    static constexpr int LOADS = 2 * YT * KC / THREADS;     // chunks staged per thread per tile (two row images)
    // chunk swizzle of the row images (the forward's: lane = row, 16-byte fragment reads)
    __device__ static __forceinline__ int swz(int row) { return KC == 4 ? ((row >> 2) & 3) : ((row >> 1) & 7); }
};

// accumulator register r of lane half `half` is row (r & 3) + 8 (r >> 2) + 4 half of the 32x32 tile
__device__ __forceinline__ int crow(int r, int half) { return (r & 3) + 8 * (r >> 2) + 4 * half; }

__device__ __forceinline__ long long head_off(const long long (&s)[4], int outer, int inner, int head) {
    return (long long)outer * s[0] + (long long)inner * s[1] + (long long)head * s[3];
}

// logical order: owned block fastest, then head, inner, outer; one XCD owns a contiguous run, so the workgroups that stream the same
// rows of one (sequence, head) read them through one L2
__device__ __forceinline__ void decode_block(const BwdParams& p, int& xb, int& head, int& inner, int& outer, long long& prob, int& sp) {
    int bid = (int)gvf_xcd_remap(blockIdx.x, gridDim.x);
    sp = bid % p.n_split; bid /= p.n_split;
    xb = bid % p.x_blocks; bid /= p.x_blocks;
    head = bid % p.H; bid /= p.H;
    inner = bid % p.n_inner;
    outer = bid / p.n_inner;
    prob = ((long long)outer * p.n_inner + inner) * p.H + head;
}

// Where a workgroup gets its problem from.  Dense: the call's lengths, rows from the tensors' bases, statistics (N, H, Lq).  Ragged: the
// row bases and lengths of sequence `outer` are read from cu_seqlens once per workgroup (uniform), statistics and partials are indexed
// [head][packed row].  stat0 / part0: first statistics row of the problem / first partial row of one split chunk.
struct Problem {
    int Lq, Lk;
    long long q0, k0, stat0, part0, part_rows;
};
template <bool VARLEN>
__device__ __forceinline__ Problem problem_of(const BwdParams& p, int outer, int head, long long prob) {
    Problem w;
    if (VARLEN) {
        w.q0 = p.cu_q[outer]; w.Lq = p.cu_q[outer + 1] - (int)w.q0;
        w.k0 = p.cu_k[outer]; w.Lk = p.cu_k[outer + 1] - (int)w.k0;
        w.stat0 = (long long)head * p.total_q + w.q0;
        w.part0 = (long long)head * p.total_k + w.k0;
        w.part_rows = (long long)p.H * p.total_k;
    } else {
        w.q0 = 0; w.k0 = 0; w.Lq = p.Lq; w.Lk = p.Lk;
        w.stat0 = prob * p.Lq;
        w.part0 = prob * p.Lk;
        w.part_rows = (long long)p.n_outer * p.n_inner * p.H * p.Lk;
    }
    return w;
}

__device__ __forceinline__ uint4 ld16(const unsigned short* ptr, bool ok) {
    return ok ? *reinterpret_cast<const uint4*>(ptr) : make_uint4(0u, 0u, 0u, 0u);
}

template <int DT>
__device__ __forceinline__ float dot8(uint4 a, uint4 b) {
    const unsigned aw[4] = {a.x, a.y, a.z, a.w}, bw[4] = {b.x, b.y, b.z, b.w};
    float s = 0.f;
#pragma unroll
    for (int i = 0; i < 4; ++i) s += GvfLp<DT>::lo(aw[i]) * GvfLp<DT>::lo(bw[i]) + GvfLp<DT>::hi(aw[i]) * GvfLp<DT>::hi(bw[i]);
    return s;
}

// four accumulator registers -> 8 bytes of a gradient row (d = 8 g + 4 half .. + 3)
template <int DT>
__device__ __forceinline__ void store4(unsigned short* dst, const f32x16& acc, int g) {
    uint2 w;
    w.x = GvfLp<DT>::pack(acc[4 * g], acc[4 * g + 1]);
    w.y = GvfLp<DT>::pack(acc[4 * g + 2], acc[4 * g + 3]);
    *reinterpret_cast<uint2*>(dst) = w;
}

// ---------------------------------------------------------------------------------------------------------------------
// Row statistics: one workgroup = 128 queries of one (sequence, head), a wave 32; the keys stream through LDS in 32-row tiles.
// S^T = K Q^T (query on the lane), online maximum / sum in the log2 domain.
template <int D, int DT, bool VARLEN>
__global__ __launch_bounds__(THREADS) void attn_bwd_stats_kernel(BwdParams p) {
    using C = Cfg<D>;
    typedef GvfLp<DT> LP;
    typedef typename LP::x8 x8;
    __shared__ uint4 sK[2][YT * C::KC];

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, half = lane >> 5, l31 = lane & 31;
    int xb, head, inner, outer, sp;
    long long prob;
    decode_block(p, xb, head, inner, outer, prob, sp);
    const Problem w = problem_of<VARLEN>(p, outer, head, prob);
    const int Lq = w.Lq, Lk = w.Lk;
    if (VARLEN && (xb * XB >= Lq || Lk <= 0)) return;      // whole workgroup (uniform): no such query block, or no key to attend to
    const unsigned short* qp = p.q + head_off(p.q_s, outer, inner, head) + w.q0 * p.q_s[2];
    const unsigned short* kp = p.k + head_off(p.k_s, outer, inner, head) + w.k0 * p.k_s[2];
    const unsigned short* op = p.o + head_off(p.o_s, outer, inner, head) + w.q0 * p.o_s[2];
    const unsigned short* gp = p.dout + head_off(p.do_s, outer, inner, head) + w.q0 * p.do_s[2];

    const int qrow = xb * XB + wave * 32 + l31;
    const bool qvalid = qrow < Lq;
    x8 qf[C::NS];
    float delta = 0.f;
#pragma unroll
    for (int s = 0; s < C::NS; ++s) {
        const int d0 = 16 * s + 8 * half;
        qf[s] = __builtin_bit_cast(x8, ld16(qp + (long long)qrow * p.q_s[2] + d0, qvalid));
        delta += dot8<DT>(ld16(gp + (long long)qrow * p.do_s[2] + d0, qvalid), ld16(op + (long long)qrow * p.o_s[2] + d0, qvalid));
    }
    delta += __shfl_xor(delta, 32, 64);

    const int n_tiles = (Lk + YT - 1) / YT;
    const bool stager = tid < YT * C::KC;
    const int st_row = tid / C::KC, st_c = tid % C::KC;
    const int st_slot = st_row * C::KC + (st_c ^ C::swz(st_row));
    uint4 kreg = ld16(kp + (long long)st_row * p.k_s[2] + st_c * 8, stager && st_row < Lk);
    if (stager) sK[0][st_slot] = kreg;
    __syncthreads();

    float m_run = -INFINITY, l_run = 0.f;
    for (int t = 0; t < n_tiles; ++t) {
        const int buf = t & 1;
        if (t + 1 < n_tiles) {
            const int y = (t + 1) * YT + st_row;
            kreg = ld16(kp + (long long)y * p.k_s[2] + st_c * 8, stager && y < Lk);
        }
        f32x16 s_acc;
#pragma unroll
        for (int r = 0; r < 16; ++r) s_acc[r] = 0.f;
#pragma unroll
        for (int st = 0; st < C::NS; ++st) {
            const x8 kf = __builtin_bit_cast(x8, sK[buf][l31 * C::KC + ((2 * st + half) ^ C::swz(l31))]);
            s_acc = LP::mfma32(kf, qf[st], s_acc);
        }
        const int key0 = t * YT;
        if (key0 + YT > Lk) {                     // last, partial tile (uniform): keys past Lk leave the softmax
#pragma unroll
            for (int r = 0; r < 16; ++r)
                if (key0 + crow(r, half) >= Lk) s_acc[r] = -INFINITY;
        }
        float mloc = s_acc[0];
#pragma unroll
        for (int r = 1; r < 16; ++r) mloc = fmaxf(mloc, s_acc[r]);
        mloc *= p.scale_log2e;                      // scale > 0: the maximum commutes with it
        mloc = fmaxf(mloc, __shfl_xor(mloc, 32, 64));
        const float m_new = fmaxf(m_run, mloc);     // finite: key key0 of every tile is valid
        float psum = 0.f;
#pragma unroll
        for (int r = 0; r < 16; ++r) psum += __builtin_amdgcn_exp2f(__builtin_fmaf(s_acc[r], p.scale_log2e, -m_new));
        l_run = l_run * __builtin_amdgcn_exp2f(m_run - m_new) + psum;
        m_run = m_new;
        if (t + 1 < n_tiles && stager) sK[buf ^ 1][st_slot] = kreg;      // that buffer was last read before the previous barrier
        __syncthreads();
    }
    const float l_tot = l_run + __shfl_xor(l_run, 32, 64);
    if (qvalid && half == 0) {
        p.lse2[w.stat0 + qrow] = m_run + log2f(l_tot);
        p.delta[w.stat0 + qrow] = delta;
    }
}

// ---------------------------------------------------------------------------------------------------------------------
// The gradient sweeps.  KEYOWN: the workgroup owns keys and streams queries (dK, dV); otherwise it owns queries and streams keys (dQ).
template <int D, bool KEYOWN, int DT, bool VARLEN>
__global__ __launch_bounds__(THREADS) void attn_bwd_sweep_kernel(BwdParams p) {
    using C = Cfg<D>;
    typedef GvfLp<DT> LP;
    typedef typename LP::x8 x8;
    constexpr int NT = KEYOWN ? 2 : 1;                                     // transposed images: Y1^T, and Y2^T (= dO^T) for dV
    __shared__ uint4 sY[2][2][YT * C::KC];                                 // [buffer][image][row][chunk ^ swz(row)]
    __shared__ __attribute__((aligned(16))) unsigned short sYT[2][NT][D * TLD];     // [buffer][image][d][y]
    __shared__ __attribute__((aligned(16))) float sStat[2][2][YT];         // KEYOWN: -lse2 / c and -delta of the staged queries

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, half = lane >> 5, l31 = lane & 31;
    int xb, head, inner, outer, sp;
    long long prob;
    decode_block(p, xb, head, inner, outer, prob, sp);
    const Problem w = problem_of<VARLEN>(p, outer, head, prob);
    const int Lx = KEYOWN ? w.Lk : w.Lq, Ly = KEYOWN ? w.Lq : w.Lk;
    // ragged: an owned block past its sequence's length has nothing to do (whole workgroup, uniform).  A sequence with no streamed rows
    // (keys without queries, queries without keys) runs no tile below and stores its zero accumulators: those gradient rows are +0.
    if (VARLEN && xb * XB >= Lx) return;
    const unsigned short* qp = p.q + head_off(p.q_s, outer, inner, head) + w.q0 * p.q_s[2];
    const unsigned short* kp = p.k + head_off(p.k_s, outer, inner, head) + w.k0 * p.k_s[2];
    const unsigned short* vp = p.v + head_off(p.v_s, outer, inner, head) + w.k0 * p.v_s[2];
    const unsigned short* gp = p.dout + head_off(p.do_s, outer, inner, head) + w.q0 * p.do_s[2];
    const unsigned short* x1p = KEYOWN ? kp : qp;
    const unsigned short* x2p = KEYOWN ? vp : gp;
    const unsigned short* y1p = KEYOWN ? qp : kp;
    const unsigned short* y2p = KEYOWN ? gp : vp;
    const long long x1_sl = KEYOWN ? p.k_s[2] : p.q_s[2], x2_sl = KEYOWN ? p.v_s[2] : p.do_s[2];
    const long long y1_sl = KEYOWN ? p.q_s[2] : p.k_s[2], y2_sl = KEYOWN ? p.do_s[2] : p.v_s[2];
    const float* lse2 = p.lse2 + w.stat0;
    const float* delta = p.delta + w.stat0;

    // ---- owned rows: B operands.  Lane (x = lane & 31, half): X[x][16 s + 8 half .. + 7]
    const int xrow = xb * XB + wave * 32 + l31;
    const bool xvalid = xrow < Lx;
    const bool wave_active = xb * XB + wave * 32 < Lx;                     // wave-uniform
    x8 x1f[C::NS], x2f[C::NS];
#pragma unroll
    for (int s = 0; s < C::NS; ++s) {
        x1f[s] = __builtin_bit_cast(x8, ld16(x1p + (long long)xrow * x1_sl + 16 * s + 8 * half, xvalid));
        x2f[s] = __builtin_bit_cast(x8, ld16(x2p + (long long)xrow * x2_sl + 16 * s + 8 * half, xvalid));
    }
    float nl_lane = 0.f, nd_lane = 0.f;                                    // sweep Q: the lane's query constants
    if (!KEYOWN && xvalid && (!VARLEN || Ly > 0)) {                       // (no keys: no statistics were written, none are used)
        nl_lane = -lse2[xrow] * p.inv_scale_log2e;
        nd_lane = -delta[xrow];
    }

    f32x16 acc1[C::ND], acc2[C::ND];                                       // acc1: dK^T or dQ^T; acc2: dV^T (sweep K only)
#pragma unroll
    for (int dt = 0; dt < C::ND; ++dt)
#pragma unroll
        for (int r = 0; r < 16; ++r) { acc1[dt][r] = 0.f; acc2[dt][r] = 0.f; }

    // ---- staging roles: chunk c = tid + i * 256 of the 2 * YT * KC chunks of a tile: image c / (YT KC), row, 16-byte chunk
    int st_img[C::LOADS], st_row[C::LOADS], st_c[C::LOADS];
#pragma unroll
    for (int i = 0; i < C::LOADS; ++i) {
        const int c = tid + i * THREADS;
        st_img[i] = c / (YT * C::KC);
        const int w = c % (YT * C::KC);
        st_row[i] = w / C::KC;
        st_c[i] = w % C::KC;
    }
    // streamed tiles [t0, t1) of this workgroup: all of them, or chunk `sp` of n_split when the key sweep is split over the queries
    // (ragged: chunks of the sequence's own tiles; a chunk past them runs no tile and hands zeros to the reduction)
    const int n_tiles_all = (Ly + YT - 1) / YT;
    const int tiles_per = (n_tiles_all + p.n_split - 1) / p.n_split;
    const int t0 = sp * tiles_per, t1 = min(n_tiles_all, t0 + tiles_per);
    uint4 yreg[C::LOADS];
    float sreg = 0.f;
    const int stat_which = tid >> 5, stat_row = tid & 31;                  // threads 0..63 stage the two row constants (sweep K)

#define GVF_BWD_LOAD(t_)                                                                                         \
    _Pragma("unroll") for (int i = 0; i < C::LOADS; ++i) {                                                       \
        const int y_ = (t_) * YT + st_row[i];                                                                    \
        const unsigned short* src_ = st_img[i] ? y2p + (long long)y_ * y2_sl : y1p + (long long)y_ * y1_sl;      \
        yreg[i] = ld16(src_ + st_c[i] * 8, y_ < Ly);                                                             \
    }                                                                                                            \
    if (KEYOWN && tid < 64) {                                                                                    \
        const int y_ = (t_) * YT + stat_row;                                                                     \
        sreg = y_ < Ly ? (stat_which ? -delta[y_] : -lse2[y_] * p.inv_scale_log2e) : 0.f;                        \
    }
#define GVF_BWD_STORE(buf_)                                                                                      \
    _Pragma("unroll") for (int i = 0; i < C::LOADS; ++i) {                                                       \
        sY[buf_][st_img[i]][st_row[i] * C::KC + (st_c[i] ^ C::swz(st_row[i]))] = yreg[i];                        \
        if (st_img[i] < NT) {                                                                                    \
            const unsigned w_[4] = {yreg[i].x, yreg[i].y, yreg[i].z, yreg[i].w};                                 \
            unsigned short* dst_ = &sYT[buf_][st_img[i] < NT ? st_img[i] : 0][st_c[i] * 8 * TLD + st_row[i]];    \
            _Pragma("unroll") for (int e = 0; e < 4; ++e) {                                                      \
                dst_[(2 * e) * TLD] = (unsigned short)(w_[e] & 0xffffu);                                         \
                dst_[(2 * e + 1) * TLD] = (unsigned short)(w_[e] >> 16);                                         \
            }                                                                                                    \
        }                                                                                                        \
    }                                                                                                            \
    if (KEYOWN && tid < 64) sStat[buf_][stat_which][stat_row] = sreg;

    GVF_BWD_LOAD(t0)
    GVF_BWD_STORE(0)
    __syncthreads();

    for (int t = t0; t < t1; ++t) {
        const int buf = (t - t0) & 1;
        if (t + 1 < t1) { GVF_BWD_LOAD(t + 1) }                            // in flight while this tile is consumed
        if (wave_active) {
            f32x16 s_acc, dp_acc;
            if (KEYOWN) {                                                   // the row constants of queries crow(r, half)
#pragma unroll
                for (int g = 0; g < 4; ++g) {
                    const float4 a = *reinterpret_cast<const float4*>(&sStat[buf][0][8 * g + 4 * half]);
                    const float4 b = *reinterpret_cast<const float4*>(&sStat[buf][1][8 * g + 4 * half]);
                    s_acc[4 * g] = a.x; s_acc[4 * g + 1] = a.y; s_acc[4 * g + 2] = a.z; s_acc[4 * g + 3] = a.w;
                    dp_acc[4 * g] = b.x; dp_acc[4 * g + 1] = b.y; dp_acc[4 * g + 2] = b.z; dp_acc[4 * g + 3] = b.w;
                }
            } else {
#pragma unroll
                for (int r = 0; r < 16; ++r) { s_acc[r] = nl_lane; dp_acc[r] = nd_lane; }
            }
            // S' = Y1 X1^T - lse2 / c,  dP' = Y2 X2^T - delta : accumulator [y = crow(r, half)][x = lane & 31]
#pragma unroll
            for (int st = 0; st < C::NS; ++st) {
                const int slot = l31 * C::KC + ((2 * st + half) ^ C::swz(l31));
                s_acc = LP::mfma32(__builtin_bit_cast(x8, sY[buf][0][slot]), x1f[st], s_acc);
                dp_acc = LP::mfma32(__builtin_bit_cast(x8, sY[buf][1][slot]), x2f[st], dp_acc);
            }
            float pr[16];
#pragma unroll
            for (int r = 0; r < 16; ++r) pr[r] = __builtin_amdgcn_exp2f(s_acc[r] * p.scale_log2e);
            if (t * YT + YT > Ly) {                                         // last, partial tile (uniform): staged rows past Ly are zeros
#pragma unroll
                for (int r = 0; r < 16; ++r)
                    if (t * YT + crow(r, half) >= Ly) pr[r] = 0.f;
            }
            unsigned pw[8], dw[8];
#pragma unroll
            for (int r = 0; r < 16; r += 2) {
                pw[r >> 1] = LP::pack(pr[r], pr[r + 1]);
                dw[r >> 1] = LP::pack(pr[r] * dp_acc[r] * p.scale, pr[r + 1] * dp_acc[r + 1] * p.scale);
            }
            // G^T[d][x] += sum_y Y^T[d][y] B[y][x]; contraction slot (u, half, e) = accumulator row 16 u + 4 half + (e & 3) + 8 (e >> 2)
#pragma unroll
            for (int u = 0; u < 2; ++u) {
                const x8 pf = __builtin_bit_cast(x8, make_uint4(pw[4 * u], pw[4 * u + 1], pw[4 * u + 2], pw[4 * u + 3]));
                const x8 df = __builtin_bit_cast(x8, make_uint4(dw[4 * u], dw[4 * u + 1], dw[4 * u + 2], dw[4 * u + 3]));
#pragma unroll
                for (int dt = 0; dt < C::ND; ++dt) {
                    const int off = (dt * 32 + l31) * TLD + 16 * u + 4 * half;
                    const uint2 a0 = *reinterpret_cast<const uint2*>(&sYT[buf][0][off]);
                    const uint2 a1 = *reinterpret_cast<const uint2*>(&sYT[buf][0][off + 8]);
                    acc1[dt] = LP::mfma32(__builtin_bit_cast(x8, make_uint4(a0.x, a0.y, a1.x, a1.y)), df, acc1[dt]);
                    if (KEYOWN) {
                        const uint2 b0 = *reinterpret_cast<const uint2*>(&sYT[buf][NT - 1][off]);
                        const uint2 b1 = *reinterpret_cast<const uint2*>(&sYT[buf][NT - 1][off + 8]);
                        acc2[dt] = LP::mfma32(__builtin_bit_cast(x8, make_uint4(b0.x, b0.y, b1.x, b1.y)), pf, acc2[dt]);
                    }
                }
            }
        }
        // the other buffer was last read in iteration t - 1; every wave has passed that iteration's barrier
        if (t + 1 < t1) { GVF_BWD_STORE(buf ^ 1) }
        __syncthreads();
    }
#undef GVF_BWD_LOAD
#undef GVF_BWD_STORE

    // ---- epilogue: accumulator column = owned row, register r = d (r & 3) + 8 (r >> 2) + 4 half (+ 32 dt)
    if (KEYOWN && p.n_split > 1) {                   // split key sweep: fp32 partials, summed in chunk order by attn_bwd_reduce_kernel
        if (xvalid) {
            float* d1 = p.part + ((long long)sp * w.part_rows + w.part0 + xrow) * D;
            float* d2 = d1 + (long long)p.n_split * w.part_rows * D;
#pragma unroll
            for (int dt = 0; dt < C::ND; ++dt)
#pragma unroll
                for (int g = 0; g < 4; ++g) {
                    const int d = dt * 32 + 8 * g + 4 * half;
                    *reinterpret_cast<float4*>(d1 + d) = make_float4(acc1[dt][4 * g], acc1[dt][4 * g + 1], acc1[dt][4 * g + 2], acc1[dt][4 * g + 3]);
                    *reinterpret_cast<float4*>(d2 + d) = make_float4(acc2[dt][4 * g], acc2[dt][4 * g + 1], acc2[dt][4 * g + 2], acc2[dt][4 * g + 3]);
                }
        }
        return;
    }
    if (xvalid) {
        unsigned short* g1 = KEYOWN ? p.dk + head_off(p.dk_s, outer, inner, head) + (w.k0 + xrow) * p.dk_s[2]
                                    : p.dq + head_off(p.dq_s, outer, inner, head) + (w.q0 + xrow) * p.dq_s[2];
#pragma unroll
        for (int dt = 0; dt < C::ND; ++dt)
#pragma unroll
            for (int g = 0; g < 4; ++g) store4<DT>(g1 + dt * 32 + 8 * g + 4 * half, acc1[dt], g);
        if (KEYOWN) {
            unsigned short* g2 = p.dv + head_off(p.dv_s, outer, inner, head) + (w.k0 + xrow) * p.dv_s[2];
#pragma unroll
            for (int dt = 0; dt < C::ND; ++dt)
#pragma unroll
                for (int g = 0; g < 4; ++g) store4<DT>(g2 + dt * 32 + 8 * g + 4 * half, acc2[dt], g);
        }
    }
}

// dK, dV = the sum of the split key sweep's fp32 partials in chunk order, rounded once.  One thread per four channels of a key row.
// (ragged: the grid covers the longest key range of every (sequence, head); threads past their sequence's keys leave)
template <int D, int DT, bool VARLEN>
__global__ __launch_bounds__(THREADS) void attn_bwd_reduce_kernel(BwdParams p, long long n_groups) {
    const long long gi = (long long)blockIdx.x * THREADS + threadIdx.x;
    if (gi >= n_groups) return;
    const int d = (int)(gi % (D / 4)) * 4;
    const long long grow = gi / (D / 4);
    const int key = (int)(grow % p.Lk);
    const long long prob = grow / p.Lk;
    const int head = (int)(prob % p.H);
    const long long oi = prob / p.H;
    const int inner = (int)(oi % p.n_inner), outer = (int)(oi / p.n_inner);
    const Problem w = problem_of<VARLEN>(p, outer, head, prob);
    if (VARLEN && key >= w.Lk) return;
    const long long row = w.part0 + key;
    const long long chunk = w.part_rows * D;                                // floats per split chunk
#pragma unroll
    for (int which = 0; which < 2; ++which) {
        const float* src = p.part + (long long)which * p.n_split * chunk + row * D + d;
        float4 a = *reinterpret_cast<const float4*>(src);
        for (int s = 1; s < p.n_split; ++s) {
            const float4 b = *reinterpret_cast<const float4*>(src + s * chunk);
            a.x += b.x; a.y += b.y; a.z += b.z; a.w += b.w;
        }
        unsigned short* dst = which == 0 ? p.dk + head_off(p.dk_s, outer, inner, head) + (w.k0 + key) * p.dk_s[2]
                                         : p.dv + head_off(p.dv_s, outer, inner, head) + (w.k0 + key) * p.dv_s[2];
        uint2 w;
        w.x = GvfLp<DT>::pack(a.x, a.y);
        w.y = GvfLp<DT>::pack(a.z, a.w);
        *reinterpret_cast<uint2*>(dst + d) = w;
    }
}

// ---------------------------------------------------------------------------------------------------------------------
// Short sequences (Lq, Lk <= 32, head_dim 32): ONE WAVE owns one (sequence, head) problem, four problems per workgroup.  Rows go
// straight from global memory into MFMA operand registers (lane = row, 16-byte chunks `half` and `2 + half`); Q, K and dO are also
// staged row-major in a per-wave LDS slab and read back by columns as the A operands of the gradient products.  First with the
// query on the lane (statistics, dQ), then with the key on the lane (dK, dV), the row constants crossing the slab.
__device__ __forceinline__ void sm_stage(unsigned short* dst, const uint4 (&c)[2], int half) {
    *reinterpret_cast<uint2*>(dst + 8 * half) = make_uint2(c[0].x, c[0].y);
    *reinterpret_cast<uint2*>(dst + 8 * half + 4) = make_uint2(c[0].z, c[0].w);
    *reinterpret_cast<uint2*>(dst + 8 * (2 + half)) = make_uint2(c[1].x, c[1].y);
    *reinterpret_cast<uint2*>(dst + 8 * (2 + half) + 4) = make_uint2(c[1].z, c[1].w);
}
// A operand of step t from staged rows: element e of lane (d = lane & 31, half) is row 16 t + 4 half + (e & 3) + 8 (e >> 2), column d
__device__ __forceinline__ uint4 sm_col(const unsigned short* slab, int t, int half, int l31) {
    const unsigned short* col = slab + (16 * t + 4 * half) * SM_LD + l31;
    uint4 f;
    f.x = (unsigned)col[0 * SM_LD] | ((unsigned)col[1 * SM_LD] << 16);
    f.y = (unsigned)col[2 * SM_LD] | ((unsigned)col[3 * SM_LD] << 16);
    f.z = (unsigned)col[8 * SM_LD] | ((unsigned)col[9 * SM_LD] << 16);
    f.w = (unsigned)col[10 * SM_LD] | ((unsigned)col[11 * SM_LD] << 16);
    return f;
}

template <int DT>
__global__ __launch_bounds__(THREADS) void attn_bwd_small_kernel(BwdParams p, long long n_problems) {
    typedef GvfLp<DT> LP;
    typedef typename LP::x8 x8;
    __shared__ __attribute__((aligned(16))) unsigned short sRows[THREADS / 64][3][32 * SM_LD];      // Q, K, dO
    __shared__ float sStat[THREADS / 64][2][32];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, l31 = lane & 31, half = lane >> 5;
    const long long prob = (long long)blockIdx.x * (THREADS / 64) + wave;
    if (prob >= n_problems) return;                  // whole wave; no workgroup barrier below
    const int head = (int)(prob % p.H);
    const long long oi = prob / p.H;
    const int inner = (int)(oi % p.n_inner), outer = (int)(oi / p.n_inner);
    const bool qv = l31 < p.Lq, kv = l31 < p.Lk;
    const unsigned short* qr = p.q + head_off(p.q_s, outer, inner, head) + (long long)l31 * p.q_s[2];
    const unsigned short* kr = p.k + head_off(p.k_s, outer, inner, head) + (long long)l31 * p.k_s[2];
    const unsigned short* vr = p.v + head_off(p.v_s, outer, inner, head) + (long long)l31 * p.v_s[2];
    const unsigned short* orow = p.o + head_off(p.o_s, outer, inner, head) + (long long)l31 * p.o_s[2];
    const unsigned short* gr = p.dout + head_off(p.do_s, outer, inner, head) + (long long)l31 * p.do_s[2];
    uint4 qc[2], kc[2], vc[2], gc[2], oc[2];
#pragma unroll
    for (int s = 0; s < 2; ++s) {
        const int d0 = 8 * (2 * s + half);
        qc[s] = ld16(qr + d0, qv); gc[s] = ld16(gr + d0, qv); oc[s] = ld16(orow + d0, qv);
        kc[s] = ld16(kr + d0, kv); vc[s] = ld16(vr + d0, kv);
    }
    sm_stage(&sRows[wave][0][l31 * SM_LD], qc, half);
    sm_stage(&sRows[wave][1][l31 * SM_LD], kc, half);
    sm_stage(&sRows[wave][2][l31 * SM_LD], gc, half);
    float delta = dot8<DT>(gc[0], oc[0]) + dot8<DT>(gc[1], oc[1]);
    delta += __shfl_xor(delta, 32, 64);

    const f32x16 zero = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    // ---- query on the lane: S^T = K Q^T, dP^T = V dO^T; accumulator [key = crow(r, half)][query = lane & 31]
    f32x16 s_acc = zero, dp_acc = zero;
#pragma unroll
    for (int st = 0; st < 2; ++st) {
        s_acc = LP::mfma32(__builtin_bit_cast(x8, kc[st]), __builtin_bit_cast(x8, qc[st]), s_acc);
        dp_acc = LP::mfma32(__builtin_bit_cast(x8, vc[st]), __builtin_bit_cast(x8, gc[st]), dp_acc);
    }
    float m = -INFINITY;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        if (crow(r, half) >= p.Lk) s_acc[r] = -INFINITY;
        m = fmaxf(m, s_acc[r]);
    }
    m = fmaxf(m, __shfl_xor(m, 32, 64));              // Lk >= 1: finite
    const float ms = m * p.scale_log2e;
    float l = 0.f;
#pragma unroll
    for (int r = 0; r < 16; ++r) l += __builtin_amdgcn_exp2f(__builtin_fmaf(s_acc[r], p.scale_log2e, -ms));
    l += __shfl_xor(l, 32, 64);
    const float lse2 = ms + log2f(l);
    if (half == 0) { sStat[wave][0][l31] = lse2; sStat[wave][1][l31] = delta; }
    {
        unsigned dw[8];
#pragma unroll
        for (int r = 0; r < 16; r += 2) {
            const float p0 = __builtin_amdgcn_exp2f(__builtin_fmaf(s_acc[r], p.scale_log2e, -lse2));          // masked keys: exp2(-inf) = 0
            const float p1 = __builtin_amdgcn_exp2f(__builtin_fmaf(s_acc[r + 1], p.scale_log2e, -lse2));
            dw[r >> 1] = LP::pack(p0 * (dp_acc[r] - delta) * p.scale, p1 * (dp_acc[r + 1] - delta) * p.scale);
        }
        __builtin_amdgcn_wave_barrier();
        f32x16 dq_acc = zero;                        // dQ^T[d][q] = sum_key K^T[d][key] dS^T[key][q]
#pragma unroll
        for (int t = 0; t < 2; ++t) {
            const uint4 kf = sm_col(&sRows[wave][1][0], t, half, l31);
            dq_acc = LP::mfma32(__builtin_bit_cast(x8, kf), __builtin_bit_cast(x8, make_uint4(dw[4 * t], dw[4 * t + 1], dw[4 * t + 2], dw[4 * t + 3])),
                                dq_acc);
        }
        if (qv) {
            unsigned short* dst = p.dq + head_off(p.dq_s, outer, inner, head) + (long long)l31 * p.dq_s[2];
#pragma unroll
            for (int g = 0; g < 4; ++g) store4<DT>(dst + 8 * g + 4 * half, dq_acc, g);
        }
    }
    // ---- key on the lane: S = Q K^T, dP = dO V^T; accumulator [query = crow(r, half)][key = lane & 31]
    __builtin_amdgcn_wave_barrier();
    s_acc = zero; dp_acc = zero;
#pragma unroll
    for (int st = 0; st < 2; ++st) {
        s_acc = LP::mfma32(__builtin_bit_cast(x8, qc[st]), __builtin_bit_cast(x8, kc[st]), s_acc);
        dp_acc = LP::mfma32(__builtin_bit_cast(x8, gc[st]), __builtin_bit_cast(x8, vc[st]), dp_acc);
    }
    unsigned pw[8], dw[8];
#pragma unroll
    for (int r = 0; r < 16; r += 2) {
        const float l0 = sStat[wave][0][crow(r, half)], l1 = sStat[wave][0][crow(r + 1, half)];
        const float d0 = sStat[wave][1][crow(r, half)], d1 = sStat[wave][1][crow(r + 1, half)];
        float p0 = __builtin_amdgcn_exp2f(__builtin_fmaf(s_acc[r], p.scale_log2e, -l0));
        float p1 = __builtin_amdgcn_exp2f(__builtin_fmaf(s_acc[r + 1], p.scale_log2e, -l1));
        if (!kv) { p0 = 0.f; p1 = 0.f; }             // lanes past Lk hold no key
        pw[r >> 1] = LP::pack(p0, p1);
        dw[r >> 1] = LP::pack(p0 * (dp_acc[r] - d0) * p.scale, p1 * (dp_acc[r + 1] - d1) * p.scale);
    }
    f32x16 dk_acc = zero, dv_acc = zero;             // dV^T[d][key] = sum_q dO^T[d][q] P[q][key]; dK^T[d][key] = sum_q Q^T[d][q] dS[q][key]
#pragma unroll
    for (int t = 0; t < 2; ++t) {
        const uint4 gf = sm_col(&sRows[wave][2][0], t, half, l31);
        const uint4 qf = sm_col(&sRows[wave][0][0], t, half, l31);
        dv_acc = LP::mfma32(__builtin_bit_cast(x8, gf), __builtin_bit_cast(x8, make_uint4(pw[4 * t], pw[4 * t + 1], pw[4 * t + 2], pw[4 * t + 3])), dv_acc);
        dk_acc = LP::mfma32(__builtin_bit_cast(x8, qf), __builtin_bit_cast(x8, make_uint4(dw[4 * t], dw[4 * t + 1], dw[4 * t + 2], dw[4 * t + 3])), dk_acc);
    }
    if (kv) {
        unsigned short* dk = p.dk + head_off(p.dk_s, outer, inner, head) + (long long)l31 * p.dk_s[2];
        unsigned short* dv = p.dv + head_off(p.dv_s, outer, inner, head) + (long long)l31 * p.dv_s[2];
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            store4<DT>(dk + 8 * g + 4 * half, dk_acc, g);
            store4<DT>(dv + 8 * g + 4 * half, dv_acc, g);
        }
    }
}

bool small_path(int Lq, int Lk, int D) { return D == 32 && Lq <= 32 && Lk <= 32; }

// Chunks the key sweep's query range is split into.  Few key blocks against many queries (the motion VAE's decoder cross attention:
// 48 key blocks, 256 query tiles each) leave most of the part idle; then every key block is swept by several workgroups over
// disjoint query chunks and their fp32 partials are summed in a fixed order.  A function of the shape alone: results stay reproducible.
int key_split(long long problems, int Lq, int Lk, int D) {
    if (small_path(Lq, Lk, D)) return 1;
    const long long wgs = problems * ((Lk + XB - 1) / XB);
    const int n_tiles = (Lq + YT - 1) / YT;
    if (wgs >= 256 || n_tiles < 16) return 1;
    long long s = (512 + wgs - 1) / wgs;
    if (s > n_tiles / 8) s = n_tiles / 8;
    if (s > 16) s = 16;
    if (s < 2) return 1;
    const int per = (int)((n_tiles + s - 1) / s);
    return (n_tiles + per - 1) / per;                 // no empty chunk
}

int workspace_bytes(int n_outer, int n_inner, int Lq, int Lk, int H, int D, size_t* out) {
    if (!out || n_outer <= 0 || n_inner <= 0 || Lq <= 0 || Lk <= 0 || H <= 0 || (D != 32 && D != 64)) return GVF_EINVAL;
    const unsigned long long rows = (unsigned long long)n_outer * n_inner * H * Lq;
    if (rows > (1ull << 40)) return GVF_EINVAL;
    size_t bytes = 2 * gvf_align_up((size_t)rows * sizeof(float), 256);      // lse2 and delta, fp32 (N, H, Lq) each
    const long long problems = (long long)n_outer * n_inner * H;
    const int split = key_split(problems, Lq, Lk, D);
    if (split > 1) bytes += 2 * (size_t)split * (size_t)problems * (size_t)Lk * D * sizeof(float);     // partial dK, dV
    *out = bytes;
    return GVF_OK;
}

template <int D, int DT, bool VARLEN>
int launch_general(const BwdParams& p0, long long problems, hipStream_t stream) {
    BwdParams p = p0;
    const long long qb = (p.Lq + XB - 1) / XB, kb = (p.Lk + XB - 1) / XB;
    if (qb * problems > 0x7fffffffLL || kb * problems > 0x7fffffffLL) return GVF_EINVAL;
    const int split = key_split(problems, p.Lq, p.Lk, D);
    if (kb * problems * split > 0x7fffffffLL) return GVF_EINVAL;
    p.x_blocks = (int)qb; p.n_split = 1;
    hipLaunchKernelGGL((attn_bwd_stats_kernel<D, DT, VARLEN>), dim3((unsigned)(qb * problems)), dim3(THREADS), 0, stream, p);
    GVF_CHECK_LAUNCH();
    p.x_blocks = (int)kb; p.n_split = split;
    hipLaunchKernelGGL((attn_bwd_sweep_kernel<D, true, DT, VARLEN>), dim3((unsigned)(kb * problems * split)), dim3(THREADS), 0, stream, p);
    GVF_CHECK_LAUNCH();
    if (split > 1) {
        const long long n_groups = problems * p.Lk * (D / 4);
        if ((n_groups + THREADS - 1) / THREADS > 0x7fffffffLL) return GVF_EINVAL;
        hipLaunchKernelGGL((attn_bwd_reduce_kernel<D, DT, VARLEN>), dim3((unsigned)((n_groups + THREADS - 1) / THREADS)), dim3(THREADS), 0, stream, p, n_groups);
        GVF_CHECK_LAUNCH();
    }
    p.x_blocks = (int)qb; p.n_split = 1;
    hipLaunchKernelGGL((attn_bwd_sweep_kernel<D, false, DT, VARLEN>), dim3((unsigned)(qb * problems)), dim3(THREADS), 0, stream, p);
    GVF_CHECK_LAUNCH();
    return GVF_OK;
}

template <int DT>
int launch_bwd(const BwdParams& p, int D, hipStream_t stream) {
    const long long problems = (long long)p.n_outer * p.n_inner * p.H;
    (void)hipGetLastError();
    if (small_path(p.Lq, p.Lk, D)) {
        if ((problems + 3) / 4 > 0x7fffffffLL) return GVF_EINVAL;
        hipLaunchKernelGGL(attn_bwd_small_kernel<DT>, dim3((unsigned)((problems + 3) / 4)), dim3(THREADS), 0, stream, p, problems);
        GVF_CHECK_LAUNCH();
        return GVF_OK;
    }
    return D == 32 ? launch_general<32, DT, false>(p, problems, stream) : launch_general<64, DT, false>(p, problems, stream);
}

// Ragged form: statistics fp32 [H][total_q] twice, then (split key sweep) the partials fp32 [2][split][H][total_k][D].  The split count is
// key_split of the host-known arguments: n_seqs * H problems of the longest lengths.
int varlen_workspace_bytes(int n_seqs, long long total_q, long long total_k, int max_Lq, int max_Lk, int H, int D, size_t* out) {
    if (!out || n_seqs <= 0 || max_Lq <= 0 || max_Lk <= 0 || H <= 0 || (D != 32 && D != 64)) return GVF_EINVAL;
    if (total_q < 0 || total_k < 0 || total_q > 0x7fffffffLL || total_k > 0x7fffffffLL) return GVF_EINVAL;      // cu_seqlens are int32
    const unsigned long long rows = (unsigned long long)H * (unsigned long long)total_q;
    if (rows > (1ull << 40)) return GVF_EINVAL;
    size_t bytes = 2 * gvf_align_up((size_t)rows * sizeof(float), 256);
    const int split = key_split((long long)n_seqs * H, max_Lq, max_Lk, D);
    if (split > 1) bytes += 2 * (size_t)split * (size_t)H * (size_t)total_k * D * sizeof(float);
    *out = bytes;
    return GVF_OK;
}

template <int DT>
int launch_varlen(const BwdParams& p, int D, hipStream_t stream) {
    const long long problems = (long long)p.n_outer * p.H;
    (void)hipGetLastError();
    return D == 32 ? launch_general<32, DT, true>(p, problems, stream) : launch_general<64, DT, true>(p, problems, stream);
}

// The checks both entry points share (pointers, alignment, scale), and the fields they fill alike.
int fill_params(BwdParams& p, const void* q, const void* k, const void* v, const void* out, const void* dout, void* dq, void* dk, void* dv,
                const int64_t* q_strides, const int64_t* k_strides, const int64_t* v_strides, const int64_t* o_strides,
                const int64_t* do_strides, const int64_t* dq_strides, const int64_t* dk_strides, const int64_t* dv_strides, float scale,
                void* workspace, size_t workspace_bytes_given, size_t need) {
    if (!q || !k || !v || !out || !dout || !dq || !dk || !dv || !workspace) return GVF_EINVAL;
    if (!q_strides || !k_strides || !v_strides || !o_strides || !do_strides || !dq_strides || !dk_strides || !dv_strides) return GVF_EINVAL;
    if (workspace_bytes_given < need || (((uintptr_t)workspace) & 15)) return GVF_EINVAL;
    if (!(scale > 0.0f) || !(scale < 3.0e38f)) return GVF_EINVAL;
    // 16-byte operand chunks, 8-byte gradient stores: bases and every stride keep that alignment
    const int64_t* in_s[5] = {q_strides, k_strides, v_strides, o_strides, do_strides};
    const int64_t* out_s[3] = {dq_strides, dk_strides, dv_strides};
    const void* in_p[5] = {q, k, v, out, dout};
    const void* out_p[3] = {dq, dk, dv};
    for (int t = 0; t < 5; ++t) {
        if (((uintptr_t)in_p[t]) & 15) return GVF_EINVAL;
        for (int i = 0; i < 4; ++i)
            if (in_s[t][i] % 8) return GVF_EINVAL;
    }
    for (int t = 0; t < 3; ++t) {
        if (((uintptr_t)out_p[t]) & 7) return GVF_EINVAL;
        for (int i = 0; i < 4; ++i)
            if (out_s[t][i] % 4) return GVF_EINVAL;
    }
    p.q = (const unsigned short*)q; p.k = (const unsigned short*)k; p.v = (const unsigned short*)v;
    p.o = (const unsigned short*)out; p.dout = (const unsigned short*)dout;
    p.dq = (unsigned short*)dq; p.dk = (unsigned short*)dk; p.dv = (unsigned short*)dv;
    for (int i = 0; i < 4; ++i) {
        p.q_s[i] = q_strides[i]; p.k_s[i] = k_strides[i]; p.v_s[i] = v_strides[i]; p.o_s[i] = o_strides[i]; p.do_s[i] = do_strides[i];
        p.dq_s[i] = dq_strides[i]; p.dk_s[i] = dk_strides[i]; p.dv_s[i] = dv_strides[i];
    }
    p.x_blocks = 1; p.n_split = 1;
    p.cu_q = nullptr; p.cu_k = nullptr; p.total_q = 0; p.total_k = 0;
    p.scale = scale;
    p.scale_log2e = scale * 1.4426950408889634f;
    p.inv_scale_log2e = 1.0f / p.scale_log2e;
    return GVF_OK;
}

}  // namespace

extern "C" int gvf_attn_bwd_workspace_bytes(int n_outer, int n_inner, int Lq, int Lk, int H, int head_dim, size_t* out) {
    return workspace_bytes(n_outer, n_inner, Lq, Lk, H, head_dim, out);
}

extern "C" int gvf_attn_bwd(int dtype, const void* q, const void* k, const void* v, const void* out, const void* dout, void* dq, void* dk,
                            void* dv, int n_outer, int n_inner, int Lq, int Lk, int H, int head_dim, const int64_t* q_strides,
                            const int64_t* k_strides, const int64_t* v_strides, const int64_t* o_strides, const int64_t* do_strides,
                            const int64_t* dq_strides, const int64_t* dk_strides, const int64_t* dv_strides, float scale, void* workspace,
                            size_t workspace_bytes_given, void* stream) {
    if (dtype != GVF_DT_BF16 && dtype != GVF_DT_F16) return GVF_EINVAL;
    size_t need = 0;
    if (workspace_bytes(n_outer, n_inner, Lq, Lk, H, head_dim, &need) != GVF_OK) return GVF_EINVAL;
    BwdParams p;
    if (fill_params(p, q, k, v, out, dout, dq, dk, dv, q_strides, k_strides, v_strides, o_strides, do_strides, dq_strides, dk_strides,
                    dv_strides, scale, workspace, workspace_bytes_given, need) != GVF_OK)
        return GVF_EINVAL;
    p.lse2 = (float*)workspace;
    const size_t stat_bytes = gvf_align_up((size_t)n_outer * n_inner * H * Lq * sizeof(float), 256);
    p.delta = (float*)((char*)workspace + stat_bytes);
    p.part = (float*)((char*)workspace + 2 * stat_bytes);
    p.n_outer = n_outer; p.n_inner = n_inner; p.Lq = Lq; p.Lk = Lk; p.H = H;
    return dtype == GVF_DT_BF16 ? launch_bwd<0>(p, head_dim, (hipStream_t)stream) : launch_bwd<1>(p, head_dim, (hipStream_t)stream);
}

extern "C" int gvf_attn_varlen_bwd_workspace_bytes(int n_seqs, long long total_q, long long total_k, int max_Lq, int max_Lk, int H,
                                                   int head_dim, size_t* out) {
    return varlen_workspace_bytes(n_seqs, total_q, total_k, max_Lq, max_Lk, H, head_dim, out);
}

extern "C" int gvf_attn_varlen_bwd(int dtype, const void* q, const void* k, const void* v, const void* out, const void* dout, void* dq,
                                   void* dk, void* dv, int n_seqs, const int32_t* cu_seqlens_q, const int32_t* cu_seqlens_k,
                                   long long total_q, long long total_k, int max_Lq, int max_Lk, int H, int head_dim,
                                   const int64_t* q_strides, const int64_t* k_strides, const int64_t* v_strides, const int64_t* o_strides,
                                   const int64_t* do_strides, const int64_t* dq_strides, const int64_t* dk_strides,
                                   const int64_t* dv_strides, float scale, void* workspace, size_t workspace_bytes_given, void* stream) {
    if (dtype != GVF_DT_BF16 && dtype != GVF_DT_F16) return GVF_EINVAL;
    size_t need = 0;
    if (varlen_workspace_bytes(n_seqs, total_q, total_k, max_Lq, max_Lk, H, head_dim, &need) != GVF_OK) return GVF_EINVAL;
    if (!cu_seqlens_q || !cu_seqlens_k) return GVF_EINVAL;
    BwdParams p;
    if (fill_params(p, q, k, v, out, dout, dq, dk, dv, q_strides, k_strides, v_strides, o_strides, do_strides, dq_strides, dk_strides,
                    dv_strides, scale, workspace, workspace_bytes_given, need) != GVF_OK)
        return GVF_EINVAL;
    p.lse2 = (float*)workspace;
    const size_t stat_bytes = gvf_align_up((size_t)H * (size_t)total_q * sizeof(float), 256);
    p.delta = (float*)((char*)workspace + stat_bytes);
    p.part = (float*)((char*)workspace + 2 * stat_bytes);
    p.n_outer = n_seqs; p.n_inner = 1; p.Lq = max_Lq; p.Lk = max_Lk; p.H = H;
    p.cu_q = cu_seqlens_q; p.cu_k = cu_seqlens_k; p.total_q = total_q; p.total_k = total_k;
    return dtype == GVF_DT_BF16 ? launch_varlen<0>(p, head_dim, (hipStream_t)stream) : launch_varlen<1>(p, head_dim, (hipStream_t)stream);
}

