// attn_xt.hip -- cross attention of the DiT block against a PRE-TILED, step-invariant K/V cache; head_dim 32, bf16
// MFMA, gfx950 (MI355X).
//
// Replaces, for the two cross attentions of model/dit.py:263-270 (image context, 1370 keys per frame; static
// context, 4096 keys shared by all frames of a sample), the flash-attn call behind
// model/attention/full_attn.py:74-140.  The keys / values of a cross attention depend on the conditions only, so they
// are projected once per sample (DiT.prepare_conditions) -- and because this library owns that cache, it is stored in
// the exact image the attention workgroups want in LDS (gvf_attn_pack_kv_bf16 below):
//   * K tile  = 64 keys x 32 dims  bf16 (4 KiB), 16-byte chunk (key, c) at chunk slot  key*4 + (c ^ ((key>>2)&3)),
//     values pre-multiplied by  softmax_scale * log2(e)  IN FP32 before the one rounding to bf16 (the reference rounds
//     k to half precision once as well; the scale then costs nothing per score),
//   * V^T tile = 32 dims x 64 key slots bf16 (4 KiB), row d, chunk j at slot  d*8 + (j ^ ((d>>1)&7)); the 8 key slots
//     of chunk j = 2g + half hold keys  16g + 4half + (e&3) + 8(e>>2)  -- the order in which a lane of the first
//     product's accumulator holds its scores, so P never moves between lanes and every operand read is ONE
//     conflict-free ds_read_b128.
// Staging is then a linear LDS-DMA copy (global_load_lds_dwordx4: no VGPR round trip, no ds_write, no in-kernel
// transpose) of two tiles (16 KiB) per stage into a ring of three stages, one workgroup barrier per stage.
//
// One workgroup = 4 waves = 256 queries of one (sample, frame, head); a wave owns TWO 32-query sub-tiles (A, B) so
// that every K / V^T fragment read from LDS feeds two MFMAs, and so that the wave always has independent work for both
// pipes: while the VALU exponentiates the scores of one sub-tile the matrix pipe computes the scores of the other
// (software pipeline, one phase = {4 QK^T MFMAs of sub-tile X} interleaved with {32 exp2, 16 cvt_pk, row sums, 4 PV
// MFMAs of sub-tile Y}).  On gfx950 a SIMD overlaps MFMA and VALU work only when ONE wave interleaves them
// (scripts/ubench/mfma_valu_overlap.hip), so the issue order of a phase is written out and fenced (sched_barrier).
// The row sums of P are taken by the matrix pipe too (one v_mfma_f32_16x16x32 per 8 packed probabilities of a lane against a
// 0 / 1 selector, see xt_phase), i.e. the denominator sums the SAME bf16-rounded probabilities the numerator multiplies.  What bounds the loop is VALU issue: 32 v_exp_f32 (two issue slots each) + 16 v_cvt_pk +
// 16 MFMA issues per phase (profiles/r02_*attn_xt*: 104 issue quads per wave-phase, matrix pipe 43-53 % busy at the
// 1.7 GHz the chip holds under this load).
//
// Softmax without the running maximum.  softmax is shift invariant; the subtraction of the row maximum only guards the
// range.  With log2-domain scores |s| < 100 (|q.k|/sqrt(d) < 69 -- every trained attention) exp2(s) neither overflows
// nor vanishes in bf16 / fp32, so the fast path computes P = exp2(s) directly: no max tree, no rescale, no subtract.
// Every query's denominator is checked at the end (finite, 2^-100 < l < 2^100); if ANY query of the workgroup fails,
// the workgroup recomputes its 256 queries with the classic online softmax (running max, exact) -- results are
// always correct, the guard only decides the speed.
#include <cstdlib>
#include "gvf_common.h"
#include "gvf_lp.h"
#include "../../include/gvf_rast.h"
#include "../../include/gvf_dit.h"

#ifndef XT_TILES_PER_STAGE
#define XT_TILES_PER_STAGE 2  // key tiles staged (and consumed) per workgroup barrier
#endif
#ifndef XT_WAVES_PER_SIMD
#define XT_WAVES_PER_SIMD 2
#endif

#ifdef XT_TIMING
static long long* g_xt_dbg;           // set by the benchmark before the launch
#endif
namespace {

typedef gvf_f32x16 f32x16;
typedef gvf_f32x4 f32x4;

constexpr int XT_THREADS = 256;
constexpr int XT_QB = 256;             // queries per workgroup (4 waves x 2 sub-tiles x 32)
constexpr int XT_KT = 64;              // keys per tile
#ifndef XT_RING_STAGES
#define XT_RING_STAGES 3
#endif
constexpr int XT_NBUF = XT_RING_STAGES;   // LDS ring depth (stages): a stage is requested XT_NBUF - 1 barriers before it is consumed
constexpr int XT_TPS = XT_TILES_PER_STAGE;   // tiles per stage = per barrier
constexpr int XT_TILE_CHUNKS = 512;    // 16-byte chunks per staged tile: 256 K + 256 V^T
constexpr int XT_PF_CHUNKS = 16;       // landing zone of the prefetch loads (one dword per lane of one wave: 256 B that nobody reads)

struct XtParams {
    const unsigned short* q;
    unsigned short* out;
    const uint4* kt;                   // [set][head][tile][256 chunks]
    const uint4* vt;                   // [set][head][tile][256 chunks]
    int n_outer, n_inner, Lq, Lk, H, q_blocks, n_tiles;
    int n_items;                       // q_blocks * n_inner * n_outer * H: the units of work the grid's workgroups share out
    long long q_so, q_si, q_sl, q_sh, o_so, o_si, o_sl, o_sh;
    long long kv_so, kv_si;            // K/V set of (outer, inner) = outer * kv_so + inner * kv_si
    int* fallbacks;                    // optional: += 1 per workgroup that took the exact path
    const float* gamma_q;              // optional MultiHeadRMSNorm gain of q, f32 [H][32]
    int out_f32;                       // out is float (same element strides): the kernel's arithmetic without the output rounding
    const char* pf; long long pf_lines; int pf_iters;      // optional: [pf, pf + 128 pf_lines) is touched once by the launch (see gvf_attn_tiled_fwd_pf)
#ifdef XT_TIMING
    long long* dbg;                    // timing builds (scripts/ubench/attn_xt_bench.hip): [workgroup][wave][4] = loop ticks, barrier ticks, tiles, -
#endif
};

template <int DT>
__device__ __forceinline__ float xt_sumsq8(uint4 raw) {
    const unsigned w[4] = {raw.x, raw.y, raw.z, raw.w};
    float s = 0.f;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const float lo = GvfLp<DT>::lo(w[i]), hi = GvfLp<DT>::hi(w[i]);
        s += lo * lo + hi * hi;
    }
    return s;
}
// 8 operand-type values of a 32-wide head row -> normalize(x) * gamma * sqrt(32) * extra, given the row's sum of squares
template <int DT>
__device__ __forceinline__ uint4 xt_rms_apply(uint4 raw, float sumsq, const float* g8, float extra) {
    const float inv = extra * 5.656854249492381f / fmaxf(sqrtf(sumsq), 1e-12f);
    unsigned w[4] = {raw.x, raw.y, raw.z, raw.w};
#pragma unroll
    for (int i = 0; i < 4; ++i)
        w[i] = GvfLp<DT>::pack(GvfLp<DT>::lo(w[i]) * inv * g8[2 * i], GvfLp<DT>::hi(w[i]) * inv * g8[2 * i + 1]);
    return make_uint4(w[0], w[1], w[2], w[3]);
}

__device__ __forceinline__ void xt_dma16(const uint4* g, uint4* l) {
    __builtin_amdgcn_global_load_lds(g, (__attribute__((address_space(3))) void*)l, 16, 0, 0);
}

// ---------------------------------------------------------------------------------------------------------------
// One pipeline phase of a wave.
//   DO_QK: s_out[sub] = K'(64 keys) q^T for the 32 queries whose fragments are qf   (4 MFMAs, C = 0), K fragments kf
//   DO_SM: P = exp2(s_in) (keys >= n_valid -> 0 when MASK), l += row sums, o += V^T P^T   (4 MFMAs), V^T fragments vf
// The operand fragments live in registers ACROSS phases: a tile's K fragments serve the QK^T of both sub-tiles (two
// consecutive phases), its V^T fragments the P V of both (two consecutive phases, one tile later), so each is read from
// LDS once per tile -- and it is read IN PLACE, right behind the last MFMA that consumes the previous contents
// (PF = 1: vf[g] <- tile sNext behind PV MFMA g; PF = 2: kf[0] <- tile sNext behind PV MFMA 0, kf[1] behind PV MFMA 3,
// i.e. never between an older fragment load and its consumer: hipcc waits lgkmcnt(0), not a counted value, in this
// loop), half a phase or more before the next use: no ds_read latency is exposed and no second register set is needed.
// The explicit issue order (every group is fenced, so source order = instruction order):
//   E0 Q0 P0 Q1 E1 V0 P1 Q2 E2 V1 P2 Q3 E3 V2 P3 V3
// E = 8 v_exp_f32 of chunk g, P = its 4 v_cvt_pk + 8 row-sum adds, Q = one QK^T MFMA, V = one PV MFMA: every MFMA is
// followed by 8-12 independent VALU / transcendental instructions that issue in its shadow.
// ---------------------------------------------------------------------------------------------------------------
template <int DT>
__device__ __forceinline__ typename GvfLp<DT>::x8 xt_ld_k(const uint4* sK, int sub, int st, int l31, int half) {
    const int key = sub * 32 + l31;
    return __builtin_bit_cast(typename GvfLp<DT>::x8, sK[key * 4 + ((2 * st + half) ^ ((key >> 2) & 3))]);
}
template <int DT>
__device__ __forceinline__ typename GvfLp<DT>::x8 xt_ld_v(const uint4* sV, int g, int l31, int half) {
    return __builtin_bit_cast(typename GvfLp<DT>::x8, sV[l31 * 8 + ((2 * g + half) ^ ((l31 >> 1) & 7))]);
}

// sQ and l4b are read by no code: without them the compiler allocates attn_xt_kernel's registers differently, so they stay until a change
// that re-validates the kernel on the GPU removes them.
// c0: initial value of the score accumulators.  bf16: zero (the compiler folds it into the MFMA's inline constant).  fp16: the splat of
// minus the query's shift (see attn_xt_kernel) -- exp2 of a raw score would leave fp16's range.
template <int DT, bool DO_QK, bool DO_SM, bool MASK, int PF, bool SHIFT = GvfLp<DT>::kNeedsShift>
__device__ __forceinline__ void xt_phase(typename GvfLp<DT>::x8 (&kf)[2][2], typename GvfLp<DT>::x8 (&vf)[4], const uint4* __restrict__ sNext,
                                         const typename GvfLp<DT>::x8 (&qf)[2], const uint4* __restrict__ sQ,
                                         f32x16 (&s_out)[2], const f32x16 (&s_in)[2], f32x16& o_acc, f32x4& l4, f32x4& l4b,
                                         int l31, int half, int n_valid, const f32x16& c0) {
    typedef GvfLp<DT> LP;
    typedef typename LP::x8 x8;
    const f32x16 zero_ = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    const f32x16 zero = SHIFT ? c0 : zero_;
    float pe[8];
    unsigned pw[4][4];
#define XT_E(g_)                                                                                            \
    if (DO_SM) {                                                                                            \
        _Pragma("unroll") for (int e = 0; e < 8; ++e) {                                                     \
            pe[e] = __builtin_amdgcn_exp2f(s_in[(g_) >> 1][8 * ((g_) & 1) + e]);                            \
            if (MASK) pe[e] = (16 * (g_) + 4 * half + (e & 3) + 8 * (e >> 2)) < n_valid ? pe[e] : 0.f;     \
        }                                                                                                   \
        __builtin_amdgcn_sched_barrier(0);                                                                  \
    }
    /* Row sums by the matrix pipe: ONE v_mfma_f32_16x16x32 per 8 probabilities of a lane against a 0 / 1 selector (4 per tile and sub-tile,
       16 cycles each; against two v_mfma_f32_4x4x4 of 17 cycles: 1-3 % per launch, profiles/HISTORY_r04.md item 2).
       The lane's 8 probabilities (query l31, key half `half`) are a B operand of the 16x16x32 shape as they stand: there lane l is column l % 16,
       k-block l / 16 -- blocks 0 / 2 are the two key halves of query l % 16, blocks 1 / 3 those of query 16 + l % 16.  Against the selector
       A[i][k-block] = (i < 8) == (block even) rows 0-7 of the product sum query n, rows 8-15 query n + 16, both halves included: lane l's
       accumulator (column l % 16, rows 4 (l / 16) ..) holds the denominator of query (l % 16) + 16 (l / 32), fetched once in the epilogue. */
    const unsigned selw = ((((unsigned)l31 >> 3) ^ ((unsigned)l31 >> 4)) & 1u) ? 0u : LP::ONE2;
    const x8 sel = __builtin_bit_cast(x8, make_uint4(selw, selw, selw, selw));
#define XT_P(g_)                                                                                            \
    if (DO_SM) {                                                                                            \
        _Pragma("unroll") for (int i = 0; i < 4; ++i) pw[g_][i] = LP::pack(pe[2 * i], pe[2 * i + 1]);       \
        l4 = LP::mfma16(sel, __builtin_bit_cast(x8, make_uint4(pw[g_][0], pw[g_][1], pw[g_][2], pw[g_][3])), l4); \
        __builtin_amdgcn_sched_barrier(0);                                                                  \
    }
#define XT_V(g_)                                                                                            \
    if (DO_SM) {                                                                                            \
        o_acc = LP::mfma32(vf[g_], __builtin_bit_cast(x8, make_uint4(pw[g_][0], pw[g_][1], pw[g_][2], pw[g_][3])), o_acc); \
        if (PF == 1) vf[g_] = xt_ld_v<DT>(sNext, g_, l31, half);                                            \
        if (PF == 2 && ((g_) == 0 || (g_) == 3)) {   /* K fragments of the next tile: sub 0 behind V0 */     \
            kf[(g_) == 3][0] = xt_ld_k<DT>(sNext, (g_) == 3, 0, l31, half);   /* (Q1 is done), sub 1 behind V3 (end of phase) */ \
            kf[(g_) == 3][1] = xt_ld_k<DT>(sNext, (g_) == 3, 1, l31, half);                                   \
        }                                                                                                   \
        __builtin_amdgcn_sched_barrier(0);                                                                  \
    }
#define XT_Q(i_)                                                                                            \
    if (DO_QK) {                                                                                            \
        if (((i_) & 1) == 0) s_out[(i_) >> 1] = LP::mfma32(kf[(i_) >> 1][0], qf[0], zero);                  \
        else {                                                                                              \
            s_out[(i_) >> 1] = LP::mfma32(kf[(i_) >> 1][1], qf[1], s_out[(i_) >> 1]);                       \
        }                                                                                                   \
        __builtin_amdgcn_sched_barrier(0);                                                                  \
    }
    __builtin_amdgcn_sched_barrier(0);
    XT_E(0) XT_Q(0) XT_P(0) XT_Q(1) XT_E(1) XT_V(0) XT_P(1) XT_Q(2) XT_E(2) XT_V(1) XT_P(2) XT_Q(3) XT_E(3) XT_V(2) XT_P(3) XT_V(3)
    if (PF == 1 && !DO_SM) {      // first phase of a workgroup: nothing to chase, load the V^T fragments now
#pragma unroll
        for (int g = 0; g < 4; ++g) vf[g] = xt_ld_v<DT>(sNext, g, l31, half);
    }
#undef XT_E
#undef XT_P
#undef XT_V
#undef XT_Q
}

// classic online softmax over one staged tile for ONE 32-query sub-tile (exact fallback; not pipelined)
template <int DT>
__device__ __forceinline__ void xt_safe_tile(const uint4* __restrict__ sK, const uint4* __restrict__ sV, const typename GvfLp<DT>::x8 (&qf)[2],
                                             f32x16& o_acc, float& m_run, float& l_run, int l31, int half, int n_valid) {
    typedef GvfLp<DT> LP;
    typedef typename LP::x8 x8;
    const f32x16 zero = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    f32x16 s[2];
#pragma unroll
    for (int sub = 0; sub < 2; ++sub) {
        const int key = sub * 32 + l31;
        const int sw = (key >> 2) & 3;
        s[sub] = LP::mfma32(__builtin_bit_cast(x8, sK[key * 4 + (half ^ sw)]), qf[0], zero);
        s[sub] = LP::mfma32(__builtin_bit_cast(x8, sK[key * 4 + ((2 + half) ^ sw)]), qf[1], s[sub]);
    }
    float mloc = -INFINITY;
#pragma unroll
    for (int g = 0; g < 4; ++g)
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const int key = 16 * g + 4 * half + (e & 3) + 8 * (e >> 2);
            if (key >= n_valid) s[g >> 1][8 * (g & 1) + e] = -INFINITY;
            mloc = fmaxf(mloc, s[g >> 1][8 * (g & 1) + e]);
        }
    mloc = fmaxf(mloc, __shfl_xor(mloc, 32, 64));
    const float m_new = fmaxf(m_run, mloc);                    // finite: every tile holds >= 1 valid key
    const float alpha = __builtin_amdgcn_exp2f(m_run - m_new); // first tile: exp2(-inf) = 0
    l_run *= alpha;
#pragma unroll
    for (int r = 0; r < 16; ++r) o_acc[r] *= alpha;
    m_run = m_new;
    const int sw = (l31 >> 1) & 7;
#pragma unroll
    for (int g = 0; g < 4; ++g) {
        unsigned pw[4];
#pragma unroll
        for (int e = 0; e < 8; e += 2) {
            const float p0 = __builtin_amdgcn_exp2f(s[g >> 1][8 * (g & 1) + e] - m_run);
            const float p1 = __builtin_amdgcn_exp2f(s[g >> 1][8 * (g & 1) + e + 1] - m_run);
            l_run += p0 + p1;
            pw[e >> 1] = LP::pack(p0, p1);
        }
        const x8 pf = __builtin_bit_cast(x8, make_uint4(pw[0], pw[1], pw[2], pw[3]));
        const x8 vf = __builtin_bit_cast(x8, sV[l31 * 8 + ((2 * g + half) ^ sw)]);
        o_acc = LP::mfma32(vf, pf, o_acc);
    }
}

// fp16 operands (DT = GVF_DT_F16): P = exp2(s) of a raw score overflows at s = 16, so every query gets a SHIFT -- the maximum of its scores
// against the first key tile (one 32-element in-lane max + one lane exchange per sub-tile per workgroup, not per tile) -- that enters every
// later QK^T MFMA as the accumulator's initial value (a 16-register splat of -shift per sub-tile): the MFMA result is again the exp2 argument,
// no per-score subtraction.  softmax is shift invariant; the true maximum is >= the shift, so the largest probability is >= 1 (full fp16
// precision where it matters) and overflows only if some later key beats the first tile's best by 2^16: P = inf -> l = inf -> the same range
// guard -> exact fallback.  bf16 needs none of this (kNeedsShift = false: the code below compiles to the round-2 kernel).
template <int DT>
__device__ __forceinline__ void xt_take_shift(f32x16 (&s)[2], f32x16& c) {
    float m = fmaxf(s[0][0], s[1][0]);
#pragma unroll
    for (int r = 1; r < 16; ++r) m = fmaxf(fmaxf(m, s[0][r]), s[1][r]);
    m = fmaxf(m, __shfl_xor(m, 32, 64));
    if (!(m > -3.0e38f && m < 3.0e38f)) m = 0.f;          // NaN / inf scores: no shift; the range guard sends the workgroup to the exact path
#pragma unroll
    for (int r = 0; r < 16; ++r) { s[0][r] -= m; s[1][r] -= m; c[r] = -m; }
}

// One unit of work: 256 queries of one (sample, frame, head) against that (set, head)'s tiles.
struct XtItem {
    const unsigned short* qp;          // first query row of the (outer, inner, head) slice
    long long o_off;                   // element offset of the slice in `out` (16-bit and fp32 output alike)
    const uint4* kbase;
    const uint4* vbase;
    int qb, head;
};
template <typename P>
__device__ __forceinline__ XtItem xt_item(const P& p, int bid) {
    XtItem it;
    it.qb = bid % p.q_blocks; bid /= p.q_blocks;
    const int inner = bid % p.n_inner; bid /= p.n_inner;
    const int outer = bid % p.n_outer;
    it.head = bid / p.n_outer;
    it.qp = p.q + outer * p.q_so + inner * p.q_si + it.head * p.q_sh;
    it.o_off = outer * p.o_so + inner * p.o_si + it.head * p.o_sh;
    const long long set = outer * p.kv_so + inner * p.kv_si;
    it.kbase = p.kt + ((set * p.H + it.head) * p.n_tiles) * 256;
    it.vbase = p.vt + ((set * p.H + it.head) * p.n_tiles) * 256;
    return it;
}
// the wave's two 32-query sub-tiles, RAW: lane (q = l31, half) holds Q[q][16 st + 8 half .. +7]; rows past Lq read row 0 and are zeroed by
// xt_mask_q where the fragments are formed -- NOT here: an AND on the loaded words right behind the loads makes the compiler wait for them
// on the spot, and the tail of an item issues these loads precisely so that they fly under its normalisation and stores
template <typename P>
__device__ __forceinline__ void xt_load_q(const P& p, const XtItem& it, int wave, int l31, int half, uint4 (&qraw)[2][2]) {
#pragma unroll
    for (int a = 0; a < 2; ++a) {
        const int row = it.qb * XT_QB + wave * 64 + a * 32 + l31;
#pragma unroll
        for (int st = 0; st < 2; ++st)
            qraw[a][st] = *reinterpret_cast<const uint4*>(it.qp + (long long)(row < p.Lq ? row : 0) * p.q_sl + 16 * st + 8 * half);
    }
}
__device__ __forceinline__ uint4 xt_mask_q(uint4 v4, bool valid) {
    const unsigned m = valid ? 0xffffffffu : 0u;
    return make_uint4(v4.x & m, v4.y & m, v4.z & m, v4.w & m);
}

// SHIFT: the per-query shift of the fp16 path (see xt_take_shift).  false for bf16, and for fp16 when the caller vouches that every score is
// bounded above (GVF_ATTN_SCORES_BOUNDED: q . k' <= 15.5 in the log2 domain -- RMS-normalised q and k with known gains): P = exp2(s) then
// fits fp16 by itself, the kernel is the bf16 one with the other MFMA opcode (no 32 splat registers, no shift pass).  A broken
// promise overflows to inf and lands in the same range guard -> exact fallback.
//
// PERSISTENT WORKGROUPS (profiles/r05_attn_persist_ab.txt).  What a 256-query workgroup does BEFORE its loop -- query rows from HBM, the first two
// stages, the two fill phases: 7-10 k cycles, ~4 k of them memory latency nothing hides at the start of a launch -- is 60 % of the loop time
// of a spatial-attention workgroup (8 key tiles), 22 % of an image one (22), 8 % of a static one (64): profiles/r04_attn_xt_timing.txt.  The
// DiT's launches have 768 such items for 512 resident workgroups, so the grid is capped at the resident count and a workgroup walks
// its items (XCD x owns ONE contiguous range of the item space, its workgroups stride through it -- neighbours in item order share K / V
// sets, i.e. one L2): the NEXT item's query rows and first two stages are requested as soon as every wave is done with the ring
// (behind the guard's barriers), i.e. they fly under the current item's normalisation and stores, and the next item starts with its
// operands on the way instead of with a cold round trip.  A launch with no more items than resident slots is the one-item kernel of
// round 4, instruction for instruction.
template <int DT, bool SHIFT>
__global__ __launch_bounds__(XT_THREADS, XT_WAVES_PER_SIMD) void attn_xt_kernel(XtParams p, int force_safe) {
    typedef GvfLp<DT> LP;
    typedef typename LP::x8 x8;
    // ring of XT_NBUF stages x XT_TPS tiles x (256 K chunks + 256 V^T chunks) + one chunk for the guard flag.  ONE LDS object on purpose:
    // with a second __shared__ variable hipcc drains the LDS-DMA queue (vmcnt(0)) in front of every ds_read.
    __shared__ uint4 smem[XT_NBUF * XT_TPS * XT_TILE_CHUNKS + 1 + XT_PF_CHUNKS];
    volatile int* s_bad = reinterpret_cast<volatile int*>(&smem[XT_NBUF * XT_TPS * XT_TILE_CHUNKS]);

    const int tid0 = threadIdx.x;
    const int wave = __builtin_amdgcn_readfirstlane(tid0 >> 6);
#ifdef XT_TIMING
    const long long xt_k0 = (long long)__builtin_amdgcn_s_memtime();
    long long xt_loop0 = 0, xt_loop1 = 0;
    long long xs[8] = {0, 0, 0, 0, 0, 0, 0, 0};      // stamps around the FIRST item boundary of the workgroup (see the benchmark's printout)
    int xt_item_no = 0;
#define XT_STAMP(k_, cond_) if (cond_) xs[k_] = (long long)__builtin_amdgcn_s_memtime();
#else
#define XT_STAMP(k_, cond_)
#endif

    // ---- the items of this workgroup: XCD (blockIdx.x & 7) owns items [lo, lo + cnt), its workgroups walk them with stride n_slots.
    // (gridDim.x == n_items: one item each, at gvf_xcd_remap's position.)
    int item, item_end, item_step;
    {
        const unsigned xcd = blockIdx.x & 7u, slot = blockIdx.x >> 3;
        const unsigned iq = (unsigned)p.n_items >> 3, ir = (unsigned)p.n_items & 7u;
        const unsigned lo = xcd < ir ? xcd * (iq + 1u) : ir * (iq + 1u) + (xcd - ir) * iq, cnt = iq + (xcd < ir ? 1u : 0u);
        const unsigned n_slots = (gridDim.x >> 3) + (xcd < (gridDim.x & 7u) ? 1u : 0u);
        item = (int)(lo + slot); item_end = (int)(lo + cnt); item_step = (int)n_slots;
        if (slot >= cnt) return;                                 // (uniform per workgroup, before any barrier)
    }
    const int T = p.n_tiles;
    const int last_valid = p.Lk - (T - 1) * XT_KT;             // valid keys of the last tile (1..64)
    const int n_stages = (T + XT_TPS - 1) / XT_TPS;

    // ---- staging: stage s = tiles [s * TPS, (s+1) * TPS) -> ring slot s % 3.  Wave w copies chunks [64w, 64w+64) of every
    // K image and of every V^T image of the stage (linear 1 KiB LDS-DMA pieces).
#define XT_TILE_AT(t_) (&smem[((((t_) / XT_TPS) % XT_NBUF) * XT_TPS + (t_) % XT_TPS) * XT_TILE_CHUNKS])
#define XT_STAGE_OF(it_, s_)                                                                           \
    _Pragma("unroll") for (int i_ = 0; i_ < XT_TPS; ++i_) {                                            \
        const int t_ = (s_) * XT_TPS + i_;                                                             \
        if (t_ < T) {                                                                                  \
            uint4* dst_ = XT_TILE_AT(t_);                                                              \
            xt_dma16((it_).kbase + (long long)t_ * 256 + wave * 64 + lane, dst_ + wave * 64);          \
            xt_dma16((it_).vbase + (long long)t_ * 256 + wave * 64 + lane, dst_ + 256 + wave * 64);    \
        }                                                                                              \
    }
#define XT_STAGE(s_) XT_STAGE_OF(cur, s_)
#define XT_K(t_) XT_TILE_AT(t_)
#define XT_V(t_) (XT_TILE_AT(t_) + 256)
    XtItem cur = xt_item(p, item);
    uint4 qraw[2][2];
    {
        const int lane = tid0 & 63;
        // The first two stages are requested BEFORE the query rows: the K / V^T tiles and the queries come from memory at the same time instead
        // of one latency after the other (the fast path's first barrier below waits for them; the exact path stages for itself).
        if (force_safe == 0) {
            XT_STAGE(0)
            if (n_stages > 1) { XT_STAGE(1) }
        }
        xt_load_q(p, cur, wave, lane & 31, lane >> 5, qraw);
    }
    bool first_item = true;

    for (;;) {
    // The lane id is LAUNDERED once per item: everything below derives from it, and left alone the compiler hoists every loop-invariant
    // lane value of the body (fragment addresses, selector constants, row addresses of the stores: ~45 registers) in front of the item loop
    // and keeps them alive across the attention loop -- 28 spilled VGPRs measured; an item's code is meant to be the one-item kernel's.
    int tid = tid0;
    asm volatile("" : "+v"(tid));
    const int lane = tid & 63, half = lane >> 5, l31 = lane & 31;
    // The NEXT item is decoded here, while this one's operands are still on their way (its descriptor then sits in scalar registers across
    // the attention loop): decoded in the tail -- kernel arguments re-read, three integer divisions -- it cost 3.4 k cycles between the
    // guard's barriers and the first request (s_memtime stamps, profiles/r05_attn_xt_item_boundary.txt).  Its query rows are touched
    // (one dword per row into the landing zone nobody reads) so that the tail's real loads find them in L2.
    const bool has_next = item + item_step < item_end;
    XtItem nxt = cur;
    if (has_next) {
        nxt = xt_item(p, item + item_step);
        uint4* pz = &smem[XT_NBUF * XT_TPS * XT_TILE_CHUNKS + 1];
#pragma unroll
        for (int a = 0; a < 2; ++a) {
            const int row = nxt.qb * XT_QB + wave * 64 + a * 32 + l31;
            __builtin_amdgcn_global_load_lds(nxt.qp + (long long)(row < p.Lq ? row : 0) * p.q_sl + 16 * half, (__attribute__((address_space(3))) void*)pz, 4, 0, 0);
        }
    }
    // ---- Q fragments (B operand of S^T = K' Q^T): lane (q = l31, half): Q[q][16 st + 8 half .. +7]
    x8 qf[2][2];
#pragma unroll
    for (int a = 0; a < 2; ++a) {
        const bool qvalid = cur.qb * XT_QB + wave * 64 + a * 32 + l31 < p.Lq;
#pragma unroll
        for (int st = 0; st < 2; ++st) qraw[a][st] = xt_mask_q(qraw[a][st], qvalid);
        if (p.gamma_q != nullptr) {     // fused MultiHeadRMSNorm (model/attention/modules.py:8-15): the row lives in this lane and lane ^ 32
            float ss = xt_sumsq8<DT>(qraw[a][0]) + xt_sumsq8<DT>(qraw[a][1]);
            ss += __shfl_xor(ss, 32, 64);
#pragma unroll
            for (int st = 0; st < 2; ++st) qraw[a][st] = xt_rms_apply<DT>(qraw[a][st], ss, p.gamma_q + cur.head * 32 + 16 * st + 8 * half, 1.0f);
        }
#pragma unroll
        for (int st = 0; st < 2; ++st) qf[a][st] = __builtin_bit_cast(x8, qraw[a][st]);
    }

    uint4* sQw = &smem[XT_NBUF * XT_TPS * XT_TILE_CHUNKS + 1] + wave * 256 + lane;      // xt_phase's unused sQ (see there)

    const f32x16 zero = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    f32x16 oA = zero, oB = zero;
    float lA = 0.f, lB = 0.f;
    f32x4 l4A = {0.f, 0.f, 0.f, 0.f}, l4B = {0.f, 0.f, 0.f, 0.f};
    f32x4 l4Ab = {0.f, 0.f, 0.f, 0.f}, l4Bb = {0.f, 0.f, 0.f, 0.f};     // xt_phase's unused l4b (see there)
    bool bad = force_safe != 0;
    const uint4* const kbase = cur.kbase;
    const uint4* const vbase = cur.vbase;

    if (!bad) {
        f32x16 sA[2], sB[2];
        f32x16 cA = zero, cB = zero;        // fp16: -shift of the lane's query in sub-tile A / B (see xt_take_shift); bf16: unused
        x8 kf[2][2], vf[4];
        // Tile t is consumed in iteration t: phase 1 = QK^T of sub-tile A on K(t) | softmax + PV of sub-tile B on V(t-1),
        // phase 2 = QK^T of B on K(t) | softmax + PV of A on V(t).  Phase 1 refills the V^T fragments with V(t), phase 2
        // the K fragments with K(t+1): tile t+1 must have landed when iteration t starts, so tiles are staged TWO ahead.
        // The first and the last tile are peeled so that the steady-state loop body is branch-free straight-line code
        // (with both variants of a phase behind an if / else the compiler hoists their common exp2 block above the
        // branch and the interleave is gone).
        XT_STAMP(4, xt_item_no == 1)
        __syncthreads();            // stages 0 and 1 have landed (own DMA drained before the barrier)
        XT_STAMP(5, xt_item_no == 1)
#pragma unroll
        for (int s_ = 2; s_ < XT_NBUF; ++s_)
            if (s_ < n_stages) { XT_STAGE(s_) }
        if (p.pf != nullptr && wave == 0 && first_item) {
            // warm the NEXT launch's weights: one dword per 128-byte line, LDS-DMA into a landing zone nobody reads (no register, no wait of
            // its own: the loads ride with the stage requests and are drained by the loop's barriers).  The lines end up in the Infinity
            // Cache (and this XCD's L2), where the row-block launch that follows finds them instead of going to HBM.
            uint4* pz = &smem[XT_NBUF * XT_TPS * XT_TILE_CHUNKS + 1];
            for (int it = 0; it < p.pf_iters; ++it) {
                const long long line = ((long long)it * gridDim.x + blockIdx.x) * 64 + lane;
                if (line < p.pf_lines)
                    __builtin_amdgcn_global_load_lds(p.pf + line * 128, (__attribute__((address_space(3))) void*)pz, 4, 0, 0);
            }
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) kf[i >> 1][i & 1] = xt_ld_k<DT>(XT_K(0), i >> 1, i & 1, l31, half);
        xt_phase<DT, true, false, false, 1, SHIFT>(kf, vf, XT_V(0), qf[0], sQw, sA, sB, oB, l4B, l4Bb, l31, half, XT_KT, cA);
        if (SHIFT) xt_take_shift<DT>(sA, cA);
        if (T > 1) {
            xt_phase<DT, true, true, false, 2, SHIFT>(kf, vf, XT_K(1), qf[1], sQw + 128, sB, sA, oA, l4A, l4Ab, l31, half, XT_KT, cB);
            if (SHIFT) xt_take_shift<DT>(sB, cB);
            // steady state, iterations t = 1 .. T-2.  Entering stage s = t / TPS: one barrier -- stage s+1 has landed
            // (iteration t may prefetch K(t+1) from it) and every wave is done with stage s-1, whose ring slot takes the
            // DMA of stage s+2.
            int t = 1;
            // whole periods of the ring: tile t + j sits at ring position (1 + j) % PER whenever (t - 1) % PER == 0 -- every LDS address of the
            // body is the lane's base plus a constant, the stage test a constant
            constexpr int PER = XT_TPS * XT_NBUF;
#define XT_RING(p_) (&smem[((p_) % PER) * XT_TILE_CHUNKS])
#ifdef XT_TIMING
            long long xt_bar = 0, xt_tiles = 0;
            const long long xt_t0 = (long long)__builtin_amdgcn_s_memtime();
            if (first_item) xt_loop0 = xt_t0;
            XT_STAMP(6, xt_item_no == 1)
#endif
            for (; t + PER < T; t += PER) {
#ifdef XT_TIMING
                xt_tiles += PER;
#endif
#pragma unroll
                for (int j = 0; j < PER; ++j) {
                    if ((1 + j) % XT_TPS == 0) {
#ifdef XT_TIMING
                        const long long b0 = (long long)__builtin_amdgcn_s_memtime();
                        __syncthreads();
                        xt_bar += (long long)__builtin_amdgcn_s_memtime() - b0;
#else
                        __syncthreads();
#endif
                        const int s2 = (t + j) / XT_TPS + (XT_NBUF - 1);
#pragma unroll
                        for (int i_ = 0; i_ < XT_TPS; ++i_) {
                            const int t_ = s2 * XT_TPS + i_;
                            if (t_ < T) {
                                uint4* dst_ = XT_RING((((1 + j) / XT_TPS + (XT_NBUF - 1)) % XT_NBUF) * XT_TPS + i_);
                                xt_dma16(kbase + (long long)t_ * 256 + wave * 64 + lane, dst_ + wave * 64);
                                xt_dma16(vbase + (long long)t_ * 256 + wave * 64 + lane, dst_ + 256 + wave * 64);
                            }
                        }
                    }
                    xt_phase<DT, true, true, false, 1, SHIFT>(kf, vf, XT_RING(1 + j) + 256, qf[0], sQw, sA, sB, oB, l4B, l4Bb, l31, half, XT_KT, cA);
                    xt_phase<DT, true, true, false, 2, SHIFT>(kf, vf, XT_RING(2 + j), qf[1], sQw + 128, sB, sA, oA, l4A, l4Ab, l31, half, XT_KT, cB);
                }
            }
#undef XT_RING
#ifdef XT_TIMING
            if (lane == 0 && p.dbg != nullptr && first_item) {
                long long* d = p.dbg + ((long long)blockIdx.x * 4 + wave) * 4;
                xt_loop1 = (long long)__builtin_amdgcn_s_memtime();
                d[0] = xt_loop1 - xt_t0; d[1] = xt_bar; d[2] = xt_tiles; d[3] = xt_loop0 - xt_k0;
            }
#endif
            for (; t + 1 < T; ++t) {
                if (t % XT_TPS == 0) {
                    __syncthreads();
                    const int s2 = t / XT_TPS + (XT_NBUF - 1);
                    if (s2 < n_stages) { XT_STAGE(s2) }
                }
                xt_phase<DT, true, true, false, 1, SHIFT>(kf, vf, XT_V(t), qf[0], sQw, sA, sB, oB, l4B, l4Bb, l31, half, XT_KT, cA);
                xt_phase<DT, true, true, false, 2, SHIFT>(kf, vf, XT_K(t + 1), qf[1], sQw + 128, sB, sA, oA, l4A, l4Ab, l31, half, XT_KT, cB);
            }
            if ((T - 1) % XT_TPS == 0) __syncthreads();      // the last tile opens a stage: it must have landed
            xt_phase<DT, true, true, false, 1, SHIFT>(kf, vf, XT_V(T - 1), qf[0], sQw, sA, sB, oB, l4B, l4Bb, l31, half, XT_KT, cA);
        }
        xt_phase<DT, true, true, true, 0, SHIFT>(kf, vf, XT_K(0), qf[1], sQw + 128, sB, sA, oA, l4A, l4Ab, l31, half, last_valid, cB);
        if (SHIFT && T == 1) xt_take_shift<DT>(sB, cB);      // a single key tile: sub-tile B's first scores come out of this phase
        xt_phase<DT, false, true, true, 0, SHIFT>(kf, vf, XT_K(0), qf[1], sQw, sA, sB, oB, l4B, l4Bb, l31, half, last_valid, cB);
        lA = __shfl(l4A[0], (l31 & 15) + 32 * (l31 >> 4), 64);      // both key halves are in already
        lB = __shfl(l4B[0], (l31 & 15) + 32 * (l31 >> 4), 64);
        // range guard.  fp16: with the shift the denominator is >= 1 unless a single, partly padded key tile
        // pushed every probability under 2^-12 (the padding's zero scores took part in the shift)
        // fp16 without the shift (bounded scores): every probability is >= 2^-14, so is the sum; below that the promise was broken
        const float l_min = SHIFT ? 0.015625f : (LP::kNeedsShift ? 3.0517578125e-05f : 7.8886e-31f);
        // upper bound: the sum is taken over the ROUNDED probabilities, so an fp16 overflow shows up as l = inf (a sum of the fp32 values would
        // have to bound l below fp16's largest number itself, as attn.hip's kvres kernel does)
        const float l_max = 1.2676e30f;
        // compared as BIT PATTERNS: this file is built with -fno-honor-nans, under which a float comparison may be inverted; as unsigned integers
        // positive floats order like their values, NaNs of either sign and every negative number fall outside [l_min, l_max) by themselves
        // (a NaN is what the selector form of the row sums makes of an infinity: 0 * inf)
        const unsigned u_min = __float_as_uint(l_min), u_span = __float_as_uint(l_max) - __float_as_uint(l_min);
        const bool okA = (__float_as_uint(lA) - u_min - 1u) < (u_span - 1u), okB = (__float_as_uint(lB) - u_min - 1u) < (u_span - 1u);
        bad = !(okA && okB);
    }
    XT_STAMP(0, xt_item_no == 0)
    XT_STAMP(7, xt_item_no == 1)
    if (tid == 0) *s_bad = 0;
    __syncthreads();
    if (bad) *s_bad = 1;
    __syncthreads();
    XT_STAMP(1, xt_item_no == 0)
    if (*s_bad != 0) {
        // exact fallback for the whole workgroup (staging is cooperative): classic online softmax, two sub-tiles per wave
        float mA = -INFINITY, mB = -INFINITY;
        if (tid == 0 && p.fallbacks != nullptr) atomicAdd(p.fallbacks, 1);
        oA = zero; oB = zero; lA = 0.f; lB = 0.f;
        __syncthreads();
        XT_STAGE(0)
        for (int t = 0; t < T; ++t) {
            if (t % XT_TPS == 0) {
                __syncthreads();
                if (t / XT_TPS + 1 < n_stages) { XT_STAGE(t / XT_TPS + 1) }
            }
            const int nv = t + 1 < T ? XT_KT : last_valid;
            xt_safe_tile<DT>(XT_K(t), XT_V(t), qf[0], oA, mA, lA, l31, half, nv);
            xt_safe_tile<DT>(XT_K(t), XT_V(t), qf[1], oB, mB, lB, l31, half, nv);
        }
        lA += __shfl_xor(lA, 32, 64);
        lB += __shfl_xor(lB, 32, 64);
        __syncthreads();            // every wave is done with the ring before the next item's stages may land in it
    }

    // ---- the next item's operands: every wave is past the guard's barriers, i.e. done with the ring -- request the next item's first two
    // stages and its query rows NOW, under this item's normalisation and stores.
    const int l31e = l31, halfe = half, wavee = wave;
    uint4 qnext[2][2];
    if (has_next) {
        if (force_safe == 0) {
            XT_STAGE_OF(nxt, 0)
            if (n_stages > 1) { XT_STAGE_OF(nxt, 1) }
        }
        xt_load_q(p, nxt, wave, l31, half, qnext);
    }
    XT_STAMP(2, xt_item_no == 0)

    // ---- epilogue: O[q][d] / l, d = (r&3) + 8 (r>>2) + 4 half
    const long long o_sl = p.o_sl;
    const int Lq_e = p.Lq;
#pragma unroll
    for (int a = 0; a < 2; ++a) {
        const int qrow_e = cur.qb * XT_QB + wavee * 64 + a * 32 + l31e;
        if (!(qrow_e < Lq_e)) continue;
        const f32x16& o = a == 0 ? oA : oB;
        const float inv = 1.0f / (a == 0 ? lA : lB);
        if (p.out_f32) {
            float* orow = reinterpret_cast<float*>(p.out) + cur.o_off + (long long)qrow_e * o_sl;
#pragma unroll
            for (int g = 0; g < 4; ++g)
                *reinterpret_cast<float4*>(orow + 8 * g + 4 * halfe) = make_float4(o[4 * g] * inv, o[4 * g + 1] * inv, o[4 * g + 2] * inv, o[4 * g + 3] * inv);
            continue;
        }
        unsigned short* orow = p.out + cur.o_off + (long long)qrow_e * o_sl;
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            uint2 w;
            w.x = LP::pack(o[4 * g] * inv, o[4 * g + 1] * inv);
            w.y = LP::pack(o[4 * g + 2] * inv, o[4 * g + 3] * inv);
            *reinterpret_cast<uint2*>(orow + 8 * g + 4 * halfe) = w;
        }
    }
#ifdef XT_TIMING
    XT_STAMP(3, xt_item_no == 0)
    if (lane == 0 && p.dbg != nullptr && xt_loop1 != 0 && first_item)
        p.dbg[((long long)gridDim.x * 4 + (long long)blockIdx.x * 4 + wave) * 4] = (long long)__builtin_amdgcn_s_memtime() - xt_loop1;
    if (lane == 0 && p.dbg != nullptr && xt_item_no == 1) {       // second item done: its boundary stamps, relative to the first item's loop end
        long long* d = p.dbg + (long long)gridDim.x * 32 + ((long long)blockIdx.x * 4 + wave) * 8;
        for (int k = 1; k < 8; ++k) d[k] = xs[k] - xs[0];
        d[0] = 1;
    }
    ++xt_item_no;
#endif
    if (!has_next) break;
    item += item_step;
    cur = nxt;
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int st = 0; st < 2; ++st) qraw[a][st] = qnext[a][st];
    first_item = false;
    }
#undef XT_STAGE
#undef XT_STAGE_OF
#undef XT_TILE_AT
#undef XT_K
#undef XT_V
}

// ---------------------------------------------------------------------------------------------------------------
// Cache builder: kv rows (fp32 or bf16; K at column k_col0 + h*32, V at v_col0 + h*32 of row set*L + key) -> tiled images.
// One workgroup = one (set, head, 64-key tile): thread (key = tid >> 2, c = tid & 3) loads the 8 K values and the 8 V values
// of its 16-byte chunk (coalesced 64 / 128-byte row pieces), K goes out directly (RMSNorm over the 4 lanes of a key row,
// scale, one rounding), V is transposed through LDS; both 4 KiB images are written as contiguous 16-byte chunks.
// Cheap enough (~2 x the bytes it moves at HBM speed) to run per denoise step for the self attention's K / V as well.
// ---------------------------------------------------------------------------------------------------------------
template <int DT>
__device__ __forceinline__ void xt_ld8(const float* p, float (&v)[8]) {
    const float4 a = *reinterpret_cast<const float4*>(p), b = *reinterpret_cast<const float4*>(p + 4);
    v[0] = a.x; v[1] = a.y; v[2] = a.z; v[3] = a.w; v[4] = b.x; v[5] = b.y; v[6] = b.z; v[7] = b.w;
}
template <int DT>
__device__ __forceinline__ void xt_ld8(const unsigned short* p, float (&v)[8]) {
    const uint4 r = *reinterpret_cast<const uint4*>(p);
    const unsigned w[4] = {r.x, r.y, r.z, r.w};
#pragma unroll
    for (int i = 0; i < 4; ++i) { v[2 * i] = GvfLp<DT>::lo(w[i]); v[2 * i + 1] = GvfLp<DT>::hi(w[i]); }
}

constexpr int XT_PK_LD = 40;     // bf16 pitch of the staged V rows (80 B): the column gathers of a wave spread over the banks

template <typename TIn, int DT>
__global__ __launch_bounds__(256) void attn_pack_kv_kernel(const TIn* __restrict__ kv, long long ld, int k_col0, int v_col0, int L, int H,
                                                           int n_tiles, float k_scale, const float* __restrict__ gamma_k,
                                                           const int* __restrict__ key_order, uint4* __restrict__ kt, uint4* __restrict__ vt,
                                                           long long group_stride, long long n_sets) {
    __shared__ unsigned short sV[XT_KT * XT_PK_LD];
    const int tid = threadIdx.x;
    // blockIdx.y = group (gvf_attn_pack_kv_groups: the 12 blocks' to_kv products of one context in ONE launch): its rows start group_stride
    // elements further, its gain / order / images follow the previous group's
    if (blockIdx.y != 0) {
        const long long g = blockIdx.y;
        kv += g * group_stride;
        if (gamma_k != nullptr) gamma_k += g * H * 32;
        if (key_order != nullptr) key_order += g * n_sets * H * L;
        kt += g * n_sets * H * n_tiles * 256; vt += g * n_sets * H * n_tiles * 256;
    }
    long long rest = blockIdx.x;
    const int tile = (int)(rest % n_tiles); rest /= n_tiles;
    const int h = (int)(rest % H);
    const long long set = rest / H;
    const int key_l = tid >> 2, c = tid & 3, key = tile * XT_KT + key_l;
    const bool valid = key < L;
    // key_order (optional, [set][head][L]): slot `key` of this (set, head) holds source row key_order[..][key] -- a permutation of the keys
    // (softmax attention does not depend on their order; K and V move together)
    const int src_key = valid ? (key_order != nullptr ? key_order[(set * H + h) * L + key] : key) : 0;
    const TIn* row = kv + (set * L + src_key) * ld + h * 32 + 8 * c;
    float k8[8], v8[8];
    xt_ld8<DT>(row + k_col0, k8);
    xt_ld8<DT>(row + v_col0, v8);
    float mul = k_scale;
    if (gamma_k != nullptr) {           // MultiHeadRMSNorm of the key row in fp32, then the softmax scale: ONE rounding
        float ss = 0.f;
#pragma unroll
        for (int e = 0; e < 8; ++e) ss += k8[e] * k8[e];
        ss += __shfl_xor(ss, 1, 64);
        ss += __shfl_xor(ss, 2, 64);
        mul = k_scale * 5.656854249492381f / fmaxf(sqrtf(ss), 1e-12f);
    }
    unsigned kw[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const float g0 = gamma_k != nullptr ? gamma_k[h * 32 + 8 * c + 2 * i] : 1.0f, g1 = gamma_k != nullptr ? gamma_k[h * 32 + 8 * c + 2 * i + 1] : 1.0f;
        kw[i] = valid ? GvfLp<DT>::pack(k8[2 * i] * mul * g0, k8[2 * i + 1] * mul * g1) : 0u;
    }
    const long long base = ((set * H + h) * n_tiles + tile) * 256;
    kt[base + key_l * 4 + (c ^ ((key_l >> 2) & 3))] = make_uint4(kw[0], kw[1], kw[2], kw[3]);
#pragma unroll
    for (int i = 0; i < 4; ++i)
        *reinterpret_cast<unsigned*>(&sV[key_l * XT_PK_LD + 8 * c + 2 * i]) = valid ? GvfLp<DT>::pack(v8[2 * i], v8[2 * i + 1]) : 0u;
    __syncthreads();
    const int d = tid >> 3, pos = tid & 7, j = pos ^ ((d >> 1) & 7), g = j >> 1, hf = j & 1;
    unsigned vw[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int e0 = 2 * i, e1 = 2 * i + 1;
        const unsigned lo = sV[(16 * g + 4 * hf + (e0 & 3) + 8 * (e0 >> 2)) * XT_PK_LD + d];
        const unsigned hi = sV[(16 * g + 4 * hf + (e1 & 3) + 8 * (e1 >> 2)) * XT_PK_LD + d];
        vw[i] = lo | (hi << 16);
    }
    vt[base + d * 8 + pos] = make_uint4(vw[0], vw[1], vw[2], vw[3]);
}

// Key order of a cross attention's cache (gvf_attn_pack_kv_ordered): the n_first largest-norm keys of every (set, head) first, everything else
// behind them, both groups in context order (a stable partition -- all the fp16 kernel's first-tile shift needs; a full sort by norm cost 2.7 ms
// per sample through torch.sort).  One workgroup per (set, head): squared norms as ordered integers in LDS, the n_first-th largest by a
// 4 x 8-bit radix select over them (ties at the threshold: the first ones in context order), then ballot prefix sums hand out the slots.
constexpr int KO_THREADS = 256, KO_MAX_L = 8192;
__global__ __launch_bounds__(KO_THREADS) void key_order_kernel(const float* __restrict__ kv, long long ld, int k_col0, int L, int H, int n_first,
                                                               int* __restrict__ order, long long group_stride, long long n_sets) {
    extern __shared__ unsigned sN[];              // L words (up to KO_MAX_L = 32 KiB): sized by the launch so that short contexts fill the CUs
    kv += (long long)blockIdx.y * group_stride;   // blockIdx.y = group (gvf_attn_key_order_groups)
    order += (long long)blockIdx.y * n_sets * H * L;
    __shared__ unsigned sHist[256];
    __shared__ unsigned sSel[4];                 // prefix, remaining, (partition) running counts
    __shared__ unsigned sWave[2][KO_THREADS / 64];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int h = blockIdx.x % H;
    const long long set = blockIdx.x / H;
    for (int k = tid; k < L; k += KO_THREADS) {
        const float4* r = reinterpret_cast<const float4*>(kv + (set * L + k) * ld + k_col0 + h * 32);
        float ss = 0.f;
#pragma unroll
        for (int i = 0; i < 8; ++i) { const float4 v = r[i]; ss += (v.x * v.x + v.y * v.y) + (v.z * v.z + v.w * v.w); }
        sN[k] = (ss == ss) ? __float_as_uint(ss) : 0u;            // non-negative floats order like their bit patterns; a NaN row sorts last
    }
    const int want = n_first < L ? n_first : L;
    if (tid == 0) { sSel[0] = 0u; sSel[1] = (unsigned)want; }
    __syncthreads();
    // radix select, most significant byte first: after the loop sSel[0] = the want-th largest value, sSel[1] = how many keys EQUAL to it are taken
    for (int shift = 24; shift >= 0; shift -= 8) {
        sHist[tid] = 0u;
        __syncthreads();
        const unsigned prefix = sSel[0], hi_mask = shift == 24 ? 0u : (0xffffffffu << (shift + 8));
        for (int k = tid; k < L; k += KO_THREADS) {
            const unsigned v = sN[k];
            if ((v & hi_mask) == prefix) atomicAdd(&sHist[(v >> shift) & 255u], 1u);
        }
        __syncthreads();
        {   // the digit d whose bin holds the rem-th largest candidate: above(d) < rem <= above(d) + hist[d], above(d) = candidates with a larger
            // digit.  Every thread sums the bins above its own (LDS broadcast reads; one thread doing the scan alone was 50 us per workgroup)
            const unsigned rem = sSel[1], mine = sHist[tid];
            unsigned above = 0u;
            for (int j = tid + 1; j < 256; ++j) above += sHist[j];
            __syncthreads();                                 // (everyone has read sSel[1])
            if (above < rem && rem <= above + mine) { sSel[0] = prefix | ((unsigned)tid << shift); sSel[1] = rem - above; }
        }
        __syncthreads();
    }
    const unsigned thr = sSel[0], n_eq = sSel[1];
    // stable partition: a key goes first if it is above the threshold, or equal to it and among the first n_eq such keys
    unsigned base_first = 0u, base_rest = (unsigned)want, seen_eq = 0u;
    for (int k0 = 0; k0 < L; k0 += KO_THREADS) {
        const int k = k0 + tid;
        const unsigned v = k < L ? sN[k] : 0u;
        const bool gt = k < L && v > thr, eq = k < L && v == thr;
        // equal keys: rank among equals so far (workgroup-wide exclusive count)
        const unsigned long long beq = __ballot(eq);
        if (lane == 0) sWave[0][wave] = (unsigned)__popcll(beq);
        __syncthreads();
        unsigned eq_before = seen_eq, eq_total = 0u;
        for (int w = 0; w < KO_THREADS / 64; ++w) { if (w < wave) eq_before += sWave[0][w]; eq_total += sWave[0][w]; }
        eq_before += (unsigned)__popcll(beq & ((1ull << lane) - 1ull));
        const bool first = gt || (eq && eq_before < n_eq);
        __syncthreads();
        const unsigned long long bf = __ballot(first), br = __ballot(k < L && !first);
        if (lane == 0) { sWave[0][wave] = (unsigned)__popcll(bf); sWave[1][wave] = (unsigned)__popcll(br); }
        __syncthreads();
        unsigned f_before = base_first, r_before = base_rest, f_total = 0u, r_total = 0u;
        for (int w = 0; w < KO_THREADS / 64; ++w) {
            if (w < wave) { f_before += sWave[0][w]; r_before += sWave[1][w]; }
            f_total += sWave[0][w]; r_total += sWave[1][w];
        }
        if (k < L) {
            const unsigned slot = first ? f_before + (unsigned)__popcll(bf & ((1ull << lane) - 1ull)) : r_before + (unsigned)__popcll(br & ((1ull << lane) - 1ull));
            order[(set * H + h) * L + slot] = k;
        }
        base_first += f_total; base_rest += r_total; seen_eq += eq_total;
        __syncthreads();
    }
}

}  // namespace

extern "C" int gvf_attn_key_order_groups(const float* kv, int64_t ld, int64_t group_stride, int n_groups, int k_col0, int n_sets, int L, int H, int n_first,
                                         int32_t* key_order, void* stream_) {
    if (n_sets < 0 || n_groups < 0 || n_groups > 65535 || group_stride < 0 || L <= 0 || L > KO_MAX_L || H <= 0 || ld <= 0 || k_col0 < 0 || n_first <= 0 ||
        (ld % 4) || (k_col0 % 4) || (group_stride % 4))
        return GVF_EINVAL;
    if (n_sets == 0 || n_groups == 0) return GVF_OK;
    if (!kv || !key_order || (((uintptr_t)kv) & 15)) return GVF_EINVAL;
    const long long blocks = (long long)n_sets * H;
    if (blocks > 0x7fffffffLL) return GVF_EINVAL;
    (void)hipGetLastError();
    key_order_kernel<<<dim3((unsigned)blocks, (unsigned)n_groups), dim3(KO_THREADS), (size_t)L * sizeof(unsigned), (hipStream_t)stream_>>>(
        kv, (long long)ld, k_col0, L, H, n_first, key_order, (long long)group_stride, (long long)n_sets);
    GVF_CHECK_LAUNCH();
    return GVF_OK;
}

extern "C" int gvf_attn_key_order(const float* kv, int64_t ld, int k_col0, int n_sets, int L, int H, int n_first, int32_t* key_order, void* stream_) {
    return gvf_attn_key_order_groups(kv, ld, 0, 1, k_col0, n_sets, L, H, n_first, key_order, stream_);
}

extern "C" int gvf_attn_pack_kv(int dtype, const void* kv, int kv_is_f32, int64_t ld, int k_col0, int v_col0, int n_sets, int L, int H,
                                float k_scale, const float* gamma_k, void* k_tiles, void* v_tiles, void* stream_) {
    return gvf_attn_pack_kv_ordered(dtype, kv, kv_is_f32, ld, k_col0, v_col0, n_sets, L, H, k_scale, gamma_k, nullptr, k_tiles, v_tiles, stream_);
}

extern "C" int gvf_attn_pack_kv_ordered(int dtype, const void* kv, int kv_is_f32, int64_t ld, int k_col0, int v_col0, int n_sets, int L, int H,
                                        float k_scale, const float* gamma_k, const int32_t* key_order, void* k_tiles, void* v_tiles, void* stream_) {
    return gvf_attn_pack_kv_groups(dtype, kv, kv_is_f32, ld, 0, 1, k_col0, v_col0, n_sets, L, H, k_scale, gamma_k, key_order, k_tiles, v_tiles, stream_);
}

extern "C" int gvf_attn_pack_kv_groups(int dtype, const void* kv, int kv_is_f32, int64_t ld, int64_t group_stride, int n_groups, int k_col0, int v_col0,
                                       int n_sets, int L, int H, float k_scale, const float* gamma_k, const int32_t* key_order, void* k_tiles,
                                       void* v_tiles, void* stream_) {
    if (dtype != GVF_DT_BF16 && dtype != GVF_DT_F16) return GVF_EINVAL;
    if (n_sets < 0 || n_groups < 0 || n_groups > 65535 || group_stride < 0 || L <= 0 || H <= 0 || ld <= 0 || k_col0 < 0 || v_col0 < 0) return GVF_EINVAL;
    if (n_sets == 0 || n_groups == 0) return GVF_OK;
    if (!kv || !k_tiles || !v_tiles) return GVF_EINVAL;
    if ((((uintptr_t)k_tiles) & 15) || (((uintptr_t)v_tiles) & 15)) return GVF_EINVAL;
    const int n_tiles = (L + XT_KT - 1) / XT_KT;
    const long long blocks = (long long)n_sets * H * n_tiles;
    if (blocks > 0x7fffffffLL) return GVF_EINVAL;
    // 16-byte (bf16) / 2 x 16-byte (fp32) row pieces: the row pitch and the two column offsets must keep that alignment
    const int al = kv_is_f32 ? 4 : 8;
    if ((ld % al) || (k_col0 % al) || (v_col0 % al) || (group_stride % al) || (((uintptr_t)kv) & 15)) return GVF_EINVAL;
    hipStream_t stream = (hipStream_t)stream_;
    const dim3 grid((unsigned)blocks, (unsigned)n_groups);
    (void)hipGetLastError();
    GVF_LP_DISPATCH(dtype,
        if (kv_is_f32)
            attn_pack_kv_kernel<float, DT><<<grid, dim3(256), 0, stream>>>((const float*)kv, ld, k_col0, v_col0, L, H, n_tiles, k_scale, gamma_k, key_order,
                                                                           (uint4*)k_tiles, (uint4*)v_tiles, (long long)group_stride, (long long)n_sets);
        else
            attn_pack_kv_kernel<unsigned short, DT><<<grid, dim3(256), 0, stream>>>((const unsigned short*)kv, ld, k_col0, v_col0, L, H, n_tiles, k_scale,
                                                                                    gamma_k, key_order, (uint4*)k_tiles, (uint4*)v_tiles,
                                                                                    (long long)group_stride, (long long)n_sets));
    GVF_CHECK_LAUNCH();
    return GVF_OK;
}

extern "C" int gvf_attn_pack_kv_bf16(const void* kv, int kv_is_f32, int64_t ld, int k_col0, int v_col0, int n_sets, int L, int H,
                                     float k_scale, const float* gamma_k, void* k_tiles, void* v_tiles, void* stream_) {
    return gvf_attn_pack_kv(GVF_DT_BF16, kv, kv_is_f32, ld, k_col0, v_col0, n_sets, L, H, k_scale, gamma_k, k_tiles, v_tiles, stream_);
}

// resident workgroups of attn_xt_kernel on the current device: XT_WAVES_PER_SIMD of them per CU (its register and LDS budgets are cut for that)
static unsigned xt_resident_workgroups() {
    static GvfPerDeviceOnce once;
    static int cus[64];
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) { (void)hipGetLastError(); return 512u; }
    gvf_once_per_device(once, [dev] {
        int n = 0;
        if (hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || n <= 0) n = 256;
        cus[dev] = n;
        return true;
    });
    return (unsigned)(cus[dev] > 0 ? cus[dev] : 256) * XT_WAVES_PER_SIMD;
}

template <int DT>
static void xt_launch(const XtParams& p, int force_safe, bool bounded, unsigned blocks, hipStream_t stream) {
    if constexpr (GvfLp<DT>::kNeedsShift) {            // (bf16 has no shifted variant: nothing to instantiate)
        if (!bounded) { attn_xt_kernel<DT, true><<<dim3(blocks), dim3(XT_THREADS), 0, stream>>>(p, force_safe); return; }
    }
    attn_xt_kernel<DT, false><<<dim3(blocks), dim3(XT_THREADS), 0, stream>>>(p, force_safe);
}

extern "C" int gvf_attn_tiled_fwd_pf(int dtype, const void* q, const void* k_tiles, const void* v_tiles, void* out, int n_outer, int n_inner,
                                  int Lq, int Lk, int H, const int64_t* q_strides, const int64_t* o_strides,
                                  int64_t kv_set_stride_outer, int64_t kv_set_stride_inner, const float* gamma_q, int out_is_f32,
                                  int force_exact, int32_t* fallback_counter, const void* prefetch, int64_t prefetch_bytes, void* stream_) {
    if (dtype != GVF_DT_BF16 && dtype != GVF_DT_F16) return GVF_EINVAL;
    if (n_outer < 0 || n_inner <= 0 || Lq < 0 || Lk <= 0 || H <= 0) return GVF_EINVAL;
    if (n_outer == 0 || Lq == 0) return GVF_OK;
    if (!q || !k_tiles || !v_tiles || !out || !q_strides || !o_strides) return GVF_EINVAL;
    for (int i = 0; i < 4; ++i)
        if ((q_strides[i] % 8) || (o_strides[i] % 4)) return GVF_EINVAL;
    if ((((uintptr_t)q) & 15) || (((uintptr_t)k_tiles) & 15) || (((uintptr_t)v_tiles) & 15) || (((uintptr_t)out) & (out_is_f32 ? 15 : 7))) return GVF_EINVAL;
    XtParams p;
    p.q = (const unsigned short*)q; p.out = (unsigned short*)out;
    p.kt = (const uint4*)k_tiles; p.vt = (const uint4*)v_tiles;
    p.n_outer = n_outer; p.n_inner = n_inner; p.Lq = Lq; p.Lk = Lk; p.H = H;
    p.q_blocks = (Lq + XT_QB - 1) / XT_QB;
    p.n_tiles = (Lk + XT_KT - 1) / XT_KT;
    p.q_so = q_strides[0]; p.q_si = q_strides[1]; p.q_sl = q_strides[2]; p.q_sh = q_strides[3];
    p.o_so = o_strides[0]; p.o_si = o_strides[1]; p.o_sl = o_strides[2]; p.o_sh = o_strides[3];
    p.kv_so = kv_set_stride_outer; p.kv_si = kv_set_stride_inner;
    p.fallbacks = fallback_counter;
#ifdef XT_TIMING
    p.dbg = g_xt_dbg;
#endif
    p.gamma_q = gamma_q;
    p.out_f32 = out_is_f32;
    if (prefetch_bytes < 0 || (prefetch_bytes > 0 && !prefetch)) return GVF_EINVAL;
    p.pf = prefetch_bytes > 0 ? (const char*)prefetch : nullptr; p.pf_lines = prefetch_bytes / 128; p.pf_iters = 0;
    long long blocks = (long long)p.q_blocks * H * n_inner * n_outer;
    if (blocks > 0x7fffffffLL) return GVF_EINVAL;
    p.n_items = (int)blocks;
    // no more workgroups than are resident at once: each walks its share of the items (see attn_xt_kernel)
    const long long res = (long long)xt_resident_workgroups();
    if (blocks > res) blocks = res;
    if (p.pf != nullptr) p.pf_iters = (int)((p.pf_lines + blocks * 64 - 1) / (blocks * 64));
    (void)hipGetLastError();
    const int force_safe = force_exact & GVF_ATTN_FORCE_EXACT;
    const bool bounded = (force_exact & GVF_ATTN_SCORES_BOUNDED) != 0;
    GVF_LP_DISPATCH(dtype, xt_launch<DT>(p, force_safe, bounded, (unsigned)blocks, (hipStream_t)stream_));
    GVF_CHECK_LAUNCH();
    return GVF_OK;
}

extern "C" int gvf_attn_tiled_fwd(int dtype, const void* q, const void* k_tiles, const void* v_tiles, void* out, int n_outer, int n_inner,
                                  int Lq, int Lk, int H, const int64_t* q_strides, const int64_t* o_strides,
                                  int64_t kv_set_stride_outer, int64_t kv_set_stride_inner, const float* gamma_q, int out_is_f32,
                                  int force_exact, int32_t* fallback_counter, void* stream_) {
    return gvf_attn_tiled_fwd_pf(dtype, q, k_tiles, v_tiles, out, n_outer, n_inner, Lq, Lk, H, q_strides, o_strides, kv_set_stride_outer,
                                 kv_set_stride_inner, gamma_q, out_is_f32, force_exact, fallback_counter, nullptr, 0, stream_);
}

extern "C" int gvf_attn_tiled_fwd_bf16(const void* q, const void* k_tiles, const void* v_tiles, void* out, int n_outer, int n_inner,
                                       int Lq, int Lk, int H, const int64_t* q_strides, const int64_t* o_strides,
                                       int64_t kv_set_stride_outer, int64_t kv_set_stride_inner, const float* gamma_q, int out_is_f32,
                                       int force_exact, int32_t* fallback_counter, void* stream_) {
    return gvf_attn_tiled_fwd(GVF_DT_BF16, q, k_tiles, v_tiles, out, n_outer, n_inner, Lq, Lk, H, q_strides, o_strides, kv_set_stride_outer,
                              kv_set_stride_inner, gamma_q, out_is_f32, force_exact, fallback_counter, stream_);
}
