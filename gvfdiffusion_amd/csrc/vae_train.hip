// vae_train.hip -- the training kernels of the motion VAE that are not matrix products or attention, for gfx950 (include/gvf_vae_train.h):
// GEGLU, the point / Gaussian embedding and the grouped posterior with the reference's clamp, each forward and backward.
//
// Reference: model/autoencoder.py:90-93 (GEGLU: x * F.gelu(gates), the exact erf form), :250-301 and :392-394 (PointEmbed, the two embedding
// LayerNorms with eps 1e-5, their sum at :532-535 and :560), :304-342 (DiagonalGaussianDistribution: clamp(logvar, -30, 20), sample, kl over
// dims [1, 2]).  Under autocast the reference runs each as a chain of launches and saves every intermediate; here each is one launch each way
// (two where a reduction needs its finaliser) and the backward recomputes from the operator's inputs.
// fp32 inside, 16-bit only at the loads and stores of GEGLU.  Reductions: one partial per workgroup in its own workspace slot, added in slot
// order in double by a finaliser: no atomics, same bits every run.
#include <cfloat>
#include <cmath>
#include "gvf_common.h"
#include "gvf_lp.h"
#include "gvf_rowops.h"
#include "../../include/gvf_rast.h"
#include "../../include/gvf_dit.h"
#include "../../include/gvf_vae_train.h"

namespace {

constexpr int WG = 256;

// ---- a. GEGLU -----------------------------------------------------------------------------------------------------------------------------
constexpr float RSQRT2 = 0.70710678118654752440f, INV_SQRT_2PI = 0.39894228040143267794f, GEGLU_CUT = 14.0f;

__device__ __forceinline__ void geglu_bwd_one(float x, float g, float da, float& dx, float& dg) {
    const float cdf = 0.5f * (1.0f + erff(g * RSQRT2));
    // g phi(g): exp(-g^2 / 2) is 0 in fp32 long before g^2 overflows, and from |g| = 14 on the term (< 2e-42) is cut to an exact 0
    const float gp = fabsf(g) < GEGLU_CUT ? g * (INV_SQRT_2PI * __expf(-0.5f * (g * g))) : 0.0f;
    dx = da * gvf_gelu_erf(g);
    // x (Phi + g phi) can overflow for a bf16 x near the largest finite value; held at +-FLT_MAX so that a zero da gives 0 and not inf * 0
    const float p = fminf(fmaxf(x * (cdf + gp), -FLT_MAX), FLT_MAX);
    dg = da * p;
}

// one 16-byte vector of 8 columns per thread: vector i is columns 8 (i % f8) .. of row i / f8
template <int DT>
__global__ __launch_bounds__(WG) void geglu_fwd_kernel(const unsigned short* __restrict__ u, long long ldu, unsigned short* __restrict__ a, long long lda,
                                                       long long total, int f8, int F) {
    const long long i = (long long)blockIdx.x * WG + threadIdx.x;
    if (i >= total) return;
    const long long r = i / f8;
    const int c = (int)(i - r * f8) << 3;
    float x[8], g[8], o[8];
    gvf_unpack8<DT>(*reinterpret_cast<const uint4*>(u + r * ldu + c), x);
    gvf_unpack8<DT>(*reinterpret_cast<const uint4*>(u + r * ldu + F + c), g);
#pragma unroll
    for (int e = 0; e < 8; ++e) o[e] = x[e] * gvf_gelu_erf(g[e]);
    *reinterpret_cast<uint4*>(a + r * lda + c) = gvf_pack8<DT>(o);
}

template <int DT>
__global__ __launch_bounds__(WG) void geglu_bwd_kernel(const unsigned short* __restrict__ u, long long ldu, const unsigned short* __restrict__ da,
                                                       long long ldda, unsigned short* __restrict__ du, long long lddu, long long total, int f8, int F) {
    const long long i = (long long)blockIdx.x * WG + threadIdx.x;
    if (i >= total) return;
    const long long r = i / f8;
    const int c = (int)(i - r * f8) << 3;
    float x[8], g[8], d[8], dx[8], dg[8];
    gvf_unpack8<DT>(*reinterpret_cast<const uint4*>(u + r * ldu + c), x);
    gvf_unpack8<DT>(*reinterpret_cast<const uint4*>(u + r * ldu + F + c), g);
    gvf_unpack8<DT>(*reinterpret_cast<const uint4*>(da + r * ldda + c), d);
#pragma unroll
    for (int e = 0; e < 8; ++e) geglu_bwd_one(x[e], g[e], d[e], dx[e], dg[e]);
    *reinterpret_cast<uint4*>(du + r * lddu + c) = gvf_pack8<DT>(dx);
    *reinterpret_cast<uint4*>(du + r * lddu + F + c) = gvf_pack8<DT>(dg);
}

// ---- b. embedding -------------------------------------------------------------------------------------------------------------------------
// One wave per row; lane l owns channels l, l + 64, ... (NI of them: 3 up to C = 192, 12 up to C = 768).  W (pitch qdim | 1: neighbouring lanes
// on distinct banks), the bias and omega sit in LDS.  A workgroup takes rows_per_wg consecutive rows (emb_rows_per_wg: a function of P alone),
// wave w the rows w, w + 4, ...  A row is a chain of dependent wave reductions and the backward runs one wave per SIMD (its dW accumulators
// fill the register file), so the row count per workgroup is kept small enough to spread P rows over about 512 workgroups.
constexpr int EMB_MAXQ = 16;
constexpr int EMB_MAXC = 768;
constexpr int EMB_MAX_ROWS = 256;

struct EmbLds {
    float* W; float* B; float* Om; int pitch;
};

__device__ __forceinline__ EmbLds emb_stage(float* smem, const float* __restrict__ W, const float* __restrict__ bias, const float* __restrict__ omega,
                                            int qdim, int C) {
    EmbLds s;
    s.pitch = qdim | 1;
    s.W = smem;
    s.B = smem + (size_t)C * s.pitch;
    s.Om = s.B + C;
    for (int i = threadIdx.x; i < C * qdim; i += WG) s.W[(i / qdim) * s.pitch + (i % qdim)] = W[i];
    for (int i = threadIdx.x; i < C; i += WG) s.B[i] = bias[i];
    for (int i = threadIdx.x; i < C / 6; i += WG) s.Om[i] = omega[i];
    __syncthreads();
    return s;
}

// the row's raw Linear output u and PointEmbed value v on this lane's channels (0 on channels >= C), and d v / d coordinate
template <int NI>
__device__ __forceinline__ void emb_raw(const EmbLds& s, const float (&qv)[EMB_MAXQ], int qdim, int C, int lane, float (&u)[NI], float (&v)[NI],
                                        float (&dvdp)[NI]) {
    const int E = C / 6;
#pragma unroll
    for (int i = 0; i < NI; ++i) {
        const int c = lane + 64 * i;
        u[i] = 0.f; v[i] = 0.f; dvdp[i] = 0.f;
        if (c < C) {
            float acc = 0.f;
#pragma unroll
            for (int k = 0; k < EMB_MAXQ; ++k)
                if (k < qdim) acc = fmaf(qv[k], s.W[c * s.pitch + k], acc);
            u[i] = acc + s.B[c];
            const int axis = c / (2 * E), j = c - axis * 2 * E;
            const float p = axis == 0 ? qv[0] : (axis == 1 ? qv[1] : qv[2]);
            const float om = s.Om[j < E ? j : j - E];
            const float sn = sinf(p * om), cs = cosf(p * om);
            v[i] = j < E ? sn : cs;
            dvdp[i] = j < E ? cs * om : -sn * om;
        }
    }
}

// t -> (t - mean) rstd on the valid channels (0 elsewhere); returns rstd.  Two passes, as torch's LayerNorm.
template <int NI>
__device__ __forceinline__ float emb_layernorm(float (&t)[NI], int C, int lane, float eps) {
    float sum = 0.f;
#pragma unroll
    for (int i = 0; i < NI; ++i) sum += t[i];                          // channels >= C hold 0
    const float mean = gvf_wave_sum_xor(sum) / (float)C;
    float q = 0.f;
#pragma unroll
    for (int i = 0; i < NI; ++i)
        if (lane + 64 * i < C) { const float d = t[i] - mean; q += d * d; }
    const float rstd = 1.0f / sqrtf(gvf_wave_sum_xor(q) / (float)C + eps);
#pragma unroll
    for (int i = 0; i < NI; ++i) t[i] = lane + 64 * i < C ? (t[i] - mean) * rstd : 0.f;
    return rstd;
}

template <int NI>
__global__ __launch_bounds__(WG) void embed_fwd_kernel(const float* __restrict__ r, int qdim, const float* __restrict__ W, const float* __restrict__ bias,
                                                       const float* __restrict__ omega, float* __restrict__ e, long long P, int C, float eps,
                                                       int rows_per_wg) {
    extern __shared__ float smem[];
    const EmbLds s = emb_stage(smem, W, bias, omega, qdim, C);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long long row0 = (long long)blockIdx.x * rows_per_wg;
    for (int rr = wave; rr < rows_per_wg; rr += 4) {
        const long long row = row0 + rr;
        if (row >= P) break;
        float qv[EMB_MAXQ];
#pragma unroll
        for (int k = 0; k < EMB_MAXQ; ++k) qv[k] = k < qdim ? r[row * qdim + k] : 0.f;
        float u[NI], v[NI], dvdp[NI];
        emb_raw<NI>(s, qv, qdim, C, lane, u, v, dvdp);
        emb_layernorm<NI>(u, C, lane, eps);
        emb_layernorm<NI>(v, C, lane, eps);
#pragma unroll
        for (int i = 0; i < NI; ++i) {
            const int c = lane + 64 * i;
            if (c < C) e[row * C + c] = u[i] + v[i];
        }
    }
}

// dW / db: a lane adds its channels' terms over its wave's rows in registers; the four waves then add into one LDS image in wave order (the
// region W occupied, free once every wave has left the row loop), which becomes the workgroup's slot [C * qdim | C] of `part`.
// dr: sixteen per-lane sums to sixteen wave totals by a halving exchange (8 + 4 + 2 + 1 + 1 + 1 shuffles): lane 4 k ends with column k.
template <int NI>
__global__ __launch_bounds__(WG) void embed_bwd_kernel(const float* __restrict__ r, int qdim, const float* __restrict__ W, const float* __restrict__ bias,
                                                       const float* __restrict__ omega, const float* __restrict__ de, float* __restrict__ dr,
                                                       float* __restrict__ part, long long P, int C, float eps, int rows_per_wg) {
    extern __shared__ float smem[];
    const EmbLds s = emb_stage(smem, W, bias, omega, qdim, C);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long long row0 = (long long)blockIdx.x * rows_per_wg;
    float accW[NI][EMB_MAXQ], accB[NI];
#pragma unroll
    for (int i = 0; i < NI; ++i) {
        accB[i] = 0.f;
#pragma unroll
        for (int k = 0; k < EMB_MAXQ; ++k) accW[i][k] = 0.f;
    }
    const float invC = 1.0f / (float)C;
    for (int rr = wave; rr < rows_per_wg; rr += 4) {
        const long long row = row0 + rr;
        if (row >= P) break;
        float qv[EMB_MAXQ];
#pragma unroll
        for (int k = 0; k < EMB_MAXQ; ++k) qv[k] = k < qdim ? r[row * qdim + k] : 0.f;
        float u[NI], v[NI], dvdp[NI], d[NI];
        emb_raw<NI>(s, qv, qdim, C, lane, u, v, dvdp);
        const float ru = emb_layernorm<NI>(u, C, lane, eps);          // u, v now hold the normalised rows
        const float rv = emb_layernorm<NI>(v, C, lane, eps);
        float sd = 0.f, su = 0.f, sv = 0.f;
#pragma unroll
        for (int i = 0; i < NI; ++i) {
            const int c = lane + 64 * i;
            d[i] = c < C ? de[row * C + c] : 0.f;
            sd += d[i]; su += d[i] * u[i]; sv += d[i] * v[i];
        }
        const float md = gvf_wave_sum_xor(sd) * invC, au = gvf_wave_sum_xor(su) * invC, av = gvf_wave_sum_xor(sv) * invC;
        float t[EMB_MAXQ];
#pragma unroll
        for (int k = 0; k < EMB_MAXQ; ++k) t[k] = 0.f;
#pragma unroll
        for (int i = 0; i < NI; ++i) {
            const int c = lane + 64 * i;
            if (c < C) {
                const float du = ru * ((d[i] - md) - u[i] * au);
                const float dv = rv * ((d[i] - md) - v[i] * av);
                accB[i] += du;
#pragma unroll
                for (int k = 0; k < EMB_MAXQ; ++k)
                    if (k < qdim) accW[i][k] = fmaf(du, qv[k], accW[i][k]);
                if (dr != nullptr) {
#pragma unroll
                    for (int k = 0; k < EMB_MAXQ; ++k)
                        if (k < qdim) t[k] = fmaf(du, s.W[c * s.pitch + k], t[k]);
                    const int axis = c / (2 * (C / 6));
                    const float g = dv * dvdp[i];
                    t[0] += axis == 0 ? g : 0.f;
                    t[1] += axis == 1 ? g : 0.f;
                    t[2] += axis == 2 ? g : 0.f;
                }
            }
        }
        if (dr != nullptr) {                                          // (uniform over the workgroup)
#pragma unroll
            for (int h = 8; h >= 1; h >>= 1) {                        // exchange across lane bit 4 h: 32, 16, 8, 4
                const bool up = (lane & (4 * h)) != 0;
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                    if (j < h) {
                        const float send = up ? t[j] : t[j + h];
                        const float keep = up ? t[j + h] : t[j];
                        t[j] = keep + __shfl_xor(send, 4 * h, 64);
                    }
                }
            }
            t[0] += __shfl_xor(t[0], 2, 64);
            t[0] += __shfl_xor(t[0], 1, 64);
            const int k = lane >> 2;                                  // slot 0 holds column (lane >> 2) & 15
            if ((lane & 3) == 0 && k < qdim) dr[row * qdim + k] = t[0];
        }
    }
    __syncthreads();                                                  // every wave is done with W in LDS
    const int nW = C * qdim;
    for (int w = 0; w < 4; ++w) {
        if (wave == w) {
#pragma unroll
            for (int i = 0; i < NI; ++i) {
                const int c = lane + 64 * i;
                if (c < C) {
#pragma unroll
                    for (int k = 0; k < EMB_MAXQ; ++k)
                        if (k < qdim) smem[c * qdim + k] = w == 0 ? accW[i][k] : smem[c * qdim + k] + accW[i][k];
                    smem[nW + c] = w == 0 ? accB[i] : smem[nW + c] + accB[i];
                }
            }
        }
        __syncthreads();
    }
    float* slot = part + (size_t)blockIdx.x * (size_t)(nW + C);
    for (int i = threadIdx.x; i < nW + C; i += WG) slot[i] = smem[i];
}

// result[i] = the slots' element i in ascending slot order, in double, rounded once; i < nW goes to dW, the rest to db
__global__ __launch_bounds__(WG) void embed_final_kernel(const float* __restrict__ part, long long n_slots, int nW, int C, float* __restrict__ dW,
                                                         float* __restrict__ db) {
    const int i = blockIdx.x * WG + threadIdx.x;
    const int n = nW + C;
    if (i >= n) return;
    double s = 0.0;
    for (long long w = 0; w < n_slots; ++w) s += (double)part[(size_t)w * n + i];
    if (i < nW) dW[i] = (float)s;
    else db[i - nW] = (float)s;
}

// ---- c. grouped posterior -----------------------------------------------------------------------------------------------------------------
constexpr long long PG_PER_WG = 4096;            // elements of one group's [L, Dl] per workgroup
constexpr float LV_MIN = -30.0f, LV_MAX = 20.0f;

template <int VW>
__device__ __forceinline__ void ld(const float* p, float (&f)[VW]) {
    if (VW == 4) { const float4 q = *reinterpret_cast<const float4*>(p); f[0] = q.x; f[1 % VW] = q.y; f[2 % VW] = q.z; f[3 % VW] = q.w; }
    else f[0] = *p;
}
template <int VW>
__device__ __forceinline__ void st(float* p, const float (&f)[VW]) {
    if (VW == 4) *reinterpret_cast<float4*>(p) = make_float4(f[0], f[1 % VW], f[2 % VW], f[3 % VW]);
    else *p = f[0];
}

// workgroup b: group b / slots, elements [(b % slots) PG_PER_WG, ...) of the group's n = L Dl; VW = 4: Dl % 4 == 0, a thread's 4 elements share a row
template <int VW>
__global__ __launch_bounds__(WG) void pg_fwd_kernel(const float* __restrict__ mean, long long ldm, const float* __restrict__ logvar, long long ldl,
                                                    const float* __restrict__ eps, float* __restrict__ z, long long n, long long L, int Dl,
                                                    long long slots, double* __restrict__ part) {
    __shared__ double red[WG];
    const long long g = blockIdx.x / slots, sl = blockIdx.x - g * slots;
    const long long e0 = sl * PG_PER_WG, e1 = e0 + PG_PER_WG < n ? e0 + PG_PER_WG : n;
    double acc = 0.0;
    for (long long e = e0 + (long long)threadIdx.x * VW; e < e1; e += WG * VW) {
        const long long row = e / Dl;
        const int c = (int)(e - row * Dl);
        const long long gr = g * L + row;
        float m[VW], lv[VW], ep[VW], o[VW];
        ld<VW>(mean + gr * ldm + c, m);
        ld<VW>(logvar + gr * ldl + c, lv);
        ld<VW>(eps + g * n + e, ep);
#pragma unroll
        for (int q = 0; q < VW; ++q) {
            const float l = fminf(fmaxf(lv[q], LV_MIN), LV_MAX);
            o[q] = m[q] + expf(0.5f * l) * ep[q];
            // squares and exponentials in fp32, the four-term sum of an element and the running sum in double
            acc += (((double)(m[q] * m[q]) + (double)expf(l)) - 1.0) - (double)l;
        }
        st<VW>(z + g * n + e, o);
    }
    acc = gvf_block_sum_tree<WG>(acc, red);
    if (threadIdx.x == 0) part[blockIdx.x] = acc;
}

__global__ __launch_bounds__(WG) void pg_final_kernel(const double* __restrict__ part, long long slots, long long G, double factor, float* __restrict__ kl) {
    const long long g = (long long)blockIdx.x * WG + threadIdx.x;
    if (g >= G) return;
    double s = 0.0;
    for (long long k = 0; k < slots; ++k) s += part[g * slots + k];
    kl[g] = (float)(s * factor);
}

template <int VW>
__global__ __launch_bounds__(WG) void pg_bwd_kernel(const float* __restrict__ mean, long long ldm, const float* __restrict__ logvar, long long ldl,
                                                    const float* __restrict__ eps, const float* __restrict__ dz, const float* __restrict__ dkl,
                                                    float* __restrict__ dmean, long long lddm, float* __restrict__ dlogvar, long long lddl,
                                                    long long total, long long n, long long L, int Dl) {
    const long long t = ((long long)blockIdx.x * WG + threadIdx.x) * VW;
    if (t >= total) return;
    const long long g = t / n, e = t - g * n;
    const long long row = e / Dl;
    const int c = (int)(e - row * Dl);
    const long long gr = g * L + row;
    // the KL part per element as (dkl m) / n and ((0.5 dkl) (exp(lv) - 1)) / n, as gvf_posterior_bwd: a factor dkl / n rounded once would put
    // its rounding error on every element of the group alike
    const float gk = dkl != nullptr ? dkl[g] : 0.0f, hk = 0.5f * gk, nf = (float)n;
    float m[VW], lv[VW], dm[VW], dl[VW];
    ld<VW>(mean + gr * ldm + c, m);
    ld<VW>(logvar + gr * ldl + c, lv);
#pragma unroll
    for (int q = 0; q < VW; ++q) {
        const float l = fminf(fmaxf(lv[q], LV_MIN), LV_MAX);
        dm[q] = (gk * m[q]) / nf;
        dl[q] = (hk * (expf(l) - 1.0f)) / nf;
    }
    if (dz != nullptr) {
        float gz[VW], ep[VW];
        ld<VW>(dz + t, gz);
        ld<VW>(eps + t, ep);
#pragma unroll
        for (int q = 0; q < VW; ++q) {
            const float l = fminf(fmaxf(lv[q], LV_MIN), LV_MAX);
            dm[q] += gz[q];
            dl[q] += gz[q] * (0.5f * expf(0.5f * l) * ep[q]);
        }
    }
#pragma unroll
    for (int q = 0; q < VW; ++q) dl[q] = (lv[q] >= LV_MIN && lv[q] <= LV_MAX) ? dl[q] : 0.0f;      // 1 on the bounds, 0 strictly outside
    st<VW>(dmean + gr * lddm + c, dm);
    st<VW>(dlogvar + gr * lddl + c, dl);
}

constexpr long long MAX_GRID = 0x7fffffffLL;

// rows * (F / 8) vectors, one thread each
inline bool geglu_dims_ok(int64_t rows, int F) { return rows >= 0 && F > 0 && (F & 7) == 0 && rows <= (MAX_GRID * 32) / (F >> 3); }

inline bool embed_dims_ok(int64_t P, int qdim, int C) {
    return P >= 0 && qdim >= 3 && qdim <= EMB_MAXQ && C > 0 && C <= EMB_MAXC && (C % 6) == 0 && P <= MAX_GRID;
}
// rows per workgroup: P / 512 rounded up to a multiple of the four waves, between 4 and EMB_MAX_ROWS -- a function of P alone, so the slots and
// the order of every sum are the same run to run
inline int emb_rows_per_wg(int64_t P) {
    long long r = (gvf_cdiv(P, 512) + 3) / 4 * 4;
    return (int)(r < 4 ? 4 : (r > EMB_MAX_ROWS ? EMB_MAX_ROWS : r));
}
inline size_t embed_lds_bytes(int qdim, int C) { return ((size_t)C * (qdim | 1) + C + C / 6) * sizeof(float); }

// G * L * Dl elements, one thread each on the element-wise path of the backward
inline bool pg_dims_ok(int64_t G, int64_t L, int Dl) {
    return G >= 0 && L > 0 && Dl > 0 && L <= MAX_GRID / Dl && (G == 0 || G <= MAX_GRID / (L * (int64_t)Dl));
}

}  // namespace

extern "C" int gvf_geglu_fwd(int dtype, const void* u, int64_t ldu, void* a, int64_t lda, int64_t rows, int F, void* stream_) {
    if (!gvf_lp_ok(dtype) || !geglu_dims_ok(rows, F)) return GVF_EINVAL;
    if (ldu < 2 * (int64_t)F || lda < F || (ldu & 7) || (lda & 7)) return GVF_EINVAL;
    if (rows == 0) return GVF_OK;
    if (!u || !a || gvf_mis(u, 15) || gvf_mis(a, 15)) return GVF_EINVAL;
    const int f8 = F >> 3;
    const long long total = rows * (long long)f8;
    (void)hipGetLastError();
    GVF_LP_DISPATCH(dtype, hipLaunchKernelGGL(geglu_fwd_kernel<DT>, dim3((unsigned)gvf_cdiv(total, WG)), dim3(WG), 0, (hipStream_t)stream_,
                                              (const unsigned short*)u, (long long)ldu, (unsigned short*)a, (long long)lda, total, f8, F));
    GVF_CHECK_LAUNCH();
    return GVF_OK;
}

extern "C" int gvf_geglu_bwd(int dtype, const void* u, int64_t ldu, const void* da, int64_t ldda, void* du, int64_t lddu, int64_t rows, int F,
                             void* stream_) {
    if (!gvf_lp_ok(dtype) || !geglu_dims_ok(rows, F)) return GVF_EINVAL;
    if (ldu < 2 * (int64_t)F || lddu < 2 * (int64_t)F || ldda < F || (ldu & 7) || (lddu & 7) || (ldda & 7)) return GVF_EINVAL;
    if (rows == 0) return GVF_OK;
    if (!u || !da || !du || gvf_mis(u, 15) || gvf_mis(da, 15) || gvf_mis(du, 15)) return GVF_EINVAL;
    const int f8 = F >> 3;
    const long long total = rows * (long long)f8;
    (void)hipGetLastError();
    GVF_LP_DISPATCH(dtype, hipLaunchKernelGGL(geglu_bwd_kernel<DT>, dim3((unsigned)gvf_cdiv(total, WG)), dim3(WG), 0, (hipStream_t)stream_,
                                              (const unsigned short*)u, (long long)ldu, (const unsigned short*)da, (long long)ldda,
                                              (unsigned short*)du, (long long)lddu, total, f8, F));
    GVF_CHECK_LAUNCH();
    return GVF_OK;
}

extern "C" int gvf_vae_embed_train_fwd(const float* r, int qdim, const float* W, const float* bias, const float* omega, float* e, int64_t P, int C,
                                       float eps, void* stream_) {
    if (!embed_dims_ok(P, qdim, C) || !(eps >= 0.0f)) return GVF_EINVAL;
    if (P == 0) return GVF_OK;
    if (!r || !W || !bias || !omega || !e || gvf_mis(r, 3) || gvf_mis(W, 3) || gvf_mis(bias, 3) || gvf_mis(omega, 3) || gvf_mis(e, 3)) return GVF_EINVAL;
    const size_t smem = embed_lds_bytes(qdim, C);
    const int rpw = emb_rows_per_wg(P);
    const dim3 grid((unsigned)gvf_cdiv(P, rpw));
    hipStream_t stream = (hipStream_t)stream_;
    (void)hipGetLastError();
    if (C <= 192) hipLaunchKernelGGL(embed_fwd_kernel<3>, grid, dim3(WG), smem, stream, r, qdim, W, bias, omega, e, (long long)P, C, eps, rpw);
    else hipLaunchKernelGGL(embed_fwd_kernel<12>, grid, dim3(WG), smem, stream, r, qdim, W, bias, omega, e, (long long)P, C, eps, rpw);
    GVF_CHECK_LAUNCH();
    return GVF_OK;
}

extern "C" int gvf_vae_embed_bwd_workspace_bytes(int64_t P, int qdim, int C, size_t* out) {
    if (!out || !embed_dims_ok(P, qdim, C)) return GVF_EINVAL;
    *out = (size_t)gvf_cdiv(P, emb_rows_per_wg(P)) * (size_t)(C * qdim + C) * sizeof(float);
    return GVF_OK;
}

extern "C" int gvf_vae_embed_bwd(const float* r, int qdim, const float* W, const float* bias, const float* omega, const float* de, float* dW, float* db,
                                 float* dr, int64_t P, int C, float eps, void* workspace, size_t workspace_bytes, void* stream_) {
    if (!embed_dims_ok(P, qdim, C) || !(eps >= 0.0f)) return GVF_EINVAL;
    if (P == 0) return GVF_OK;
    if (!r || !W || !bias || !omega || !de || !dW || !db || !workspace) return GVF_EINVAL;
    if (gvf_mis(r, 3) || gvf_mis(W, 3) || gvf_mis(bias, 3) || gvf_mis(omega, 3) || gvf_mis(de, 3) || gvf_mis(dW, 3) || gvf_mis(db, 3) || gvf_mis(dr, 3) || gvf_mis(workspace, 7))
        return GVF_EINVAL;
    size_t need = 0;
    if (gvf_vae_embed_bwd_workspace_bytes(P, qdim, C, &need) != GVF_OK || workspace_bytes < need) return GVF_EINVAL;
    const size_t smem = embed_lds_bytes(qdim, C);
    const int rpw = emb_rows_per_wg(P);
    const long long slots = gvf_cdiv(P, rpw);
    float* part = (float*)workspace;
    hipStream_t stream = (hipStream_t)stream_;
    (void)hipGetLastError();
    if (C <= 192) hipLaunchKernelGGL(embed_bwd_kernel<3>, dim3((unsigned)slots), dim3(WG), smem, stream, r, qdim, W, bias, omega, de, dr, part, (long long)P, C, eps, rpw);
    else hipLaunchKernelGGL(embed_bwd_kernel<12>, dim3((unsigned)slots), dim3(WG), smem, stream, r, qdim, W, bias, omega, de, dr, part, (long long)P, C, eps, rpw);
    GVF_CHECK_LAUNCH();
    hipLaunchKernelGGL(embed_final_kernel, dim3((unsigned)gvf_cdiv(C * qdim + C, WG)), dim3(WG), 0, stream, (const float*)part, slots, C * qdim, C, dW, db);
    GVF_CHECK_LAUNCH();
    return GVF_OK;
}

extern "C" int gvf_posterior_groups_workspace_bytes(int64_t G, int64_t L, int Dl, size_t* out) {
    if (!out || !pg_dims_ok(G, L, Dl)) return GVF_EINVAL;
    *out = (size_t)G * (size_t)gvf_cdiv(L * (long long)Dl, PG_PER_WG) * sizeof(double);
    return GVF_OK;
}

extern "C" int gvf_posterior_groups_fwd(const float* mean, int64_t ld_mean, const float* logvar, int64_t ld_logvar, const float* eps, float* z, float* kl,
                                        int64_t G, int64_t L, int Dl, void* workspace, size_t workspace_bytes, void* stream_) {
    if (!pg_dims_ok(G, L, Dl) || ld_mean < Dl || ld_logvar < Dl) return GVF_EINVAL;
    if (G == 0) return GVF_OK;
    if (!mean || !logvar || !eps || !z || !kl || !workspace) return GVF_EINVAL;
    if (gvf_mis(mean, 3) || gvf_mis(logvar, 3) || gvf_mis(eps, 3) || gvf_mis(z, 3) || gvf_mis(kl, 3) || gvf_mis(workspace, 7)) return GVF_EINVAL;
    size_t need = 0;
    if (gvf_posterior_groups_workspace_bytes(G, L, Dl, &need) != GVF_OK || workspace_bytes < need) return GVF_EINVAL;
    const long long n = L * (long long)Dl, slots = gvf_cdiv(n, PG_PER_WG);
    if (G * slots > MAX_GRID) return GVF_EINVAL;
    const bool vec = (Dl % 4) == 0 && (ld_mean % 4) == 0 && (ld_logvar % 4) == 0 && !gvf_mis(mean, 15) && !gvf_mis(logvar, 15) && !gvf_mis(eps, 15) && !gvf_mis(z, 15);
    hipStream_t stream = (hipStream_t)stream_;
    double* part = (double*)workspace;
    (void)hipGetLastError();
    if (vec) hipLaunchKernelGGL(pg_fwd_kernel<4>, dim3((unsigned)(G * slots)), dim3(WG), 0, stream, mean, (long long)ld_mean, logvar, (long long)ld_logvar, eps,
                                z, n, (long long)L, Dl, slots, part);
    else hipLaunchKernelGGL(pg_fwd_kernel<1>, dim3((unsigned)(G * slots)), dim3(WG), 0, stream, mean, (long long)ld_mean, logvar, (long long)ld_logvar, eps, z,
                            n, (long long)L, Dl, slots, part);
    GVF_CHECK_LAUNCH();
    hipLaunchKernelGGL(pg_final_kernel, dim3((unsigned)gvf_cdiv(G, WG)), dim3(WG), 0, stream, (const double*)part, slots, (long long)G, 0.5 / (double)n, kl);
    GVF_CHECK_LAUNCH();
    return GVF_OK;
}

extern "C" int gvf_posterior_groups_bwd(const float* mean, int64_t ld_mean, const float* logvar, int64_t ld_logvar, const float* eps, const float* dz,
                                        const float* dkl, float* dmean, int64_t ld_dmean, float* dlogvar, int64_t ld_dlogvar, int64_t G, int64_t L,
                                        int Dl, void* stream_) {
    if (!pg_dims_ok(G, L, Dl) || ld_mean < Dl || ld_logvar < Dl || ld_dmean < Dl || ld_dlogvar < Dl) return GVF_EINVAL;
    if (G == 0) return GVF_OK;
    if (!mean || !logvar || !dmean || !dlogvar || (dz != nullptr && !eps)) return GVF_EINVAL;
    if (gvf_mis(mean, 3) || gvf_mis(logvar, 3) || gvf_mis(eps, 3) || gvf_mis(dz, 3) || gvf_mis(dkl, 3) || gvf_mis(dmean, 3) || gvf_mis(dlogvar, 3)) return GVF_EINVAL;
    const long long n = L * (long long)Dl, total = G * n;
    const bool vec = (Dl % 4) == 0 && (ld_mean % 4) == 0 && (ld_logvar % 4) == 0 && (ld_dmean % 4) == 0 && (ld_dlogvar % 4) == 0 && !gvf_mis(mean, 15) &&
                     !gvf_mis(logvar, 15) && !gvf_mis(eps, 15) && !gvf_mis(dz, 15) && !gvf_mis(dmean, 15) && !gvf_mis(dlogvar, 15);
    hipStream_t stream = (hipStream_t)stream_;
    (void)hipGetLastError();
    if (vec) hipLaunchKernelGGL(pg_bwd_kernel<4>, dim3((unsigned)gvf_cdiv(total / 4, WG)), dim3(WG), 0, stream, mean, (long long)ld_mean, logvar,
                                (long long)ld_logvar, eps, dz, dkl, dmean, (long long)ld_dmean, dlogvar, (long long)ld_dlogvar, total, n, (long long)L, Dl);
    else hipLaunchKernelGGL(pg_bwd_kernel<1>, dim3((unsigned)gvf_cdiv(total, WG)), dim3(WG), 0, stream, mean, (long long)ld_mean, logvar, (long long)ld_logvar,
                            eps, dz, dkl, dmean, (long long)ld_dmean, dlogvar, (long long)ld_dlogvar, total, n, (long long)L, Dl);
    GVF_CHECK_LAUNCH();
    return GVF_OK;
}
