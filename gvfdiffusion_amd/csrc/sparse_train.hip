// sparse_train.hip -- the training kernels of the static VAE that are not matrix products, for gfx950 (include/gvf_sparse_train.h): the
// tanh-GELU between mlp.0 and mlp.2, the row gather of the window partition, the posterior sample with its KL term and the volume / opacity
// regularisers of the Gaussians, each forward and backward, and the fp32 column sums a closing projection's bias gradient is taken from.
//
// Reference: model/sparse_voxel_diffusion/sparse_transformer.py:115-126 (SparseGELU(approximate="tanh")), sparse/attention/windowed_attn.py
// (feats[fwd_indices] ... out[bwd_indices]), sparse_vae.py:351 (kl) and :229-249 (get_regularization_loss).  Under autocast the reference
// runs each as a chain of launches, the gather's gradient as index_put_(accumulate=True) on float atomics; here each is one launch each way.
// fp32 inside, 16-bit only at loads and stores, 16-byte accesses where the addresses allow.  Means over rows: one double-precision partial per
// workgroup in its own workspace slot, added in slot order by sum_slots_kernel: no atomics, same bits every run.
#include <cmath>
#include "gvf_common.h"
#include "gvf_lp.h"
#include "gvf_rowops.h"
#include "../../include/gvf_rast.h"
#include "../../include/gvf_dit.h"
#include "../../include/gvf_sparse_train.h"

namespace {

constexpr int WG = 256;
constexpr long long POST_PER_WG = 4096;           // elements of [T, L] per workgroup (posterior)
constexpr long long REG_PER_WG = 1024;            // Gaussians per workgroup (regularisers: 4 per thread)
constexpr int MAX_SCALARS = 2;

// ---- a. tanh-GELU -------------------------------------------------------------------------------------------------------------------------
constexpr float GELU_K = 0.7978845608028654f, GELU_C = 0.044715f;

// 0.5 (1 + tanh(y)) = sigmoid(2 y) = 1 / (1 + exp(-2 y)): the same function without tanh's subtraction of two numbers near 1 for negative
// y (relative accuracy over the whole range) and on the hardware exponential (its error, 1e-6 relative at |2 y| = 20, is 0.5 % of an fp16
// rounding).  exp(-2 y) = inf for a very negative y gives a = u / inf = -0, and = 0 for a very positive one gives a = u: finite everywhere.
__device__ __forceinline__ float gelu_fwd(float u) {
    const float in = GELU_K * (u + GELU_C * (u * u * u));                // u^3 = inf for a huge bf16 u: exp(-+inf) = 0 or inf
    return u / (1.0f + __expf(-2.0f * in));
}
__device__ __forceinline__ float gelu_bwd(float u, float da) {
    const float in = GELU_K * (u + GELU_C * (u * u * u));
    const float e = __expf(-2.0f * in);
    const float sg = 1.0f / (1.0f + e);                                   // 0.5 (1 + t)
    // 0.5 u (1 - t^2) in' = u sg (1 - sg) 2 in', 1 - sg = e / (1 + e).  From |in| = 10 on the term is below 2^-25 of the first one (or both
    // are below 1e-7): dropping it there changes nothing that is stored and keeps inf / inf and 0 * inf out for |u| near the largest
    // finite value
    const float sech = fabsf(in) < 10.0f ? (u * sg) * (e * sg) * (2.0f * GELU_K * (1.0f + 3.0f * GELU_C * (u * u))) : 0.0f;
    return da * (sg + sech);
}

// nv vectors of 8 elements, then the elements [8 nv, n) one by one (thread i of the grid takes tail element i)
template <int DT, bool BWD>
__global__ __launch_bounds__(WG) void gelu_kernel(const unsigned short* __restrict__ u, const unsigned short* __restrict__ da,
                                                  unsigned short* __restrict__ out, long long nv, long long n) {
    const long long i = (long long)blockIdx.x * WG + threadIdx.x;
    if (i < nv) {
        float f[8], g[8], o[8];
        gvf_unpack8<DT>(reinterpret_cast<const uint4*>(u)[i], f);
        if (BWD) gvf_unpack8<DT>(reinterpret_cast<const uint4*>(da)[i], g);
#pragma unroll
        for (int e = 0; e < 8; ++e) o[e] = BWD ? gelu_bwd(f[e], g[e]) : gelu_fwd(f[e]);
        reinterpret_cast<uint4*>(out)[i] = gvf_pack8<DT>(o);
    }
    const long long t = nv * 8 + i;
    if (t < n) {
        const float f = GvfLp<DT>::from16(u[t]);
        out[t] = GvfLp<DT>::to16(BWD ? gelu_bwd(f, GvfLp<DT>::from16(da[t])) : gelu_fwd(f));
    }
}

// ---- b. row gather ------------------------------------------------------------------------------------------------------------------------
// one 16-byte chunk per thread: chunk c of row i, cpr chunks a row
__global__ __launch_bounds__(WG) void gather_rows_kernel(const unsigned char* __restrict__ src, long long src_stride, const long long* __restrict__ index,
                                                         uint4* __restrict__ out, long long rows, long long cpr) {
    const long long t = (long long)blockIdx.x * WG + threadIdx.x;
    if (t >= rows * cpr) return;
    const long long i = t / cpr, c = t - i * cpr;
    out[t] = *reinterpret_cast<const uint4*>(src + index[i] * src_stride + c * 16);
}

// ---- sums: a workgroup's 256 double terms -> one slot (gvf_block_sum_tree); the slots -> the scalar ---------------------------------------
// out[o] = factor[o] * (slots of scalar o in ascending order): thread k adds slots k, k + 256, ..., then the fixed tree.  blockIdx.x = o.
struct SumJobs { float* out[MAX_SCALARS]; double factor[MAX_SCALARS]; };
__global__ __launch_bounds__(WG) void sum_slots_kernel(const double* __restrict__ part, long long n_slots, SumJobs jobs) {
    __shared__ double red[WG];
    const int o = blockIdx.x;
    if (jobs.out[o] == nullptr) return;
    double s = 0.0;
    for (long long w = threadIdx.x; w < n_slots; w += WG) s += part[(size_t)o * n_slots + w];
    s = gvf_block_sum_tree<WG>(s, red);
    if (threadIdx.x == 0) *jobs.out[o] = (float)(s * jobs.factor[o]);
}

// ---- c. posterior -------------------------------------------------------------------------------------------------------------------------
// element e of [T, L]: row e / L, column e % L.  VEC: L % 4 == 0, a thread takes 4 consecutive columns of one row.
template <bool VEC>
__global__ __launch_bounds__(WG) void posterior_fwd_kernel(const float* __restrict__ h, long long ldh, const float* __restrict__ eps, float* __restrict__ z,
                                                           long long total, int L, double* __restrict__ part) {
    __shared__ double red[WG];
    const long long e0 = (long long)blockIdx.x * POST_PER_WG;
    const long long e1 = e0 + POST_PER_WG < total ? e0 + POST_PER_WG : total;
    double acc = 0.0;
    if (VEC) {
        for (long long e = e0 + (long long)threadIdx.x * 4; e < e1; e += WG * 4) {
            const long long row = e / L;
            const int c = (int)(e - row * L);
            const float4 m = *reinterpret_cast<const float4*>(h + row * ldh + c);
            const float4 lv = *reinterpret_cast<const float4*>(h + row * ldh + L + c);
            const float4 n = *reinterpret_cast<const float4*>(eps + e);
            float4 o;
            o.x = m.x + expf(0.5f * lv.x) * n.x; o.y = m.y + expf(0.5f * lv.y) * n.y;
            o.z = m.z + expf(0.5f * lv.z) * n.z; o.w = m.w + expf(0.5f * lv.w) * n.w;
            *reinterpret_cast<float4*>(z + e) = o;
            // squares and exponentials in fp32, the four-term sum of an element and the running sum in double
            acc += (((double)(m.x * m.x) + (double)expf(lv.x)) - (double)lv.x) - 1.0;
            acc += (((double)(m.y * m.y) + (double)expf(lv.y)) - (double)lv.y) - 1.0;
            acc += (((double)(m.z * m.z) + (double)expf(lv.z)) - (double)lv.z) - 1.0;
            acc += (((double)(m.w * m.w) + (double)expf(lv.w)) - (double)lv.w) - 1.0;
        }
    } else {
        for (long long e = e0 + threadIdx.x; e < e1; e += WG) {
            const long long row = e / L;
            const int c = (int)(e - row * L);
            const float m = h[row * ldh + c], lv = h[row * ldh + L + c];
            z[e] = m + expf(0.5f * lv) * eps[e];
            acc += (((double)(m * m) + (double)expf(lv)) - (double)lv) - 1.0;
        }
    }
    acc = gvf_block_sum_tree<WG>(acc, red);
    if (threadIdx.x == 0) part[blockIdx.x] = acc;
}

template <bool VEC>
__global__ __launch_bounds__(WG) void posterior_bwd_kernel(const float* __restrict__ h, long long ldh, const float* __restrict__ eps, const float* __restrict__ dz,
                                                           const float* __restrict__ dkl, float* __restrict__ dh, long long lddh, long long total, int L) {
    // the KL part per element as (dkl m) / n and ((0.5 dkl) (exp(lv) - 1)) / n: a factor dkl / n rounded once would put ITS rounding error
    // on every element alike (a relative L2 of up to 2^-24 on the whole tensor instead of independent half-ulps)
    const float gk = dkl != nullptr ? *dkl : 0.0f, hk = 0.5f * gk, n_el = (float)total;
    const long long e = ((long long)blockIdx.x * WG + threadIdx.x) * (VEC ? 4 : 1);
    if (e >= total) return;
    const long long row = e / L;
    const int c = (int)(e - row * L);
    if (VEC) {
        const float4 m = *reinterpret_cast<const float4*>(h + row * ldh + c);
        const float4 lv = *reinterpret_cast<const float4*>(h + row * ldh + L + c);
        float4 dm = make_float4((gk * m.x) / n_el, (gk * m.y) / n_el, (gk * m.z) / n_el, (gk * m.w) / n_el);
        float4 dl = make_float4((hk * (expf(lv.x) - 1.0f)) / n_el, (hk * (expf(lv.y) - 1.0f)) / n_el, (hk * (expf(lv.z) - 1.0f)) / n_el,
                                (hk * (expf(lv.w) - 1.0f)) / n_el);
        if (dz != nullptr) {
            const float4 g = *reinterpret_cast<const float4*>(dz + e);
            const float4 n = *reinterpret_cast<const float4*>(eps + e);
            dm.x += g.x; dm.y += g.y; dm.z += g.z; dm.w += g.w;
            dl.x += g.x * (0.5f * expf(0.5f * lv.x) * n.x); dl.y += g.y * (0.5f * expf(0.5f * lv.y) * n.y);
            dl.z += g.z * (0.5f * expf(0.5f * lv.z) * n.z); dl.w += g.w * (0.5f * expf(0.5f * lv.w) * n.w);
        }
        *reinterpret_cast<float4*>(dh + row * lddh + c) = dm;
        *reinterpret_cast<float4*>(dh + row * lddh + L + c) = dl;
    } else {
        const float m = h[row * ldh + c], lv = h[row * ldh + L + c];
        float dm = (gk * m) / n_el, dl = (hk * (expf(lv) - 1.0f)) / n_el;
        if (dz != nullptr) {
            dm += dz[e];
            dl += dz[e] * (0.5f * expf(0.5f * lv) * eps[e]);
        }
        dh[row * lddh + c] = dm;
        dh[row * lddh + L + c] = dl;
    }
}

// ---- d. regularisers ----------------------------------------------------------------------------------------------------------------------
struct RegConst { float bs, bo, k2; int softplus; };

__device__ __forceinline__ float reg_act(float x, int softplus) { return softplus ? (x > 20.0f ? x : log1pf(expf(x))) : expf(x); }
// d act / d x: exp -> the activation itself; softplus -> sigmoid, 1 on the linear branch
__device__ __forceinline__ float reg_dact(float x, float a, int softplus) { return softplus ? (x > 20.0f ? 1.0f : 1.0f / (1.0f + expf(-x))) : a; }
__device__ __forceinline__ float reg_sigmoid(float x) { return 1.0f / (1.0f + expf(-x)); }
// 1 - sigmoid(x) = e / (1 + e), e = exp(-x): no subtraction of two numbers near 1 (an opacity near 1 is where this regulariser ends up)
__device__ __forceinline__ float reg_one_minus_sigmoid(float x) { const float e = expf(-x); return e > 1e30f ? 1.0f : e / (1.0f + e); }

__device__ __forceinline__ void reg_fwd_one(const float (&s)[3], float o, const RegConst& K, double& vol, double& opa) {
    float q[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) { const float a = reg_act(s[k] + K.bs, K.softplus); q[k] = sqrtf(a * a + K.k2); }
    vol += (double)((q[0] * q[1]) * q[2]);
    const float d = reg_one_minus_sigmoid(o + K.bo);
    opa += (double)(d * d);
}
__device__ __forceinline__ void reg_bwd_one(const float (&s)[3], float o, const RegConst& K, float gv, float go, float (&ds)[3], float& d_o) {
    float q[3], r[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const float x = s[k] + K.bs;
        const float a = reg_act(x, K.softplus);
        q[k] = sqrtf(a * a + K.k2);
        r[k] = (q[k] > 0.0f ? a / q[k] : 0.0f) * reg_dact(x, a, K.softplus);
    }
    ds[0] = gv * ((q[1] * q[2]) * r[0]);
    ds[1] = gv * ((q[0] * q[2]) * r[1]);
    ds[2] = gv * ((q[0] * q[1]) * r[2]);
    const float sg = reg_sigmoid(o + K.bo), om = reg_one_minus_sigmoid(o + K.bo);
    d_o = go * ((-2.0f * om) * (sg * om));
}

// a thread takes Gaussians 4 j .. 4 j + 3 (VEC: three float4 of scaling, one of opacity), the last thread of the data the N % 4 left over
template <bool VEC>
__global__ __launch_bounds__(WG) void reg_fwd_kernel(const float* __restrict__ sc, const float* __restrict__ op, long long N, RegConst K,
                                                     double* __restrict__ part, long long n_slots) {
    __shared__ double red[WG];
    const long long i0 = ((long long)blockIdx.x * WG + threadIdx.x) * 4;
    double vol = 0.0, opa = 0.0;
    if (VEC && i0 + 4 <= N) {
        const float4 a = *reinterpret_cast<const float4*>(sc + i0 * 3), b = *reinterpret_cast<const float4*>(sc + i0 * 3 + 4),
                     c = *reinterpret_cast<const float4*>(sc + i0 * 3 + 8), o = *reinterpret_cast<const float4*>(op + i0);
        const float s0[3] = {a.x, a.y, a.z}, s1[3] = {a.w, b.x, b.y}, s2[3] = {b.z, b.w, c.x}, s3[3] = {c.y, c.z, c.w};
        reg_fwd_one(s0, o.x, K, vol, opa); reg_fwd_one(s1, o.y, K, vol, opa); reg_fwd_one(s2, o.z, K, vol, opa); reg_fwd_one(s3, o.w, K, vol, opa);
    } else {
        for (long long i = i0; i < i0 + 4 && i < N; ++i) {
            const float s[3] = {sc[i * 3], sc[i * 3 + 1], sc[i * 3 + 2]};
            reg_fwd_one(s, op[i], K, vol, opa);
        }
    }
    vol = gvf_block_sum_tree<WG>(vol, red);
    opa = gvf_block_sum_tree<WG>(opa, red);
    if (threadIdx.x == 0) { part[blockIdx.x] = vol; part[n_slots + blockIdx.x] = opa; }
}

template <bool VEC>
__global__ __launch_bounds__(WG) void reg_bwd_kernel(const float* __restrict__ sc, const float* __restrict__ op, long long N, RegConst K,
                                                     const float* __restrict__ dvol, const float* __restrict__ dopa, float* __restrict__ dsc,
                                                     float* __restrict__ dop) {
    const float gv = dvol != nullptr ? *dvol / (float)N : 0.0f, go = dopa != nullptr ? *dopa / (float)N : 0.0f;
    const long long i0 = ((long long)blockIdx.x * WG + threadIdx.x) * 4;
    if (i0 >= N) return;
    if (VEC && i0 + 4 <= N) {
        const float4 a = *reinterpret_cast<const float4*>(sc + i0 * 3), b = *reinterpret_cast<const float4*>(sc + i0 * 3 + 4),
                     c = *reinterpret_cast<const float4*>(sc + i0 * 3 + 8), o = *reinterpret_cast<const float4*>(op + i0);
        const float s0[3] = {a.x, a.y, a.z}, s1[3] = {a.w, b.x, b.y}, s2[3] = {b.z, b.w, c.x}, s3[3] = {c.y, c.z, c.w};
        float d0[3], d1[3], d2[3], d3[3];
        float4 g;
        reg_bwd_one(s0, o.x, K, gv, go, d0, g.x); reg_bwd_one(s1, o.y, K, gv, go, d1, g.y);
        reg_bwd_one(s2, o.z, K, gv, go, d2, g.z); reg_bwd_one(s3, o.w, K, gv, go, d3, g.w);
        if (dsc != nullptr) {
            *reinterpret_cast<float4*>(dsc + i0 * 3) = make_float4(d0[0], d0[1], d0[2], d1[0]);
            *reinterpret_cast<float4*>(dsc + i0 * 3 + 4) = make_float4(d1[1], d1[2], d2[0], d2[1]);
            *reinterpret_cast<float4*>(dsc + i0 * 3 + 8) = make_float4(d2[2], d3[0], d3[1], d3[2]);
        }
        if (dop != nullptr) *reinterpret_cast<float4*>(dop + i0) = g;
    } else {
        for (long long i = i0; i < i0 + 4 && i < N; ++i) {
            const float s[3] = {sc[i * 3], sc[i * 3 + 1], sc[i * 3 + 2]};
            float d[3], g;
            reg_bwd_one(s, op[i], K, gv, go, d, g);
            if (dsc != nullptr) { dsc[i * 3] = d[0]; dsc[i * 3 + 1] = d[1]; dsc[i * 3 + 2] = d[2]; }
            if (dop != nullptr) dop[i] = g;
        }
    }
}

// ---- e. column sums of fp32 rows (the bias gradient of a projection that closes a sub-layer, from the UNROUNDED stream gradient) -----------
// a thread owns one column of COLSUM_ROWS rows (neighbouring threads, neighbouring columns: coalesced), double accumulation, one slot per
// (row chunk, column); the finaliser adds a column's slots in chunk order
constexpr long long COLSUM_ROWS = 64;
__global__ __launch_bounds__(WG) void colsum_part_kernel(const float* __restrict__ x, long long rows, int C, double* __restrict__ part) {
    const int c = blockIdx.x * WG + threadIdx.x;
    if (c >= C) return;
    const long long r0 = (long long)blockIdx.y * COLSUM_ROWS, r1 = r0 + COLSUM_ROWS < rows ? r0 + COLSUM_ROWS : rows;
    double s = 0.0;
    for (long long r = r0; r < r1; ++r) s += (double)x[r * C + c];
    part[(size_t)blockIdx.y * C + c] = s;
}
__global__ __launch_bounds__(WG) void colsum_final_kernel(const double* __restrict__ part, long long chunks, int C, float* __restrict__ out) {
    const int c = blockIdx.x * WG + threadIdx.x;
    if (c >= C) return;
    double s = 0.0;
    for (long long k = 0; k < chunks; ++k) s += part[(size_t)k * C + c];
    out[c] = (float)s;
}

constexpr long long MAX_GRID = 0x7fffffffLL;

template <bool BWD>
int launch_gelu(int dtype, const void* u, const void* da, void* out, int64_t n, void* stream_) {
    if (!gvf_lp_ok(dtype) || n < 0) return GVF_EINVAL;
    if (n == 0) return GVF_OK;
    if (!u || !out || (BWD && !da)) return GVF_EINVAL;
    if (gvf_mis(u, 1) || gvf_mis(out, 1) || gvf_mis(da, 1)) return GVF_EINVAL;
    const bool vec = !gvf_mis(u, 15) && !gvf_mis(out, 15) && !gvf_mis(da, 15);
    const long long nv = vec ? n / 8 : 0, tail = n - nv * 8;
    const long long blocks = gvf_cdiv(nv > tail ? nv : tail, WG);
    if (blocks > MAX_GRID) return GVF_EINVAL;
    hipStream_t stream = (hipStream_t)stream_;
    (void)hipGetLastError();
    GVF_LP_DISPATCH(dtype, hipLaunchKernelGGL((gelu_kernel<DT, BWD>), dim3((unsigned)blocks), dim3(WG), 0, stream, (const unsigned short*)u,
                                              (const unsigned short*)da, (unsigned short*)out, nv, (long long)n));
    GVF_CHECK_LAUNCH();
    return GVF_OK;
}

int launch_sum(const double* part, long long n_slots, const SumJobs& jobs, int n_jobs, hipStream_t stream) {
    hipLaunchKernelGGL(sum_slots_kernel, dim3(n_jobs), dim3(WG), 0, stream, part, n_slots, jobs);
    GVF_CHECK_LAUNCH();
    return GVF_OK;
}

}  // namespace

extern "C" int gvf_gelu_tanh_fwd(int dtype, const void* u, void* a, int64_t n, void* stream) { return launch_gelu<false>(dtype, u, nullptr, a, n, stream); }

extern "C" int gvf_gelu_tanh_bwd(int dtype, const void* u, const void* da, void* du, int64_t n, void* stream) {
    return launch_gelu<true>(dtype, u, da, du, n, stream);
}

extern "C" int gvf_gather_rows(const void* src, int64_t src_stride_bytes, const int64_t* index, void* out, int64_t rows, int64_t width_bytes,
                               void* stream_) {
    if (rows < 0 || width_bytes <= 0 || (width_bytes % 16) != 0) return GVF_EINVAL;
    if (src_stride_bytes < width_bytes || (src_stride_bytes % 16) != 0) return GVF_EINVAL;
    if (rows == 0) return GVF_OK;
    if (!src || !index || !out || gvf_mis(src, 15) || gvf_mis(out, 15) || gvf_mis(index, 7)) return GVF_EINVAL;
    const long long cpr = width_bytes / 16;
    if (rows > (MAX_GRID * WG) / cpr) return GVF_EINVAL;
    hipStream_t stream = (hipStream_t)stream_;
    (void)hipGetLastError();
    hipLaunchKernelGGL(gather_rows_kernel, dim3((unsigned)gvf_cdiv(rows * cpr, WG)), dim3(WG), 0, stream, (const unsigned char*)src,
                       (long long)src_stride_bytes, (const long long*)index, (uint4*)out, (long long)rows, cpr);
    GVF_CHECK_LAUNCH();
    return GVF_OK;
}

// T * L elements, one thread each on the scalar path of the backward: at most 2^31 - 1 of them
static int posterior_dims_ok(int64_t T, int L) { return T >= 0 && L > 0 && T <= MAX_GRID / L; }

extern "C" int gvf_posterior_workspace_bytes(int64_t T, int L, size_t* out) {
    if (!out || !posterior_dims_ok(T, L)) return GVF_EINVAL;
    *out = (size_t)gvf_cdiv(T * (long long)L, POST_PER_WG) * sizeof(double);
    return GVF_OK;
}

extern "C" int gvf_posterior_fwd(const float* h, int64_t ldh, const float* eps, float* z, float* kl, int64_t T, int L, void* workspace,
                                 size_t workspace_bytes, void* stream_) {
    if (!posterior_dims_ok(T, L) || T == 0) return GVF_EINVAL;
    if (!h || !eps || !z || !kl || !workspace) return GVF_EINVAL;
    if (ldh < 2 * (int64_t)L || gvf_mis(h, 3) || gvf_mis(eps, 3) || gvf_mis(z, 3) || gvf_mis(kl, 3) || gvf_mis(workspace, 7)) return GVF_EINVAL;
    size_t need = 0;
    if (gvf_posterior_workspace_bytes(T, L, &need) != GVF_OK || workspace_bytes < need) return GVF_EINVAL;
    const long long total = T * (long long)L, slots = gvf_cdiv(total, POST_PER_WG);
    const bool vec = (L % 4) == 0 && (ldh % 4) == 0 && !gvf_mis(h, 15) && !gvf_mis(eps, 15) && !gvf_mis(z, 15);
    hipStream_t stream = (hipStream_t)stream_;
    (void)hipGetLastError();
    double* part = (double*)workspace;
    if (vec) hipLaunchKernelGGL(posterior_fwd_kernel<true>, dim3((unsigned)slots), dim3(WG), 0, stream, h, (long long)ldh, eps, z, total, L, part);
    else hipLaunchKernelGGL(posterior_fwd_kernel<false>, dim3((unsigned)slots), dim3(WG), 0, stream, h, (long long)ldh, eps, z, total, L, part);
    GVF_CHECK_LAUNCH();
    SumJobs jobs = {};
    jobs.out[0] = kl;
    jobs.factor[0] = 0.5 / (double)total;
    return launch_sum(part, slots, jobs, 1, stream);
}

extern "C" int gvf_posterior_bwd(const float* h, int64_t ldh, const float* eps, const float* dz, const float* dkl, float* dh, int64_t lddh, int64_t T,
                                 int L, void* stream_) {
    if (!posterior_dims_ok(T, L)) return GVF_EINVAL;
    if (T == 0) return GVF_OK;
    if (!h || !dh || (dz != nullptr && !eps)) return GVF_EINVAL;
    if (ldh < 2 * (int64_t)L || lddh < 2 * (int64_t)L || gvf_mis(h, 3) || gvf_mis(eps, 3) || gvf_mis(dz, 3) || gvf_mis(dkl, 3) || gvf_mis(dh, 3)) return GVF_EINVAL;
    const long long total = T * (long long)L;
    const bool vec = (L % 4) == 0 && (ldh % 4) == 0 && (lddh % 4) == 0 && !gvf_mis(h, 15) && !gvf_mis(eps, 15) && !gvf_mis(dz, 15) && !gvf_mis(dh, 15);
    hipStream_t stream = (hipStream_t)stream_;
    (void)hipGetLastError();
    if (vec) hipLaunchKernelGGL(posterior_bwd_kernel<true>, dim3((unsigned)gvf_cdiv(total / 4, WG)), dim3(WG), 0, stream, h, (long long)ldh, eps, dz, dkl, dh,
                                (long long)lddh, total, L);
    else hipLaunchKernelGGL(posterior_bwd_kernel<false>, dim3((unsigned)gvf_cdiv(total, WG)), dim3(WG), 0, stream, h, (long long)ldh, eps, dz, dkl, dh,
                            (long long)lddh, total, L);
    GVF_CHECK_LAUNCH();
    return GVF_OK;
}

static int reg_args_ok(int64_t N, float min_kernel_size, int activation) {
    return N >= 0 && N <= MAX_GRID && (activation == 0 || activation == 1) && min_kernel_size >= 0.0f;
}

extern "C" int gvf_gaussian_reg_workspace_bytes(int64_t N, size_t* out) {
    if (!out || N < 0 || N > MAX_GRID) return GVF_EINVAL;
    *out = (size_t)MAX_SCALARS * (size_t)gvf_cdiv(N, REG_PER_WG) * sizeof(double);
    return GVF_OK;
}

extern "C" int gvf_gaussian_reg_fwd(const float* scaling, const float* opacity, int64_t N, float scale_bias, float opacity_bias, float min_kernel_size,
                                    int activation, float* vol, float* opa, void* workspace, size_t workspace_bytes, void* stream_) {
    if (!reg_args_ok(N, min_kernel_size, activation) || N == 0) return GVF_EINVAL;
    if (!scaling || !opacity || !vol || !opa || !workspace) return GVF_EINVAL;
    if (gvf_mis(scaling, 3) || gvf_mis(opacity, 3) || gvf_mis(vol, 3) || gvf_mis(opa, 3) || gvf_mis(workspace, 7)) return GVF_EINVAL;
    size_t need = 0;
    if (gvf_gaussian_reg_workspace_bytes(N, &need) != GVF_OK || workspace_bytes < need) return GVF_EINVAL;
    const long long slots = gvf_cdiv(N, REG_PER_WG);
    const bool vec = !gvf_mis(scaling, 15) && !gvf_mis(opacity, 15);
    const RegConst K = {scale_bias, opacity_bias, min_kernel_size * min_kernel_size, activation};
    hipStream_t stream = (hipStream_t)stream_;
    (void)hipGetLastError();
    double* part = (double*)workspace;
    if (vec) hipLaunchKernelGGL(reg_fwd_kernel<true>, dim3((unsigned)slots), dim3(WG), 0, stream, scaling, opacity, (long long)N, K, part, slots);
    else hipLaunchKernelGGL(reg_fwd_kernel<false>, dim3((unsigned)slots), dim3(WG), 0, stream, scaling, opacity, (long long)N, K, part, slots);
    GVF_CHECK_LAUNCH();
    SumJobs jobs = {};
    jobs.out[0] = vol; jobs.out[1] = opa;
    jobs.factor[0] = jobs.factor[1] = 1.0 / (double)N;
    return launch_sum(part, slots, jobs, 2, stream);
}

extern "C" int gvf_gaussian_reg_bwd(const float* scaling, const float* opacity, int64_t N, float scale_bias, float opacity_bias, float min_kernel_size,
                                    int activation, const float* dvol, const float* dopa, float* dscaling, float* dopacity, void* stream_) {
    if (!reg_args_ok(N, min_kernel_size, activation)) return GVF_EINVAL;
    if (N == 0) return GVF_OK;
    if (!scaling || !opacity) return GVF_EINVAL;
    if ((dvol != nullptr && !dscaling) || (dopa != nullptr && !dopacity) || (!dscaling && !dopacity)) return GVF_EINVAL;
    if (gvf_mis(scaling, 3) || gvf_mis(opacity, 3) || gvf_mis(dvol, 3) || gvf_mis(dopa, 3) || gvf_mis(dscaling, 3) || gvf_mis(dopacity, 3)) return GVF_EINVAL;
    const bool vec = !gvf_mis(scaling, 15) && !gvf_mis(opacity, 15) && !gvf_mis(dscaling, 15) && !gvf_mis(dopacity, 15);
    const RegConst K = {scale_bias, opacity_bias, min_kernel_size * min_kernel_size, activation};
    hipStream_t stream = (hipStream_t)stream_;
    (void)hipGetLastError();
    const dim3 grid((unsigned)gvf_cdiv(N, REG_PER_WG));
    if (vec) hipLaunchKernelGGL(reg_bwd_kernel<true>, grid, dim3(WG), 0, stream, scaling, opacity, (long long)N, K, dvol, dopa, dscaling, dopacity);
    else hipLaunchKernelGGL(reg_bwd_kernel<false>, grid, dim3(WG), 0, stream, scaling, opacity, (long long)N, K, dvol, dopa, dscaling, dopacity);
    GVF_CHECK_LAUNCH();
    return GVF_OK;
}

extern "C" int gvf_colsum_f32_workspace_bytes(int64_t rows, int C, size_t* out) {
    if (!out || rows < 0 || C <= 0 || rows > 65535 * COLSUM_ROWS) return GVF_EINVAL;
    *out = (size_t)gvf_cdiv(rows, COLSUM_ROWS) * (size_t)C * sizeof(double);
    return GVF_OK;
}

extern "C" int gvf_colsum_f32(const float* x, int64_t rows, int C, float* out, void* workspace, size_t workspace_bytes, void* stream_) {
    size_t need = 0;
    if (gvf_colsum_f32_workspace_bytes(rows, C, &need) != GVF_OK || rows == 0) return GVF_EINVAL;
    if (!x || !out || !workspace || workspace_bytes < need || gvf_mis(x, 3) || gvf_mis(out, 3) || gvf_mis(workspace, 7)) return GVF_EINVAL;
    const long long chunks = gvf_cdiv(rows, COLSUM_ROWS);
    hipStream_t stream = (hipStream_t)stream_;
    (void)hipGetLastError();
    const unsigned gx = (unsigned)gvf_cdiv(C, WG);
    hipLaunchKernelGGL(colsum_part_kernel, dim3(gx, (unsigned)chunks), dim3(WG), 0, stream, x, (long long)rows, C, (double*)workspace);
    GVF_CHECK_LAUNCH();
    hipLaunchKernelGGL(colsum_final_kernel, dim3(gx), dim3(WG), 0, stream, (const double*)workspace, chunks, C, out);
    GVF_CHECK_LAUNCH();
    return GVF_OK;
}
