// optim.hip -- fused gradient norm / clip + AdamW + EMA optimizer step, gfx950.  C ABI, formulas and operation order: include/gvf_optim.h.
//
// Memory-bound streaming over a chunk table: one 256-thread workgroup per chunk (grid-stride), lane t of the workgroup owns the
// 4-element groups t, t + 256, ... of the chunk, so a chunk of CHUNK = 8192 elements is 8 x 16 bytes per lane and stream.
//   norm:     4 B per element read; gu^2 in double per lane -> fixed shuffle tree -> one double per chunk (its own slot).
//   finalize: one workgroup sums the slots (lane t of 1024: slots t, t + 1024, ... in index order, then the same tree) and writes the step record.
//             A launch of its own rather than "the last workgroup to arrive": the kernel boundary is the only cross-XCD hand-off here.
//   update:   36 B per element (p, g, m, v, e read; p, m, v, e written; 12 B more per further EMA).
// float4 is used for loads and stores only; the arithmetic is per component (no packed fp32: _build.py).  Built with -ffp-contract=off:
// every operation below rounds once, which is what the conformance bars of tests/test_optim_gpu.py count.
#include "gvf_common.h"
#include "gvf_rowops.h"
#include "../../include/gvf_rast.h"
#include "../../include/gvf_optim.h"

#include <math.h>

namespace {

constexpr int NT = 256;            // threads per workgroup
constexpr int NT_FIN = 1024;       // threads of the finalize workgroup
constexpr int CHUNK = 8192;        // elements per chunk
constexpr int MAX_GRID = 1 << 20;  // workgroups per launch (grid-stride beyond)
static_assert(CHUNK % 4 == 0 && CHUNK % (4 * NT) == 0, "chunk length");
static_assert(sizeof(gvf_optim_tensor) == 72 && sizeof(gvf_optim_chunk) == 16 && sizeof(gvf_optim_record) == 128, "table layout");

// The data pointers come out of a table in memory, so the compiler cannot see that they are global: without the address-space casts
// below every access would be a flat_ instruction (both counters, the aperture check) instead of a global_ one.
typedef float vf4 __attribute__((ext_vector_type(4)));
typedef __attribute__((address_space(1))) float gf32;
typedef __attribute__((address_space(1))) vf4 gvf4;

__device__ __forceinline__ float ld(const float* a) { return *(const gf32*)a; }
__device__ __forceinline__ void st(float* a, float x) { *(gf32*)a = x; }

template <bool VEC>
__device__ __forceinline__ void load4(const float* a, float (&x)[4]) {
    if (VEC) {
        const vf4 t = *(const gvf4*)a;
        x[0] = t.x; x[1] = t.y; x[2] = t.z; x[3] = t.w;
    } else {
        x[0] = ld(a); x[1] = ld(a + 1); x[2] = ld(a + 2); x[3] = ld(a + 3);
    }
}

template <bool VEC>
__device__ __forceinline__ void store4(float* a, const float (&x)[4]) {
    if (VEC) {
        vf4 t;
        t.x = x[0]; t.y = x[1]; t.z = x[2]; t.w = x[3];
        *(gvf4*)a = t;
    } else {
        st(a, x[0]); st(a + 1, x[1]); st(a + 2, x[2]); st(a + 3, x[3]);
    }
}

__device__ __forceinline__ bool aligned16(const void* p) { return ((uintptr_t)p & 15u) == 0; }

// ---------------------------------------------------------------------------------------------------------------- norm

template <bool VEC>
__device__ __forceinline__ double chunk_sumsq(const float* __restrict__ g, int count, float inv) {
    const int n4 = count >> 2;
    double acc = 0.0;
#pragma unroll 4
    for (int i = threadIdx.x; i < n4; i += NT) {
        float x[4];
        load4<VEC>(g + 4 * (int64_t)i, x);
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            const float gu = x[c] * inv;
            acc += (double)gu * (double)gu;
        }
    }
    const int i = 4 * n4 + (int)threadIdx.x;    // at most 3 elements at a tensor's end
    if (i < count) {
        const float gu = ld(g + i) * inv;
        acc += (double)gu * (double)gu;
    }
    return acc;
}

__global__ __launch_bounds__(NT) void optim_norm_kernel(const gvf_optim_tensor* __restrict__ tensors, const gvf_optim_chunk* __restrict__ chunks,
                                                        int64_t n_chunks, const float* __restrict__ inv_scale, double* __restrict__ part) {
    __shared__ double s_red[NT / GVF_WAVE];
    const float inv = inv_scale ? *inv_scale : 1.f;
    for (int64_t c = blockIdx.x; c < n_chunks; c += gridDim.x) {
        const gvf_optim_chunk ck = chunks[c];
        const float* g = tensors[ck.tensor].g + ck.first;
        // the same elements per lane on either path: the partial does not depend on the alignment
        const double acc = aligned16(g) ? chunk_sumsq<true>(g, ck.count, inv) : chunk_sumsq<false>(g, ck.count, inv);
        const double s = gvf_block_sum_waves<NT>(acc, s_red);
        if (threadIdx.x == 0) part[c] = s;
    }
}

struct FinalizeArgs {
    double lr[GVF_OPTIM_MAX_GROUPS];
    double beta1, beta2, max_grad_norm;
    int n_groups;
};

// 1024 lanes, four loads in flight per lane: the DiT's 13 122 slots are one latency-bound sweep of a single workgroup
__global__ __launch_bounds__(NT_FIN) void optim_finalize_kernel(const double* __restrict__ part, int64_t n_chunks, FinalizeArgs a,
                                                                gvf_optim_record* __restrict__ rec) {
    __shared__ double s_red[NT_FIN / GVF_WAVE];
    double s = 0.0;
    for (int64_t i = threadIdx.x; i < n_chunks; i += 4 * NT_FIN) {
        double x[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) x[u] = i + u * NT_FIN < n_chunks ? part[i + u * NT_FIN] : 0.0;
#pragma unroll
        for (int u = 0; u < 4; ++u) s += x[u];      // index order within the lane
    }
    s = gvf_block_sum_waves<NT_FIN>(s, s_red);
    if (threadIdx.x == 0) {
        const bool finite = isfinite(s);
        const float norm = (float)sqrt(s);
        float clip = 1.f;
        // torch.nn.utils.clip_grad_norm_: clamp(max_norm / (total_norm + 1e-6), max=1), where torch evaluates scalar / tensor as
        // reciprocal(tensor) * scalar -- two roundings, kept here so that the coefficient equals torch's bit for bit
        if (a.max_grad_norm >= 0.0) clip = fminf(1.f, (1.f / (norm + 1e-6f)) * (float)a.max_grad_norm);
        const int64_t step = rec->step + (finite ? 1 : 0);
        const double bc1 = 1.0 - pow(a.beta1, (double)step);
        const double rs2 = 1.0 / sqrt(1.0 - pow(a.beta2, (double)step));
        rec->grad_norm = norm;
        rec->found_inf = finite ? 0 : 1;
        rec->clip_coef = clip;
        rec->rsqrt_bc2 = (float)rs2;
        rec->step = step;
        rec->bc1 = bc1;
        rec->rsqrt_bc2_f64 = rs2;
        for (int g = 0; g < GVF_OPTIM_MAX_GROUPS; ++g) rec->step_size[g] = g < a.n_groups ? (float)(a.lr[g] / bc1) : 0.f;
    }
}

// -------------------------------------------------------------------------------------------------------------- update

struct UpdateCoef {
    float decay[GVF_OPTIM_MAX_GROUPS];   // 1 - lr * wd
    float beta1, omb1, beta2, omb2, eps;
    float rate[GVF_OPTIM_MAX_EMA], omr[GVF_OPTIM_MAX_EMA];
    int n_ema;
};

struct ElemCoef {
    float decay, step_size, rs2, clip, inv;
};

// p, m, v of one element (the order of gvf_optim.h; one rounding per operation)
__device__ __forceinline__ void adamw_elem(float& p, float g, float& m, float& v, const UpdateCoef& k, const ElemCoef& e) {
    const float gc = (g * e.inv) * e.clip;
    p = p * e.decay;
    m = k.beta1 * m + k.omb1 * gc;
    v = k.beta2 * v + (k.omb2 * gc) * gc;
    p = p - (e.step_size * m) / (sqrtf(v) * e.rs2 + k.eps);
}

template <bool VEC>
__device__ __forceinline__ void update_chunk(const gvf_optim_tensor& t, int64_t first, int count, const UpdateCoef& k, const ElemCoef& e, bool skip) {
    float* __restrict__ P = t.p + first;
    const float* __restrict__ G = t.g + first;
    float* __restrict__ M = t.m + first;
    float* __restrict__ V = t.v + first;
    const int n4 = count >> 2;
#pragma unroll 2
    for (int i = threadIdx.x; i < n4; i += NT) {
        const int64_t o = 4 * (int64_t)i;
        float p[4];
        load4<VEC>(P + o, p);
        if (!skip) {
            float g[4], m[4], v[4];
            load4<VEC>(G + o, g);
            load4<VEC>(M + o, m);
            load4<VEC>(V + o, v);
#pragma unroll
            for (int c = 0; c < 4; ++c) adamw_elem(p[c], g[c], m[c], v[c], k, e);
            store4<VEC>(P + o, p);
            store4<VEC>(M + o, m);
            store4<VEC>(V + o, v);
        }
#pragma unroll
        for (int j = 0; j < GVF_OPTIM_MAX_EMA; ++j) {
            if (j < k.n_ema) {
                float* __restrict__ E = t.ema[j] + first + o;
                float x[4];
                load4<VEC>(E, x);
#pragma unroll
                for (int c = 0; c < 4; ++c) x[c] = k.rate[j] * x[c] + k.omr[j] * p[c];
                store4<VEC>(E, x);
            }
        }
    }
    const int i = 4 * n4 + (int)threadIdx.x;    // at most 3 elements at a tensor's end
    if (i < count) {
        float p = ld(P + i);
        if (!skip) {
            float m = ld(M + i), v = ld(V + i);
            adamw_elem(p, ld(G + i), m, v, k, e);
            st(P + i, p);
            st(M + i, m);
            st(V + i, v);
        }
#pragma unroll
        for (int j = 0; j < GVF_OPTIM_MAX_EMA; ++j) {
            if (j < k.n_ema) {
                float* __restrict__ E = t.ema[j] + first;
                st(E + i, k.rate[j] * ld(E + i) + k.omr[j] * p);
            }
        }
    }
}

__global__ __launch_bounds__(NT) void optim_update_kernel(const gvf_optim_tensor* __restrict__ tensors, const gvf_optim_chunk* __restrict__ chunks,
                                                          int64_t n_chunks, const float* __restrict__ inv_scale,
                                                          const gvf_optim_record* __restrict__ rec, UpdateCoef k) {
    const bool skip = rec->found_inf != 0;
    ElemCoef e;
    e.inv = inv_scale ? *inv_scale : 1.f;
    e.clip = rec->clip_coef;
    e.rs2 = rec->rsqrt_bc2;
    for (int64_t c = blockIdx.x; c < n_chunks; c += gridDim.x) {
        const gvf_optim_chunk ck = chunks[c];
        const gvf_optim_tensor t = tensors[ck.tensor];
        const int grp = t.group & (GVF_OPTIM_MAX_GROUPS - 1);
        e.decay = k.decay[grp];
        e.step_size = rec->step_size[grp];
        bool vec = aligned16(t.p) && aligned16(t.g) && aligned16(t.m) && aligned16(t.v);
        for (int j = 0; j < GVF_OPTIM_MAX_EMA; ++j)
            if (j < k.n_ema) vec = vec && aligned16(t.ema[j]);
        if (vec)
            update_chunk<true>(t, ck.first, ck.count, k, e, skip);
        else
            update_chunk<false>(t, ck.first, ck.count, k, e, skip);
    }
}

bool in_unit_half_open(double b) { return b >= 0.0 && b < 1.0; }   // false for nan

bool hyper_ok(const gvf_optim_hyper* h) {
    if (!h) return false;
    if (h->n_groups < 1 || h->n_groups > GVF_OPTIM_MAX_GROUPS || h->n_ema < 0 || h->n_ema > GVF_OPTIM_MAX_EMA) return false;
    if (!in_unit_half_open(h->beta1) || !in_unit_half_open(h->beta2)) return false;
    if (!(h->eps > 0.0) || !isfinite(h->eps) || isnan(h->max_grad_norm)) return false;
    for (int g = 0; g < h->n_groups; ++g)
        if (!isfinite(h->lr[g]) || !isfinite(h->weight_decay[g])) return false;
    for (int j = 0; j < h->n_ema; ++j)
        if (!(h->ema_rate[j] >= 0.0 && h->ema_rate[j] <= 1.0)) return false;
    return true;
}

unsigned grid_of(int64_t n_chunks) { return (unsigned)(n_chunks < MAX_GRID ? n_chunks : MAX_GRID); }

}  // namespace

extern "C" int gvf_optim_chunk_len(void) { return CHUNK; }

extern "C" int gvf_optim_scratch_bytes(int64_t n_chunks, size_t* out) {
    if (!out || n_chunks <= 0 || n_chunks > ((int64_t)1 << 40)) return GVF_EINVAL;
    *out = gvf_align_up((size_t)n_chunks * sizeof(double), 256);
    return GVF_OK;
}

extern "C" int gvf_optim_norm(const gvf_optim_tensor* tensors, int n_tensors, const gvf_optim_chunk* chunks, int64_t n_chunks,
                              const gvf_optim_hyper* hyper, const float* inv_scale, gvf_optim_record* record, void* scratch,
                              size_t scratch_bytes, void* stream) {
    size_t need = 0;
    if (!tensors || !chunks || !record || !scratch || n_tensors <= 0 || !hyper_ok(hyper)) return GVF_EINVAL;
    if (gvf_optim_scratch_bytes(n_chunks, &need) != GVF_OK || scratch_bytes < need) return GVF_EINVAL;
    hipStream_t s = (hipStream_t)stream;
    double* part = (double*)scratch;
    optim_norm_kernel<<<dim3(grid_of(n_chunks)), NT, 0, s>>>(tensors, chunks, n_chunks, inv_scale, part);
    GVF_CHECK_LAUNCH();
    FinalizeArgs a;
    for (int g = 0; g < GVF_OPTIM_MAX_GROUPS; ++g) a.lr[g] = g < hyper->n_groups ? hyper->lr[g] : 0.0;
    a.beta1 = hyper->beta1;
    a.beta2 = hyper->beta2;
    a.max_grad_norm = hyper->max_grad_norm;
    a.n_groups = hyper->n_groups;
    optim_finalize_kernel<<<1, NT_FIN, 0, s>>>(part, n_chunks, a, record);
    GVF_CHECK_LAUNCH();
    return GVF_OK;
}

extern "C" int gvf_optim_adamw_update(const gvf_optim_tensor* tensors, int n_tensors, const gvf_optim_chunk* chunks, int64_t n_chunks,
                                      const gvf_optim_hyper* hyper, const float* inv_scale, const gvf_optim_record* record, void* stream) {
    if (!tensors || !chunks || !record || n_tensors <= 0 || n_chunks <= 0 || !hyper_ok(hyper)) return GVF_EINVAL;
    UpdateCoef k;
    for (int g = 0; g < GVF_OPTIM_MAX_GROUPS; ++g)
        k.decay[g] = g < hyper->n_groups ? (float)(1.0 - hyper->lr[g] * hyper->weight_decay[g]) : 1.f;
    k.beta1 = (float)hyper->beta1;
    k.omb1 = (float)(1.0 - hyper->beta1);
    k.beta2 = (float)hyper->beta2;
    k.omb2 = (float)(1.0 - hyper->beta2);
    k.eps = (float)hyper->eps;
    for (int j = 0; j < GVF_OPTIM_MAX_EMA; ++j) {
        k.rate[j] = j < hyper->n_ema ? (float)hyper->ema_rate[j] : 1.f;
        k.omr[j] = j < hyper->n_ema ? (float)(1.0 - hyper->ema_rate[j]) : 0.f;
    }
    k.n_ema = hyper->n_ema;
    optim_update_kernel<<<dim3(grid_of(n_chunks)), NT, 0, (hipStream_t)stream>>>(tensors, chunks, n_chunks, inv_scale, record, k);
    GVF_CHECK_LAUNCH();
    return GVF_OK;
}
