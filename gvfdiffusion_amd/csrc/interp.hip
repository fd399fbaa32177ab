// interp.hip -- KNN interpolation loss (forward and gradient), gfx950.  C ABI and rules 1-5: include/gvf_interp.h.
//
//   search:   one query per lane, 256 queries per workgroup.  The query and its running top K (distance + index, KP = K padded to
//             1, 4, 8 or 16) live in registers; the anchors of the sample pass through a 1024-anchor LDS tile ({x, y, z, -} per anchor,
//             read as one broadcast ds_read_b128 per anchor and wave).  A candidate is compared with the current K-th distance
//             first, so the sorted insert (divergent, about K ln(N / K) accepts per query) stays off the common path; strict < with anchors
//             visited in ascending index puts the lower index first among equal distances.  The epilogue computes the weights (rule 3).
//   apply / loss forward: one (b, p) per lane over a chunk of frames: the K indices, weights and static anchor rows stay in registers, the
//             moving rows are gathered per frame (the (T, N, 3) table of a sample is L2-sized).  The K products w_k (m_k - a_k) are formed and
//             summed in double (exact products of fp32 numbers, neighbour order) and rounded once for the fp32 estimate.  The loss variant
//             reads pred through its row stride, accumulates |pred - est| in double against the unrounded estimate and writes one double per
//             workgroup; one workgroup sums them in a fixed order.
//   backward: one (b, t, p) row per lane: sign byte -> three scaled signs (+ zero fill of the further channels).
// Every loop is bounded by an argument; no workgroup waits for another.
// Built with -ffp-contract=off (_build.py): rule 1 rounds every operation on its own (index decisions), rule 4 is a fixed sequence.
#include "gvf_common.h"
#include "gvf_rowops.h"
#include "../../include/gvf_rast.h"
#include "../../include/gvf_interp.h"

namespace {

constexpr int NT = 256;        // threads per workgroup
constexpr int TILE = 1024;     // anchors per LDS tile (16 KiB)
constexpr int MAXK = GVF_INTERP_MAX_K;

__device__ __forceinline__ int valid_queries(const int32_t* __restrict__ len, int b, int P) {
    if (!len) return P;
    const int v = len[b];
    return v < 0 ? 0 : (v > P ? P : v);
}

template <int KP>
__global__ __launch_bounds__(NT) void knn_search_kernel(const float* __restrict__ q, const int32_t* __restrict__ len,
                                                        const float* __restrict__ a, int P, int N, int K, float beta, int adaptive,
                                                        int32_t* __restrict__ idx, float* __restrict__ w, float* __restrict__ dist) {
    __shared__ float4 s_a[TILE];
    const int b = blockIdx.y;
    const int p = blockIdx.x * NT + threadIdx.x;
    const int nv = valid_queries(len, b, P);
    const bool valid = p < nv;
    const int64_t row = (int64_t)b * P + p;
    if ((int)(blockIdx.x * NT) >= nv) {        // a workgroup of padded queries only (uniform): zeros, no search
        if (p < P)
            for (int k = 0; k < K; ++k) {
                idx[row * K + k] = 0;
                w[row * K + k] = 0.f;
                if (dist) dist[row * K + k] = 0.f;
            }
        return;
    }
    float qx = 0.f, qy = 0.f, qz = 0.f;
    if (valid) {
        qx = q[row * 3];
        qy = q[row * 3 + 1];
        qz = q[row * 3 + 2];
    }
    float d[KP];
    int id[KP];
#pragma unroll
    for (int k = 0; k < KP; ++k) {
        d[k] = __builtin_inff();
        id[k] = 0;                              // stays in range even if no candidate is ever accepted (non-finite input)
    }
    const float* ab = a + (int64_t)b * N * 3;
    for (int n0 = 0; n0 < N; n0 += TILE) {
        const int cnt = N - n0 < TILE ? N - n0 : TILE;
        __syncthreads();
        for (int i = threadIdx.x; i < cnt; i += NT) {
            const float* s = ab + (int64_t)(n0 + i) * 3;
            s_a[i] = make_float4(s[0], s[1], s[2], 0.f);
        }
        __syncthreads();
        if (valid) {
#pragma unroll 4
            for (int j = 0; j < cnt; ++j) {
                const float4 v = s_a[j];
                const float dx = qx - v.x, dy = qy - v.y, dz = qz - v.z;
                const float dd = (dx * dx + dy * dy) + dz * dz;
                if (dd < d[KP - 1]) {
                    const int n = n0 + j;
#pragma unroll
                    for (int k = KP - 1; k > 0; --k) {
                        const bool shift = dd < d[k - 1];
                        const bool here = dd < d[k];
                        id[k] = shift ? id[k - 1] : (here ? n : id[k]);
                        d[k] = shift ? d[k - 1] : (here ? dd : d[k]);
                    }
                    if (dd < d[0]) {
                        d[0] = dd;
                        id[0] = n;
                    }
                }
            }
        }
    }
    if (p >= P) return;
    float wk[KP];
    if (valid) {
        float sum = 0.f;
#pragma unroll
        for (int k = 0; k < KP; ++k)
            if (k < K) sum += d[k];
        const float r = sqrtf(sum / (float)K) + 1e-6f;
        const float r2 = r * r;
        float ws = 0.f;
#pragma unroll
        for (int k = 0; k < KP; ++k) {
            float e = 0.f;
            if (k < K) {
                if (adaptive)
                    e = d[k] <= r2 ? expf((-beta * d[k]) / r2) : 0.f;
                else
                    e = expf(-beta * d[k]);
                ws += e;
            }
            wk[k] = e;
        }
        ws += 1e-8f;
#pragma unroll
        for (int k = 0; k < KP; ++k) wk[k] = wk[k] / ws;
    }
#pragma unroll
    for (int k = 0; k < KP; ++k) {
        if (k < K) {
            idx[row * K + k] = valid ? id[k] : 0;
            w[row * K + k] = valid ? wk[k] : 0.f;
            if (dist) dist[row * K + k] = valid ? d[k] : 0.f;
        }
    }
}

__device__ __forceinline__ int sgn3(double d) { return d > 0.0 ? 2 : (d < 0.0 ? 0 : 1); }   // sign + 1

// grid: (ceil(P / NT), frame chunks, B); frames [blockIdx.y * tc, min(T, (blockIdx.y + 1) * tc)).
// LOSS: reads pred, writes part[workgroup]; est / sign are written where not null.
template <int KP, bool LOSS>
__global__ __launch_bounds__(NT) void interp_apply_kernel(const float* __restrict__ pred, int64_t pstride, const int32_t* __restrict__ idx,
                                                          const float* __restrict__ w, const float* __restrict__ a,
                                                          const float* __restrict__ m, const int32_t* __restrict__ len, int T, int P, int N,
                                                          int K, int tc, float* __restrict__ est, uint8_t* __restrict__ sign,
                                                          double* __restrict__ part) {
    __shared__ double s_red[NT / GVF_WAVE];
    const int b = blockIdx.z;
    const int p = blockIdx.x * NT + threadIdx.x;
    const int t0 = blockIdx.y * tc;
    const int t1 = t0 + tc < T ? t0 + tc : T;
    const bool in = p < P;
    const bool valid = LOSS ? p < valid_queries(len, b, P) : in;
    double acc = 0.0;
    if (in) {
        const int64_t row = (int64_t)b * P + p;
        int id[KP];
        float wk[KP], ax[KP], ay[KP], az[KP];
#pragma unroll
        for (int k = 0; k < KP; ++k) {
            id[k] = 0;
            wk[k] = 0.f;
            ax[k] = ay[k] = az[k] = 0.f;
            if (k < K && valid) {
                const int i = idx[row * K + k];
                id[k] = i < 0 ? 0 : (i >= N ? N - 1 : i);
                wk[k] = w[row * K + k];
                const float* s = a + ((int64_t)b * N + id[k]) * 3;
                ax[k] = s[0];
                ay[k] = s[1];
                az[k] = s[2];
            }
        }
        for (int t = t0; t < t1; ++t) {
            const float* mt = m + ((int64_t)b * T + t) * N * 3;
            double ex = 0.0, ey = 0.0, ez = 0.0;           // exact products, summed in neighbour order, rounded once
            if (valid) {
#pragma unroll
                for (int k = 0; k < KP; ++k) {
                    if (k < K) {
                        const float* s = mt + (int64_t)id[k] * 3;
                        const double wd = (double)wk[k];
                        ex += wd * ((double)s[0] - (double)ax[k]);
                        ey += wd * ((double)s[1] - (double)ay[k]);
                        ez += wd * ((double)s[2] - (double)az[k]);
                    }
                }
            }
            const int64_t o = ((int64_t)b * T + t) * P + p;
            if (est) {
                est[o * 3] = (float)ex;
                est[o * 3 + 1] = (float)ey;
                est[o * 3 + 2] = (float)ez;
            }
            if (LOSS) {
                int code = 0x15;
                if (valid) {
                    const float* pr = pred + o * pstride;
                    const double gx = (double)pr[0] - ex, gy = (double)pr[1] - ey, gz = (double)pr[2] - ez;
                    acc += (fabs(gx) + fabs(gy)) + fabs(gz);
                    code = sgn3(gx) | (sgn3(gy) << 2) | (sgn3(gz) << 4);
                }
                if (sign) sign[o] = (uint8_t)code;
            }
        }
    }
    if (LOSS) {
        const double s = gvf_block_sum_waves<NT>(acc, s_red);
        if (threadIdx.x == 0) part[((int64_t)blockIdx.z * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x] = s;
    }
}

__device__ __forceinline__ double valid_total(const int32_t* __restrict__ len, int B, int P) {
    int64_t n = 0;
    for (int b = 0; b < B; ++b) n += valid_queries(len, b, P);
    return (double)n;
}

// one workgroup: fixed-order sum of the partials, divided by 3 T sum_b len[b]
__global__ __launch_bounds__(NT) void interp_loss_reduce_kernel(const double* __restrict__ part, int64_t nblk, const int32_t* __restrict__ len,
                                                                int B, int T, int P, float* __restrict__ loss_out) {
    __shared__ double s_red[NT / GVF_WAVE];
    double s = 0.0;
    for (int64_t i = threadIdx.x; i < nblk; i += NT) s += part[i];
    s = gvf_block_sum_waves<NT>(s, s_red);
    if (threadIdx.x == 0) loss_out[0] = (float)(s / (3.0 * (double)T * valid_total(len, B, P)));
}

__global__ __launch_bounds__(NT) void interp_loss_bwd_kernel(const uint8_t* __restrict__ sign, const float* __restrict__ grad_loss,
                                                             const int32_t* __restrict__ len, int B, int T, int P, int64_t rows,
                                                             float* __restrict__ grad, int64_t gstride, int gch) {
    __shared__ float s_c;                       // grad_loss / (3 T sum_b len[b]): one pass over len[] per workgroup
    if (threadIdx.x == 0) s_c = (float)((double)grad_loss[0] / (3.0 * (double)T * valid_total(len, B, P)));
    __syncthreads();
    const float c = s_c;
    for (int64_t o = (int64_t)blockIdx.x * NT + threadIdx.x; o < rows; o += (int64_t)gridDim.x * NT) {
        const int code = sign[o];
        float* g = grad + o * gstride;
        g[0] = c * (float)((code & 3) - 1);
        g[1] = c * (float)(((code >> 2) & 3) - 1);
        g[2] = c * (float)(((code >> 4) & 3) - 1);
        for (int ch = 3; ch < gch; ++ch) g[ch] = 0.f;
    }
}

struct Geom {
    int pblk, tchunks, tc;
    int64_t nblk;
};

// sizes shared by every entry point; the (b, t, p) row count times the widest row stride must fit the 64-bit offsets comfortably
bool sizes_ok(int B, int T, int P) {
    if (B <= 0 || T <= 0 || P <= 0 || B > 65535) return false;
    return (int64_t)B * T <= ((int64_t)1 << 40) / P;
}

bool knn_ok(int N, int K) { return N > 0 && K >= 1 && K <= MAXK && K <= N; }

// frame chunks: enough workgroups to fill the part when there are few queries, whole frame ranges per lane otherwise
bool geom_of(int B, int T, int P, Geom& g) {
    if (!sizes_ok(B, T, P)) return false;
    g.pblk = (P + NT - 1) / NT;
    const int64_t base = (int64_t)g.pblk * B;
    int want = (int)((2048 + base - 1) / base);
    if (want < 1) want = 1;
    if (want > T) want = T;
    g.tc = (T + want - 1) / want;
    g.tchunks = (T + g.tc - 1) / g.tc;
    if (g.tchunks > 65535) return false;
    g.nblk = base * g.tchunks;
    return true;
}

template <bool LOSS>
int launch_apply(const float* pred, int64_t pstride, const int32_t* idx, const float* w, const float* a, const float* m, const int32_t* len,
                 int B, int T, int P, int N, int K, const Geom& g, float* est, uint8_t* sign, double* part, hipStream_t s) {
    const dim3 grid((unsigned)g.pblk, (unsigned)g.tchunks, (unsigned)B);
#define GVF_INTERP_APPLY(KP) \
    interp_apply_kernel<KP, LOSS><<<grid, NT, 0, s>>>(pred, pstride, idx, w, a, m, len, T, P, N, K, g.tc, est, sign, part)
    if (K <= 1) GVF_INTERP_APPLY(1);
    else if (K <= 4) GVF_INTERP_APPLY(4);
    else if (K <= 8) GVF_INTERP_APPLY(8);
    else GVF_INTERP_APPLY(16);
#undef GVF_INTERP_APPLY
    GVF_CHECK_LAUNCH();
    return GVF_OK;
}

}  // namespace

extern "C" int gvf_knn_interp_weights(const float* q, const int32_t* len, const float* a, int B, int P, int N, int K, float beta,
                                      int adaptive, int32_t* idx, float* w, float* dist, void* stream) {
    if (!q || !a || !idx || !w || !sizes_ok(B, 1, P) || !knn_ok(N, K)) return GVF_EINVAL;
    hipStream_t s = (hipStream_t)stream;
    const dim3 grid((unsigned)((P + NT - 1) / NT), (unsigned)B);
#define GVF_INTERP_SEARCH(KP) knn_search_kernel<KP><<<grid, NT, 0, s>>>(q, len, a, P, N, K, beta, adaptive, idx, w, dist)
    if (K <= 1) GVF_INTERP_SEARCH(1);
    else if (K <= 4) GVF_INTERP_SEARCH(4);
    else if (K <= 8) GVF_INTERP_SEARCH(8);
    else GVF_INTERP_SEARCH(16);
#undef GVF_INTERP_SEARCH
    GVF_CHECK_LAUNCH();
    return GVF_OK;
}

extern "C" int gvf_knn_interp_apply(const int32_t* idx, const float* w, const float* a, const float* m, int B, int T, int P, int N, int K,
                                    float* est, void* stream) {
    Geom g;
    if (!idx || !w || !a || !m || !est || !knn_ok(N, K) || !geom_of(B, T, P, g)) return GVF_EINVAL;
    return launch_apply<false>(nullptr, 3, idx, w, a, m, nullptr, B, T, P, N, K, g, est, nullptr, nullptr, (hipStream_t)stream);
}

extern "C" int gvf_interp_loss_scratch_bytes(int B, int T, int P, size_t* out) {
    Geom g;
    if (!out || !geom_of(B, T, P, g)) return GVF_EINVAL;
    *out = gvf_align_up((size_t)g.nblk * sizeof(double), 256);
    return GVF_OK;
}

extern "C" int gvf_interp_loss_forward(const float* pred, int64_t pred_stride, const int32_t* idx, const float* w, const float* a,
                                       const float* m, const int32_t* len, int B, int T, int P, int N, int K, float* loss_out, float* est,
                                       uint8_t* sign, void* scratch, size_t scratch_bytes, void* stream) {
    Geom g;
    if (!pred || !idx || !w || !a || !m || !loss_out || !scratch || pred_stride < 3 || pred_stride > (1 << 20) || !knn_ok(N, K) ||
        !geom_of(B, T, P, g))
        return GVF_EINVAL;
    if (scratch_bytes < gvf_align_up((size_t)g.nblk * sizeof(double), 256)) return GVF_ENOSPC;
    hipStream_t s = (hipStream_t)stream;
    double* part = (double*)scratch;
    const int rc = launch_apply<true>(pred, pred_stride, idx, w, a, m, len, B, T, P, N, K, g, est, sign, part, s);
    if (rc != GVF_OK) return rc;
    interp_loss_reduce_kernel<<<1, NT, 0, s>>>(part, g.nblk, len, B, T, P, loss_out);
    GVF_CHECK_LAUNCH();
    return GVF_OK;
}

extern "C" int gvf_interp_loss_backward(const uint8_t* sign, const float* grad_loss, const int32_t* len, int B, int T, int P,
                                        float* grad_pred, int64_t grad_stride, int grad_channels, void* stream) {
    if (!sign || !grad_loss || !grad_pred || grad_stride < 3 || grad_stride > (1 << 20) || grad_channels < 3 ||
        grad_channels > grad_stride || !sizes_ok(B, T, P))
        return GVF_EINVAL;
    const int64_t rows = (int64_t)B * T * P;
    const int64_t blocks = (rows + NT - 1) / NT;
    interp_loss_bwd_kernel<<<dim3((unsigned)(blocks < 16384 ? blocks : 16384)), NT, 0, (hipStream_t)stream>>>(
        sign, grad_loss, len, B, T, P, rows, grad_pred, grad_stride, grad_channels);
    GVF_CHECK_LAUNCH();
    return GVF_OK;
}
