// rast_bwd.hip -- backward of the rasteriser operator (R7) over the workspace its forward call (rast.hip) left.
// blend_backward grid (tiles, F) -> per-(frame, Gaussian) accumulators in the caller's scratch; then one thread per Gaussian
// applies the chain rule -- per frame for gvf_rast_backward (preprocess_backward), per delta slice and its frames, then the GaussianModel
// activation Jacobian, for gvf_rast_backward_batched (activation_backward).  The forward records its record layout in the workspace.
#include <vector>
#include "rast_common.h"

namespace {

// ---------------------------------------------------------------------------------------------
// R7: backward of the operator (SURVEY.md section 8f NEXT #4; upstream backward.cu restated from its published
// algorithm, checked against oracle/rast_bwd_oracle.c which is pinned by finite differences).
// Conventions taken over from upstream: the gradient passes THROUGH alpha = min(0.99, .); a clamped EWA view
// coordinate gets no gradient; the screen-space mean's gradient is reported in NDC units.
// ---------------------------------------------------------------------------------------------

// Sums over the lanes of a wave without LDS round trips (a __shfl_xor butterfly is six ds_bpermute / ds_swizzle per
// value): rows of 16 lanes by DPP (quad permutes, then the two mirror patterns: after each step a lane holds the sum
// of a group twice as large); the four rows and the two halves by the gfx950 lane-swap instructions.
__device__ __forceinline__ float row_sum(float v) {          // every lane: sum of its row of 16 lanes
    int x;
#define GVF_DPP_ADD(ctrl_)                                                                                   \
    x = __builtin_amdgcn_update_dpp(0, __float_as_int(v), ctrl_, 0xf, 0xf, false);                          \
    v += __int_as_float(x);
    GVF_DPP_ADD(0xB1)      // quad_perm [1,0,3,2]
    GVF_DPP_ADD(0x4E)      // quad_perm [2,3,0,1]
    GVF_DPP_ADD(0x141)     // row_half_mirror
    GVF_DPP_ADD(0x140)     // row_mirror
#undef GVF_DPP_ADD
    return v;
}
__device__ __forceinline__ float across_rows_sum(float v) {  // every lane: sum of the lanes at its position in the 4 rows
    {   // rows (r0, r1, r2, r3) -> r0 + r1 resp. r2 + r3
        const auto sw = __builtin_amdgcn_permlane16_swap(__float_as_uint(v), __float_as_uint(v), false, false);
        v = __uint_as_float(sw[0]) + __uint_as_float(sw[1]);
    }
    {   // halves
        const auto sw = __builtin_amdgcn_permlane32_swap(__float_as_uint(v), __float_as_uint(v), false, false);
        v = __uint_as_float(sw[0]) + __uint_as_float(sw[1]);
    }
    return v;
}

// One workgroup per 16x16 tile, the 4 waves own its four 8x8 quadrants and walk per-wave lists of the splats whose
// alpha >= 1/255 box reaches the quadrant (exactly blend_kernel's culling, so the same splats are evaluated).
// Phase A replays the forward compositing (same arithmetic as blend_kernel: same skip / stop decisions) to get
// each pixel's final transmittance and the list position after its last contributor; phase B walks the lists back
// to front, forms the per-(pixel, splat) gradients, sums them over the 64 pixels of the wave and adds the wave
// sums to the per-Gaussian accumulators with hardware fp32 atomics.
// AUX: the depth / alpha outputs carry gradients (diff_gauss); the mip path has three channels and nine partials.
// Grid (tiles, F): frame f = blockIdx.y reads segment (f, tile) and the frame's records exactly as blend_kernel does -- the layout word the
// forward left in the workspace says whether a Gaussian's record sits at its id or at its Morton slot (rec_of) -- and adds into the
// frame's own accumulators acc[f][id][BWD_ACC] (the chain to 3-D differs by camera).
template <bool AUX>
__global__ __launch_bounds__(BLEND_THREADS) void blend_backward_kernel(
    int P, int H, int W, int gx, float bg0, float bg1, float bg2, const uint2* __restrict__ ranges,
    const uint32_t* __restrict__ point_list, const float4* __restrict__ splats, const float* __restrict__ subpixel_offset,
    const float* __restrict__ dL_dcolor, const float* __restrict__ dL_dalpha, const float* __restrict__ dL_ddepth,
    float* __restrict__ acc, const uint32_t* __restrict__ layout_word, const uint32_t* __restrict__ slot_of_id) {
    __shared__ float4 sA[BLEND_THREADS];
    __shared__ float4 sB[BLEND_THREADS];
    __shared__ float2 sC[BLEND_THREADS];
    __shared__ uint32_t sId[BLEND_THREADS];
    __shared__ float4 sL[BLEND_THREADS];                  // the forward's Cholesky form of the exponent (splat_cholesky): l11, l12, l22, c1
    __shared__ float2 sL2[BLEND_THREADS];                 // c2, log2(opacity)
    __shared__ unsigned char sMask[BLEND_THREADS];
    __shared__ unsigned char sList[4][BLEND_THREADS];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int tile = blockIdx.x, f = blockIdx.y;
    const int tx = tile % gx, ty = tile / gx;
    const int px = tx * TILE + (wave & 1) * 8 + (lane & 7), py = ty * TILE + (wave >> 1) * 8 + (lane >> 3);
    const bool inside = px < W && py < H;
    const size_t pid = (size_t)py * W + px, hw = (size_t)H * W;
    float pxf = (float)px, pyf = (float)py;
    if (subpixel_offset != nullptr && inside) { pxf += subpixel_offset[2 * pid]; pyf += subpixel_offset[2 * pid + 1]; }
    const uint32_t layout = *layout_word;
    const uint32_t* rec_of = (layout & LAYOUT_SLOT_ORDER) ? slot_of_id : nullptr;
    const uint2 rng = ranges[(size_t)f * gridDim.x + tile];              // blend_kernel's segment (gridDim.x = tiles of a frame)
    const float4* fsplats = splats + 4 * (size_t)f * P;
    dL_dcolor += (size_t)f * 3 * hw;
    if (dL_dalpha != nullptr) dL_dalpha += (size_t)f * hw;
    if (dL_ddepth != nullptr) dL_ddepth += (size_t)f * hw;
    acc += (size_t)f * P * BWD_ACC;
    const int n = (int)(rng.y - rng.x);
    const int rounds = (n + BLEND_THREADS - 1) / BLEND_THREADS;
    const uint64_t lt_mask = (1ull << lane) - 1ull;

// stage batch r_ (records, ids, quadrant masks) and compact it into this wave's list (ascending = depth order)
#define GVF_BWD_STAGE(r_, n_w_)                                                                     \
    {                                                                                               \
        const int k_ = (r_) * BLEND_THREADS + t;                                                    \
        if (k_ < n) {                                                                               \
            const uint32_t id_ = point_list[rng.x + (uint32_t)k_];                                  \
            const float4* rec_ = fsplats + 4 * (size_t)(rec_of != nullptr ? rec_of[id_] : id_);    \
            const float4 a_ = rec_[0];                                                              \
            const float4 c_ = rec_[2];                                                              \
            const float4 b_ = rec_[1];                                                              \
            const SplatChol ch_ = splat_cholesky(a_.x, a_.y, a_.z, a_.w, b_.x, (float)(tx * TILE), (float)(ty * TILE));   \
            sA[t] = a_; sB[t] = make_float4(b_.x, ch_.ok ? b_.y : 0.f, b_.z, b_.w); sC[t] = make_float2(c_.x, c_.y); sId[t] = id_;   \
            sL[t] = make_float4(ch_.l11, ch_.l12, ch_.l22, ch_.c1);                                  \
            sL2[t] = make_float2(ch_.c2, ch_.ok ? __builtin_amdgcn_logf(b_.y) : -__builtin_inff());  \
            sMask[t] = (unsigned char)quadrant_mask(a_.x, a_.y, a_.z, a_.w, b_.x, b_.y, c_.z, (float)(tx * TILE), (float)(ty * TILE), subpixel_offset != nullptr); \
        }                                                                                           \
        __syncthreads();                                                                            \
        const int cnt_ = min(BLEND_THREADS, n - (r_) * BLEND_THREADS);                              \
        n_w_ = 0;                                                                                   \
        _Pragma("unroll") for (int q_ = 0; q_ < BLEND_THREADS / GVF_WAVE; ++q_) {                   \
            const int idx_ = q_ * GVF_WAVE + lane;                                                  \
            const bool hit_ = idx_ < cnt_ && ((sMask[idx_] >> wave) & 1u);                          \
            const uint64_t bal_ = __ballot(hit_);                                                   \
            if (hit_) sList[wave][n_w_ + __popcll(bal_ & lt_mask)] = (unsigned char)idx_;           \
            n_w_ += __popcll(bal_);                                                                 \
        }                                                                                           \
        __builtin_amdgcn_wave_barrier();                                                            \
    }
    const float pxr = pxf - (float)(tx * TILE), pyr = pyf - (float)(ty * TILE);
    // ---- phase A: forward replay
    bool done = !inside;
    float T = 1.0f;
    int last = 0;
    for (int r = 0; r < rounds; ++r) {
        if (__syncthreads_count(done) == BLEND_THREADS) break;
        int n_w;
        GVF_BWD_STAGE(r, n_w)
        for (int jj = 0; jj < n_w; ++jj) {
            if (__all(done)) break;
            const int j = sList[wave][jj];
            const float4 L = sL[j];
            const float2 L2 = sL2[j];
            const float alpha = fminf(0.99f, __builtin_amdgcn_exp2f(-splat_neg_exponent(L.x, L.y, L.z, L.w, L2.x, pxr, pyr, L2.y)));   // the forward's arithmetic: same decisions
            const bool ok = !done && !(alpha < 1.0f / 255.0f);
            const float test_T = T - alpha * T;            // the forward's form
            const bool stop = ok && test_T < 0.0001f;
            done = done || stop;
            if (ok && !stop) { T = test_T; last = r * BLEND_THREADS + j + 1; }
        }
        __syncthreads();                                   // the batch is restaged next round
    }
    const float T_final = T;
    constexpr int NCH = AUX ? 5 : 3;                        // channels r, g, b (, depth, one)
    constexpr int NACC = AUX ? BWD_ACC : BWD_ACC - 1;       // without AUX the depth partial is identically zero
    float dch[5] = {0.f, 0.f, 0.f, 0.f, 0.f};
    if (inside) {
        dch[0] = dL_dcolor[pid]; dch[1] = dL_dcolor[hw + pid]; dch[2] = dL_dcolor[2 * hw + pid];
        if (AUX && dL_ddepth != nullptr) dch[3] = dL_ddepth[pid];
        if (AUX && dL_dalpha != nullptr) dch[4] = dL_dalpha[pid];
    }
    // what lies behind the current splat, per channel (r, g, b, depth, one); backgrounds (bg, 0, 0)
    float suf[5] = {T_final * bg0, T_final * bg1, T_final * bg2, 0.f, 0.f};
    int max_last = last;
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) max_last = max(max_last, __shfl_xor(max_last, o, 64));
    // ---- phase B: back to front
    __syncthreads();
    for (int r = rounds - 1; r >= 0; --r) {
        int n_w;
        GVF_BWD_STAGE(r, n_w)
        if (r * BLEND_THREADS < max_last) {                // else: nothing of this batch reached this wave's pixels
            for (int jj = n_w - 1; jj >= 0; --jj) {
                const int j = sList[wave][jj];
                const int k = r * BLEND_THREADS + j;
                if (k >= max_last) continue;               // wave-uniform
                const float4 a = sA[j];
                const float4 b = sB[j];
                const float2 c = sC[j];
                const float dx = a.x - pxf, dy = a.y - pyf;
                const float4 L = sL[j];
                const float2 L2 = sL2[j];
                const float G = __builtin_amdgcn_exp2f(-splat_neg_exponent(L.x, L.y, L.z, L.w, L2.x, pxr, pyr));
                const float alpha = fminf(0.99f, __builtin_amdgcn_exp2f(-splat_neg_exponent(L.x, L.y, L.z, L.w, L2.x, pxr, pyr, L2.y)));   // (the forward's alpha)
                const bool on = inside && k < last && !(alpha < 1.0f / 255.0f);
                if (!__any(on)) continue;
                float g[BWD_ACC];
#pragma unroll
                for (int e = 0; e < BWD_ACC; ++e) g[e] = 0.f;
                if (on) {
                    T = T / (1.f - alpha);                 // transmittance in front of this splat
                    const float cch[5] = {b.z, b.w, c.x, c.y, 1.0f};
                    const float inv1ma = 1.0f / (1.f - alpha);
                    float dL_da = 0.f;
#pragma unroll
                    for (int ch = 0; ch < NCH; ++ch) {
                        dL_da += (cch[ch] * T - suf[ch] * inv1ma) * dch[ch];
                        suf[ch] += cch[ch] * alpha * T;
                    }
                    const float w = alpha * T;
                    g[6] = w * dch[0]; g[7] = w * dch[1]; g[8] = w * dch[2];
                    if (AUX) g[9] = w * dch[3];
                    g[5] = G * dL_da;
                    const float dG = b.y * dL_da * G;      // dL/dpower (gradient passes through the 0.99 clamp)
                    const float ca = a.z * CONIC_IK1, cb = a.w * CONIC_IK2, cc = b.x * CONIC_IK1;   // the conic itself
                    g[0] = dG * (-ca * dx - cb * dy);
                    g[1] = dG * (-cc * dy - cb * dx);
                    g[2] = dG * (-0.5f * dx * dx);
                    g[3] = dG * (-dx * dy);
                    g[4] = dG * (-0.5f * dy * dy);
                }
                // row sums of the ten components, then position e of every row keeps component e, so that ONE
                // cross-row reduction finishes all ten; lanes 0-9 add them with one atomic instruction
#pragma unroll
                for (int e = 0; e < NACC; ++e) g[e] = row_sum(g[e]);
                float mine = g[0];
#pragma unroll
                for (int e = 1; e < NACC; ++e) mine = (lane & 15) == e ? g[e] : mine;
                mine = across_rows_sum(mine);
                if (lane < NACC) unsafeAtomicAdd(acc + (size_t)sId[j] * BWD_ACC + lane, mine);
            }
        }
        __syncthreads();                                   // everyone is done with this batch
    }
#undef GVF_BWD_STAGE
}

struct BwdParams {
    int P, M, deg, H, W, mode;
    float kernel_size, scale_modifier;
    GvfRastFrame fr;
};

// Per-(frame, Gaussian) chain rule from the blend's accumulators a[] to the activated inputs of that frame, geometry part: screen-space
// mean, depth, opacity and mip coefficient, EWA (2-D covariance, Jacobian, view transform), 3-D covariance -> scale and rotation (the
// forward intermediates are recomputed).  c6_precomp: the 3-D covariance given (s, q unused), else from s and q.  gcol = d/d(rgb).
struct FrameGeomGrad {
    float gm[3], gm2[2], gsc[3], gq[4], gc6[6], gop, gcol[3];
    bool vis;
};
__device__ __forceinline__ FrameGeomGrad frame_geom_backward(const GvfRastFrame& fr, int W, int H, int mode, float kernel_size,
                                                             float scale_modifier, const float (&a)[BWD_ACC], const float (&p)[3],
                                                             const float (&s)[3], const float (&q)[4], const float* c6_precomp,
                                                             float opacity) {
    FrameGeomGrad o;
#pragma unroll
    for (int k = 0; k < 3; ++k) { o.gm[k] = 0.f; o.gsc[k] = 0.f; o.gcol[k] = 0.f; }
#pragma unroll
    for (int k = 0; k < 4; ++k) o.gq[k] = 0.f;
#pragma unroll
    for (int k = 0; k < 6; ++k) o.gc6[k] = 0.f;
    o.gm2[0] = 0.f; o.gm2[1] = 0.f; o.gop = 0.f; o.vis = false;
    float pv[3];
    xform43(fr.viewmatrix, p, pv);
    if (pv[2] > 0.2f) {
        float ph[4];
        xform44(fr.projmatrix, p, ph);
        const float pw = 1.0f / (ph[3] + 0.0000001f);
        float c6[6];
        if (c6_precomp != nullptr) {
#pragma unroll
            for (int k = 0; k < 6; ++k) c6[k] = c6_precomp[k];
        } else {
            cov3d_from_scale_rot(s, scale_modifier, q, c6);
        }
        const float fx = (float)W / (2.0f * fr.tanfovx), fy = (float)H / (2.0f * fr.tanfovy);
        const float limx = 1.3f * fr.tanfovx, limy = 1.3f * fr.tanfovy;
        const float txtz = pv[0] / pv[2], tytz = pv[1] / pv[2];
        const float xmul = (txtz < -limx || txtz > limx) ? 0.f : 1.f, ymul = (tytz < -limy || tytz > limy) ? 0.f : 1.f;
        const float tx = fminf(limx, fmaxf(-limx, txtz)) * pv[2], ty = fminf(limy, fmaxf(-limy, tytz)) * pv[2], tz = pv[2];
        const float J00 = fx / tz, J02 = -(fx * tx) / (tz * tz), J11 = fy / tz, J12 = -(fy * ty) / (tz * tz);
        float A0[3], A1[3];
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const float w0 = fr.viewmatrix[c * 4 + 0], w1 = fr.viewmatrix[c * 4 + 1], w2 = fr.viewmatrix[c * 4 + 2];
            A0[c] = J00 * w0 + J02 * w2;
            A1[c] = J11 * w1 + J12 * w2;
        }
        const float S[3][3] = {{c6[0], c6[1], c6[2]}, {c6[1], c6[3], c6[4]}, {c6[2], c6[4], c6[5]}};
        float SA0[3], SA1[3];
#pragma unroll
        for (int r = 0; r < 3; ++r) {
            SA0[r] = S[r][0] * A0[0] + S[r][1] * A0[1] + S[r][2] * A0[2];
            SA1[r] = S[r][0] * A1[0] + S[r][1] * A1[1] + S[r][2] * A1[2];
        }
        const float cxx = A0[0] * SA0[0] + A0[1] * SA0[1] + A0[2] * SA0[2];
        const float cxy = A0[0] * SA1[0] + A0[1] * SA1[1] + A0[2] * SA1[2];
        const float cyy = A1[0] * SA1[0] + A1[1] * SA1[1] + A1[2] * SA1[2];
        const float kf = mode == GVF_RAST_MODE_MIP ? kernel_size : 0.3f;
        float coef = 1.0f;
        const float det0r = cxx * cyy - cxy * cxy, det1r = (cxx + kf) * (cyy + kf) - cxy * cxy;
        if (mode == GVF_RAST_MODE_MIP) {
            const float det0 = fmaxf(1e-6f, det0r), det1 = fmaxf(1e-6f, det1r);
            coef = sqrtf(det0 / (det1 + 1e-6f) + 1e-6f);
            if (det0 <= 1e-6f || det1 <= 1e-6f) coef = 0.0f;
        }
        const float ap = cxx + kf, bq = cxy, cp = cyy + kf;
        const float det = ap * cp - bq * bq;
        if (det != 0.0f) {
            o.vis = true;
            // screen-space mean (NDC units) and its path into the 3D mean
            o.gm2[0] = a[0] * 0.5f * (float)W; o.gm2[1] = a[1] * 0.5f * (float)H;
            const float* m = fr.projmatrix;
            const float mul1 = ph[0] * pw * pw, mul2 = ph[1] * pw * pw;
            o.gm[0] += (m[0] * pw - m[3] * mul1) * o.gm2[0] + (m[1] * pw - m[3] * mul2) * o.gm2[1];
            o.gm[1] += (m[4] * pw - m[7] * mul1) * o.gm2[0] + (m[5] * pw - m[7] * mul2) * o.gm2[1];
            o.gm[2] += (m[8] * pw - m[11] * mul1) * o.gm2[0] + (m[9] * pw - m[11] * mul2) * o.gm2[1];
            // depth output
            o.gm[0] += fr.viewmatrix[2] * a[9]; o.gm[1] += fr.viewmatrix[6] * a[9]; o.gm[2] += fr.viewmatrix[10] * a[9];
            // colour (precomputed colours directly; SH: frame_sh_backward)
            o.gcol[0] = a[6]; o.gcol[1] = a[7]; o.gcol[2] = a[8];
            // opacity and the mip coefficient
            o.gop = a[5] * coef;
            float gcxx = 0.f, gcxy = 0.f, gcyy = 0.f;
            if (mode == GVF_RAST_MODE_MIP && coef > 0.0f) {
                const float dcoef = a[5] * opacity;
                const float dr = dcoef * 0.5f / coef;
                const float d1e = det1r + 1e-6f;
                const float dd0 = dr / d1e, dd1 = -dr * det0r / (d1e * d1e);
                gcxx += dd0 * cyy + dd1 * (cyy + kf);
                gcyy += dd0 * cxx + dd1 * (cxx + kf);
                gcxy += -2.0f * cxy * (dd0 + dd1);
            }
            {
                const float d2 = 1.0f / (det * det);
                const float gA = a[2], gB = a[3], gC = a[4];
                gcxx += d2 * (-cp * cp * gA + bq * cp * gB - bq * bq * gC);
                gcxy += d2 * (2.f * bq * cp * gA - (det + 2.f * bq * bq) * gB + 2.f * ap * bq * gC);
                gcyy += d2 * (-bq * bq * gA + ap * bq * gB - ap * ap * gC);
            }
            float Gm[3][3];
#pragma unroll
            for (int r = 0; r < 3; ++r)
#pragma unroll
                for (int c = 0; c < 3; ++c) Gm[r][c] = gcxx * A0[r] * A0[c] + gcxy * A0[r] * A1[c] + gcyy * A1[r] * A1[c];
            o.gc6[0] = Gm[0][0]; o.gc6[3] = Gm[1][1]; o.gc6[5] = Gm[2][2];
            o.gc6[1] = Gm[0][1] + Gm[1][0]; o.gc6[2] = Gm[0][2] + Gm[2][0]; o.gc6[4] = Gm[1][2] + Gm[2][1];
            float dJ00 = 0.f, dJ02 = 0.f, dJ11 = 0.f, dJ12 = 0.f;
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const float dA0 = 2.f * gcxx * SA0[c] + gcxy * SA1[c], dA1 = 2.f * gcyy * SA1[c] + gcxy * SA0[c];
                const float w0 = fr.viewmatrix[c * 4 + 0], w1 = fr.viewmatrix[c * 4 + 1], w2 = fr.viewmatrix[c * 4 + 2];
                dJ00 += dA0 * w0; dJ02 += dA0 * w2; dJ11 += dA1 * w1; dJ12 += dA1 * w2;
            }
            const float tz2 = 1.0f / (tz * tz), tz3 = tz2 / tz;
            const float dtx = xmul * (-fx * tz2 * dJ02), dty = ymul * (-fy * tz2 * dJ12);
            const float dtz = -fx * tz2 * dJ00 - fy * tz2 * dJ11 + 2.f * fx * tx * tz3 * dJ02 + 2.f * fy * ty * tz3 * dJ12;
            const float* v = fr.viewmatrix;
            o.gm[0] += v[0] * dtx + v[1] * dty + v[2] * dtz;
            o.gm[1] += v[4] * dtx + v[5] * dty + v[6] * dtz;
            o.gm[2] += v[8] * dtx + v[9] * dty + v[10] * dtz;
            if (c6_precomp == nullptr) {
                const float r = q[0], x = q[1], y = q[2], z = q[3];
                const float R[3][3] = {{1.f - 2.f * (y * y + z * z), 2.f * (x * y - r * z), 2.f * (x * z + r * y)},
                                       {2.f * (x * y + r * z), 1.f - 2.f * (x * x + z * z), 2.f * (y * z - r * x)},
                                       {2.f * (x * z - r * y), 2.f * (y * z + r * x), 1.f - 2.f * (x * x + y * y)}};
                const float sc[3] = {scale_modifier * s[0], scale_modifier * s[1], scale_modifier * s[2]};
                const float Gs[3][3] = {{o.gc6[0], 0.5f * o.gc6[1], 0.5f * o.gc6[2]}, {0.5f * o.gc6[1], o.gc6[3], 0.5f * o.gc6[4]},
                                        {0.5f * o.gc6[2], 0.5f * o.gc6[4], o.gc6[5]}};
                float dR[3][3];
#pragma unroll
                for (int c = 0; c < 3; ++c) {
                    float acc_s = 0.f;
#pragma unroll
                    for (int r2 = 0; r2 < 3; ++r2) {
                        float dl = 0.f;
#pragma unroll
                        for (int kk = 0; kk < 3; ++kk) dl += 2.f * Gs[r2][kk] * R[kk][c] * sc[c];
                        acc_s += dl * R[r2][c];
                        dR[r2][c] = dl * sc[c];
                    }
                    o.gsc[c] = scale_modifier * acc_s;
                }
                o.gq[0] = 2.f * (-z * dR[0][1] + y * dR[0][2] + z * dR[1][0] - x * dR[1][2] - y * dR[2][0] + x * dR[2][1]);
                o.gq[1] = 2.f * (y * dR[0][1] + z * dR[0][2] + y * dR[1][0] - 2.f * x * dR[1][1] - r * dR[1][2] + z * dR[2][0] + r * dR[2][1] - 2.f * x * dR[2][2]);
                o.gq[2] = 2.f * (-2.f * y * dR[0][0] + x * dR[0][1] + r * dR[0][2] + x * dR[1][0] + z * dR[1][2] - r * dR[2][0] + z * dR[2][1] - 2.f * y * dR[2][2]);
                o.gq[3] = 2.f * (-2.f * z * dR[0][0] - r * dR[0][1] + x * dR[0][2] + r * dR[1][0] - 2.f * z * dR[1][1] + y * dR[1][2] + x * dR[2][0] + y * dR[2][1]);
            }
        }
    }
    return o;
}

// SH part of the per-frame chain rule (visible Gaussians): d/d(coefficients) = basis * d/d(rgb) where the +0.5 / clamp let it through,
// d/d(direction) -> added to the mean's gradient gm.  shc: the coefficients the forward evaluated (with the rgb delta added, fused path).
template <int DEG>
__device__ __forceinline__ void frame_sh_backward(const GvfRastFrame& fr, const float (&p)[3], const float (&shc)[(DEG + 1) * (DEG + 1)][3],
                                                  const float (&gcol_sh)[3], float (&gsh)[(DEG + 1) * (DEG + 1)][3], float (&gm)[3]) {
    constexpr int deg = DEG;
    const float dxc = p[0] - fr.campos[0], dyc = p[1] - fr.campos[1], dzc = p[2] - fr.campos[2];
    const float len = sqrtf(dxc * dxc + dyc * dyc + dzc * dzc);
    const float x = dxc / len, y = dyc / len, z = dzc / len;
    const float dirv[3] = {x, y, z};
    float bas[16], db[16][3];
#pragma unroll
    for (int k = 0; k < 16; ++k) { bas[k] = 0.f; db[k][0] = 0.f; db[k][1] = 0.f; db[k][2] = 0.f; }
    bas[0] = SH_C0;
    if (deg > 0) {
        bas[1] = -SH_C1 * y; bas[2] = SH_C1 * z; bas[3] = -SH_C1 * x;
        db[1][1] = -SH_C1; db[2][2] = SH_C1; db[3][0] = -SH_C1;
        if (deg > 1) {
            const float xx = x * x, yy = y * y, zz = z * z, xy = x * y, yz = y * z, xz = x * z;
            bas[4] = SH_C2[0] * xy; bas[5] = SH_C2[1] * yz; bas[6] = SH_C2[2] * (2.f * zz - xx - yy);
            bas[7] = SH_C2[3] * xz; bas[8] = SH_C2[4] * (xx - yy);
            db[4][0] = SH_C2[0] * y; db[4][1] = SH_C2[0] * x;
            db[5][1] = SH_C2[1] * z; db[5][2] = SH_C2[1] * y;
            db[6][0] = SH_C2[2] * -2.f * x; db[6][1] = SH_C2[2] * -2.f * y; db[6][2] = SH_C2[2] * 4.f * z;
            db[7][0] = SH_C2[3] * z; db[7][2] = SH_C2[3] * x;
            db[8][0] = SH_C2[4] * 2.f * x; db[8][1] = SH_C2[4] * -2.f * y;
            if (deg > 2) {
                bas[9] = SH_C3[0] * y * (3.f * xx - yy); bas[10] = SH_C3[1] * xy * z; bas[11] = SH_C3[2] * y * (4.f * zz - xx - yy);
                bas[12] = SH_C3[3] * z * (2.f * zz - 3.f * xx - 3.f * yy); bas[13] = SH_C3[4] * x * (4.f * zz - xx - yy);
                bas[14] = SH_C3[5] * z * (xx - yy); bas[15] = SH_C3[6] * x * (xx - 3.f * yy);
                db[9][0] = SH_C3[0] * 6.f * xy; db[9][1] = SH_C3[0] * (3.f * xx - 3.f * yy);
                db[10][0] = SH_C3[1] * yz; db[10][1] = SH_C3[1] * xz; db[10][2] = SH_C3[1] * xy;
                db[11][0] = SH_C3[2] * -2.f * xy; db[11][1] = SH_C3[2] * (4.f * zz - xx - 3.f * yy); db[11][2] = SH_C3[2] * 8.f * yz;
                db[12][0] = SH_C3[3] * -6.f * xz; db[12][1] = SH_C3[3] * -6.f * yz; db[12][2] = SH_C3[3] * (6.f * zz - 3.f * xx - 3.f * yy);
                db[13][0] = SH_C3[4] * (4.f * zz - 3.f * xx - yy); db[13][1] = SH_C3[4] * -2.f * xy; db[13][2] = SH_C3[4] * 8.f * xz;
                db[14][0] = SH_C3[5] * 2.f * xz; db[14][1] = SH_C3[5] * -2.f * yz; db[14][2] = SH_C3[5] * (xx - yy);
                db[15][0] = SH_C3[6] * (3.f * xx - 3.f * yy); db[15][1] = SH_C3[6] * -6.f * xy;
            }
        }
    }
    constexpr int nb = (DEG + 1) * (DEG + 1);
    float ddir[3] = {0.f, 0.f, 0.f};
    float res[3] = {0.f, 0.f, 0.f};
#pragma unroll
    for (int k = 0; k < nb; ++k)
#pragma unroll
        for (int c = 0; c < 3; ++c) res[c] += bas[k] * shc[k][c];
    float gr[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) gr[c] = (res[c] + 0.5f < 0.f) ? 0.f : gcol_sh[c];
#pragma unroll
    for (int k = 0; k < nb; ++k)
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            gsh[k][c] = bas[k] * gr[c];
            const float sg = shc[k][c] * gr[c];
            ddir[0] += db[k][0] * sg; ddir[1] += db[k][1] * sg; ddir[2] += db[k][2] * sg;
        }
    const float dot = ddir[0] * dirv[0] + ddir[1] * dirv[1] + ddir[2] * dirv[2];
    gm[0] += (ddir[0] - dirv[0] * dot) / len; gm[1] += (ddir[1] - dirv[1] * dot) / len; gm[2] += (ddir[2] - dirv[2] * dot) / len;
}

// Per-Gaussian chain rule from the blend's accumulators to the operator's inputs (one frame: gvf_rast_backward).
template <int DEG>      // SH degree: compile-time trip counts keep the basis arrays in registers
__global__ __launch_bounds__(PRE_THREADS) void preprocess_backward_kernel(
    BwdParams bp, const float* __restrict__ means3D, const float* __restrict__ shs, const float* __restrict__ colors_precomp,
    const float* __restrict__ opacities, const float* __restrict__ scales, const float* __restrict__ rotations,
    const float* __restrict__ cov3D_precomp, const float* __restrict__ acc, float* __restrict__ g_means3D,
    float* __restrict__ g_means2D, float* __restrict__ g_shs, float* __restrict__ g_colors, float* __restrict__ g_opac,
    float* __restrict__ g_scales, float* __restrict__ g_rots, float* __restrict__ g_cov3D) {
    const int i = blockIdx.x * PRE_THREADS + threadIdx.x;
    if (i >= bp.P) return;
    const GvfRastFrame& fr = bp.fr;
    const int M = bp.M;
    float a[BWD_ACC];
#pragma unroll
    for (int e = 0; e < BWD_ACC; ++e) a[e] = acc[(size_t)i * BWD_ACC + e];
    const float p[3] = {means3D[3 * (size_t)i], means3D[3 * (size_t)i + 1], means3D[3 * (size_t)i + 2]};
    float s[3] = {0.f, 0.f, 0.f}, q[4] = {0.f, 0.f, 0.f, 0.f};
    if (cov3D_precomp == nullptr) {
#pragma unroll
        for (int k = 0; k < 3; ++k) s[k] = scales[3 * (size_t)i + k];
#pragma unroll
        for (int k = 0; k < 4; ++k) q[k] = rotations[4 * (size_t)i + k];
    }
    const FrameGeomGrad g = frame_geom_backward(fr, bp.W, bp.H, bp.mode, bp.kernel_size, bp.scale_modifier, a, p, s, q,
                                                cov3D_precomp != nullptr ? cov3D_precomp + 6 * (size_t)i : nullptr, opacities[i]);
    float gm[3] = {g.gm[0], g.gm[1], g.gm[2]};
    if (shs != nullptr && g_shs != nullptr) {
        float* gs = g_shs + (size_t)i * M * 3;
        if (!g.vis) {
            for (int k = 0; k < M * 3; ++k) gs[k] = 0.f;
        } else {
            constexpr int nb = (DEG + 1) * (DEG + 1);
            const float* sh = shs + (size_t)i * M * 3;
            float shc[nb][3], gsh[nb][3];
#pragma unroll
            for (int k = 0; k < nb; ++k)
#pragma unroll
                for (int c = 0; c < 3; ++c) shc[k][c] = sh[k * 3 + c];
            frame_sh_backward<DEG>(fr, p, shc, g.gcol, gsh, gm);
#pragma unroll
            for (int k = 0; k < nb; ++k)
#pragma unroll
                for (int c = 0; c < 3; ++c) gs[k * 3 + c] = gsh[k][c];
            for (int k = nb * 3; k < M * 3; ++k) gs[k] = 0.f;      // coefficients above the active degree
        }
    }
#pragma unroll
    for (int e = 0; e < 3; ++e) g_means3D[3 * (size_t)i + e] = gm[e];
    if (g_means2D != nullptr) { g_means2D[2 * (size_t)i] = g.gm2[0]; g_means2D[2 * (size_t)i + 1] = g.gm2[1]; }
    if (g_colors != nullptr) {
        const bool c = colors_precomp != nullptr;
        g_colors[3 * (size_t)i] = c ? g.gcol[0] : 0.f; g_colors[3 * (size_t)i + 1] = c ? g.gcol[1] : 0.f; g_colors[3 * (size_t)i + 2] = c ? g.gcol[2] : 0.f;
    }
    g_opac[i] = g.gop;
    if (g_scales != nullptr) { g_scales[3 * (size_t)i] = g.gsc[0]; g_scales[3 * (size_t)i + 1] = g.gsc[1]; g_scales[3 * (size_t)i + 2] = g.gsc[2]; }
    if (g_rots != nullptr) { g_rots[4 * (size_t)i] = g.gq[0]; g_rots[4 * (size_t)i + 1] = g.gq[1]; g_rots[4 * (size_t)i + 2] = g.gq[2]; g_rots[4 * (size_t)i + 3] = g.gq[3]; }
    if (g_cov3D != nullptr) {
#pragma unroll
        for (int e = 0; e < 6; ++e) g_cov3D[6 * (size_t)i + e] = g.gc6[e];
    }
}

// ---- backward of gvf_rast_forward_batched: the frames' chain rules composed with the GaussianModel activations (gaussian_model.py:84-114)
struct BwdBatchedParams {
    int P, M, H, W, mode, F, nslices;
    float kernel_size, scale_modifier;
    GvfGaussianActivation act;
};

// Small host tables (the slice grouping below) travel as kernel arguments like the camera blocks: capturable, no host buffer outlives the call.
struct IntChunk { int32_t v[256]; };
__global__ void upload_ints_kernel(IntChunk c, int count, int32_t* __restrict__ dst) {
    if ((int)threadIdx.x < count) dst[threadIdx.x] = c.v[threadIdx.x];
}

// One thread per Gaussian.  groups = [F] frame indices grouped by delta slice (slices in order of first use, frames ascending inside) |
// [nslices + 1] group starts | [nslices] the slices' delta indices (-1: no delta).  Per slice: the activations are recomputed with the
// forward's own function (activate_one: the same bits the forward splatted), the gradients of the activated values are summed over the
// slice's frames (frame_geom_backward / frame_sh_backward, the single-frame chain rule), the activation Jacobian is applied once, which gives
// the slice's delta row, and that row is summed into the raw-parameter gradients.  A fixed order and no atomics: the result depends only on
// the blend backward's atomic order.  Null outputs are not written.
template <int DEG>
__global__ __launch_bounds__(PRE_THREADS) void activation_backward_kernel(
    BwdBatchedParams bp, const GvfRastFrame* __restrict__ frames, const int32_t* __restrict__ groups,
    const float* __restrict__ xyz_raw, const float* __restrict__ features_dc, const float* __restrict__ scaling_raw,
    const float* __restrict__ rotation_raw, const float* __restrict__ opacity_raw, const float* __restrict__ delta,
    const float* __restrict__ acc, float* __restrict__ g_xyz, float* __restrict__ g_fdc, float* __restrict__ g_scaling,
    float* __restrict__ g_rotation, float* __restrict__ g_opacity, float* __restrict__ g_delta) {
    const int i = blockIdx.x * PRE_THREADS + threadIdx.x;
    const int P = bp.P, M = bp.M;
    if (i >= P) return;
    constexpr int nb = (DEG + 1) * (DEG + 1);
    const GvfGaussianActivation& A = bp.act;
    const int32_t* grp = groups;
    const int32_t* gstart = groups + bp.F;
    const int32_t* gdi = gstart + bp.nslices + 1;
    float rx[3] = {0.f, 0.f, 0.f}, rs[3] = {0.f, 0.f, 0.f}, rq[4] = {0.f, 0.f, 0.f, 0.f}, ro = 0.f, rf[nb][3];
#pragma unroll
    for (int k = 0; k < nb; ++k) { rf[k][0] = 0.f; rf[k][1] = 0.f; rf[k][2] = 0.f; }
    for (int sl = 0; sl < bp.nslices; ++sl) {
        const int di = gdi[sl];
        const float* d = (delta != nullptr && di >= 0) ? delta + ((size_t)di * P + i) * 14 : nullptr;
        const ActGaussian g = activate_one(i, A, xyz_raw, scaling_raw, rotation_raw, opacity_raw, d);
        float shc[nb][3];
#pragma unroll
        for (int k = 0; k < nb; ++k)
#pragma unroll
            for (int c = 0; c < 3; ++c) shc[k][c] = features_dc[((size_t)i * M + k) * 3 + c] + g.drgb[c];   // sh_to_rgb's (sh + dadd)
        // gradients of the activated values, summed over the slice's frames
        float vp[3] = {0.f, 0.f, 0.f}, vs[3] = {0.f, 0.f, 0.f}, vq[4] = {0.f, 0.f, 0.f, 0.f}, vo = 0.f, vsh[nb][3];
#pragma unroll
        for (int k = 0; k < nb; ++k) { vsh[k][0] = 0.f; vsh[k][1] = 0.f; vsh[k][2] = 0.f; }
        for (int e = gstart[sl]; e < gstart[sl + 1]; ++e) {
            const int f = grp[e];
            const GvfRastFrame& fr = frames[f];
            float a[BWD_ACC];
            const float* af = acc + ((size_t)f * P + i) * BWD_ACC;
#pragma unroll
            for (int k = 0; k < BWD_ACC; ++k) a[k] = af[k];
            const FrameGeomGrad fg = frame_geom_backward(fr, bp.W, bp.H, bp.mode, bp.kernel_size, bp.scale_modifier, a, g.p, g.s, g.q,
                                                         nullptr, g.op);
            float gm[3] = {fg.gm[0], fg.gm[1], fg.gm[2]};
            if (fg.vis) {
                float gsh[nb][3];
                frame_sh_backward<DEG>(fr, g.p, shc, fg.gcol, gsh, gm);
#pragma unroll
                for (int k = 0; k < nb; ++k) { vsh[k][0] += gsh[k][0]; vsh[k][1] += gsh[k][1]; vsh[k][2] += gsh[k][2]; }
            }
#pragma unroll
            for (int k = 0; k < 3; ++k) { vp[k] += gm[k]; vs[k] += fg.gsc[k]; }
#pragma unroll
            for (int k = 0; k < 4; ++k) vq[k] += fg.gq[k];
            vo += fg.gop;
        }
        // activation Jacobians (activate_vals): d/d(pre-activation value) = d/d(delta entry)
        float dd[14];
#pragma unroll
        for (int k = 0; k < 3; ++k) dd[k] = vp[k];                                       // xyz: _xyz * aabb[3:] + aabb[:3] + delta
#pragma unroll
        for (int k = 0; k < 3; ++k) {                                                    // scale: sqrt(act(x)^2 + k^2)
            float x = scaling_raw[3 * (size_t)i + k] + A.scale_bias;
            if (d) x = x + d[3 + k];
            float av, dav;
            if (A.scaling_activation == 0) { av = act_expf(x); dav = av; }
            else if (x > 20.0f) { av = x; dav = 1.0f; }                                  // softplus' linear branch (threshold 20)
            else { const float ex = act_expf(x); av = act_log1pf(ex); dav = ex / (1.0f + ex); }
            dd[3 + k] = vs[k] * (av * dav / g.s[k]);
        }
        {                                                                                // rotation: q / max(|q|, 1e-12)
            float q[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                q[k] = rotation_raw[4 * (size_t)i + k] + (k == 0 ? 1.0f : 0.0f);
                if (d) q[k] = q[k] + d[6 + k];
            }
            const float n = sqrtf(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
            if (n > 1e-12f) {
                const float dot = g.q[0] * vq[0] + g.q[1] * vq[1] + g.q[2] * vq[2] + g.q[3] * vq[3];
#pragma unroll
                for (int k = 0; k < 4; ++k) dd[6 + k] = (vq[k] - g.q[k] * dot) / n;
            } else {
#pragma unroll
                for (int k = 0; k < 4; ++k) dd[6 + k] = vq[k] / 1e-12f;
            }
        }
#pragma unroll
        for (int c = 0; c < 3; ++c) {                                                    // rgb: added to every SH coefficient row
            float sum = 0.f;
#pragma unroll
            for (int k = 0; k < nb; ++k) sum += vsh[k][c];
            dd[10 + c] = sum;
        }
        dd[13] = vo * (g.op * (1.0f - g.op));                                            // opacity: sigmoid
        if (g_delta != nullptr && d != nullptr) {
            float* o = g_delta + ((size_t)di * P + i) * 14;
#pragma unroll
            for (int k = 0; k < 14; ++k) o[k] = dd[k];
        }
#pragma unroll
        for (int k = 0; k < 3; ++k) { rx[k] += dd[k] * A.aabb[3 + k]; rs[k] += dd[3 + k]; }
#pragma unroll
        for (int k = 0; k < 4; ++k) rq[k] += dd[6 + k];
        ro += dd[13];
#pragma unroll
        for (int k = 0; k < nb; ++k) { rf[k][0] += vsh[k][0]; rf[k][1] += vsh[k][1]; rf[k][2] += vsh[k][2]; }
    }
    if (g_xyz != nullptr) { g_xyz[3 * (size_t)i] = rx[0]; g_xyz[3 * (size_t)i + 1] = rx[1]; g_xyz[3 * (size_t)i + 2] = rx[2]; }
    if (g_scaling != nullptr) { g_scaling[3 * (size_t)i] = rs[0]; g_scaling[3 * (size_t)i + 1] = rs[1]; g_scaling[3 * (size_t)i + 2] = rs[2]; }
    if (g_rotation != nullptr) {
#pragma unroll
        for (int k = 0; k < 4; ++k) g_rotation[4 * (size_t)i + k] = rq[k];
    }
    if (g_opacity != nullptr) g_opacity[i] = ro;
    if (g_fdc != nullptr) {
        float* o = g_fdc + (size_t)i * M * 3;
#pragma unroll
        for (int k = 0; k < nb; ++k) { o[3 * k] = rf[k][0]; o[3 * k + 1] = rf[k][1]; o[3 * k + 2] = rf[k][2]; }
        for (int k = nb * 3; k < M * 3; ++k) o[k] = 0.f;                                 // coefficients above the active degree
    }
}

// blend_backward over (tiles, F frames) of the forward call's workspace; AUX when the alpha / depth outputs carry gradients
void launch_blend_backward(hipStream_t stream, const GvfRastSettings& st, int P, int F, const Workspace& w, const float* subpixel_offset,
                           const float* dL_dcolor, const float* dL_dalpha, const float* dL_ddepth, float* acc) {
    const int H = st.image_height, W = st.image_width;
    const int gx = (W + TILE - 1) / TILE, gy = (H + TILE - 1) / TILE;
    auto* kernel = (dL_dalpha != nullptr || dL_ddepth != nullptr) ? blend_backward_kernel<true> : blend_backward_kernel<false>;
    hipLaunchKernelGGL(kernel, dim3(gx * gy, F), dim3(BLEND_THREADS), 0, stream, P, H, W, gx, st.bg[0], st.bg[1], st.bg[2], w.ranges, w.ids,
                       w.splats, subpixel_offset, dL_dcolor, dL_dalpha, dL_ddepth, acc, w.mm + LAYOUT_WORD, w.order_alt);
}

}  // namespace

extern "C" int gvf_rast_backward_scratch_bytes(int P, size_t* bytes) {
    if (!bytes || P < 0) return GVF_EINVAL;
    *bytes = gvf_align_up((size_t)(P > 0 ? P : 1) * BWD_ACC * sizeof(float), 256);
    return GVF_OK;
}

extern "C" int gvf_rast_backward(const GvfRastSettings* st, const GvfRastFrame* frame_host, int P, int M,
                                 const float* means3D, const float* shs, const float* colors_precomp,
                                 const float* opacities, const float* scales, const float* rotations,
                                 const float* cov3D_precomp, const float* subpixel_offset, const void* workspace,
                                 size_t workspace_bytes, int64_t max_rendered, const float* dL_dcolor,
                                 const float* dL_dalpha, const float* dL_ddepth, void* scratch, size_t scratch_bytes,
                                 float* dL_dmeans3D, float* dL_dmeans2D, float* dL_dshs, float* dL_dcolors,
                                 float* dL_dopacities, float* dL_dscales, float* dL_drotations, float* dL_dcov3D,
                                 void* stream_) {
    if (!st || !frame_host || !workspace || !dL_dcolor || P < 0) return GVF_EINVAL;
    const int H = st->image_height, W = st->image_width;
    if (H <= 0 || W <= 0 || st->sh_degree < 0 || st->sh_degree > 3) return GVF_EINVAL;
    if (st->mode != GVF_RAST_MODE_MIP && st->mode != GVF_RAST_MODE_DILATE) return GVF_EINVAL;
    if (P == 0) return GVF_OK;
    if (!means3D || !opacities || !scratch || !dL_dmeans3D || !dL_dopacities) return GVF_EINVAL;
    if ((shs == nullptr) == (colors_precomp == nullptr)) return GVF_EINVAL;
    const bool have_sr = scales != nullptr && rotations != nullptr;
    if (have_sr == (cov3D_precomp != nullptr)) return GVF_EINVAL;
    if (shs != nullptr && (M < (st->sh_degree + 1) * (st->sh_degree + 1) || M > MAX_SH_COEFFS || !dL_dshs)) return GVF_EINVAL;
    if (colors_precomp != nullptr && !dL_dcolors) return GVF_EINVAL;
    if (have_sr && (!dL_dscales || !dL_drotations)) return GVF_EINVAL;
    if (!have_sr && !dL_dcov3D) return GVF_EINVAL;
    size_t need = 0;
    gvf_rast_backward_scratch_bytes(P, &need);
    if (scratch_bytes < need) return GVF_ENOSPC;
    if ((((uintptr_t)workspace) & 255) != 0 || (((uintptr_t)scratch) & 15) != 0) return GVF_EINVAL;
    hipStream_t stream = (hipStream_t)stream_;
    (void)hipGetLastError();
    // the layout of the forward call's workspace: same (P, F = 1, H, W, max_rendered) => same carve
    Workspace w = carve(const_cast<void*>(workspace), workspace_bytes, P, 1, H, W, max_rendered);
    if (!w.ok) return GVF_ENOSPC;
    float* acc = (float*)scratch;
    if (hipMemsetAsync(acc, 0, (size_t)P * BWD_ACC * sizeof(float), stream) != hipSuccess) return GVF_ELAUNCH;
    if (max_rendered > 0) launch_blend_backward(stream, *st, P, 1, w, subpixel_offset, dL_dcolor, dL_dalpha, dL_ddepth, acc);
    GVF_CHECK_LAUNCH();
    BwdParams bp;
    bp.P = P; bp.M = M; bp.deg = st->sh_degree; bp.H = H; bp.W = W; bp.mode = st->mode;
    bp.kernel_size = st->kernel_size; bp.scale_modifier = st->scale_modifier; bp.fr = *frame_host;
#define GVF_PRE_BWD(D_)                                                                                                         \
    hipLaunchKernelGGL(preprocess_backward_kernel<D_>, dim3((P + PRE_THREADS - 1) / PRE_THREADS), dim3(PRE_THREADS), 0, stream, bp, \
                       means3D, shs, colors_precomp, opacities, scales, rotations, cov3D_precomp, acc, dL_dmeans3D, dL_dmeans2D,    \
                       dL_dshs, dL_dcolors, dL_dopacities, dL_dscales, dL_drotations, dL_dcov3D)
    switch (shs != nullptr ? st->sh_degree : 0) {
        case 0: GVF_PRE_BWD(0); break;
        case 1: GVF_PRE_BWD(1); break;
        case 2: GVF_PRE_BWD(2); break;
        default: GVF_PRE_BWD(3); break;
    }
#undef GVF_PRE_BWD
    GVF_CHECK_LAUNCH();
    return GVF_OK;
}

extern "C" int gvf_rast_backward_batched_scratch_bytes(int P, int F, size_t* bytes) {
    if (!bytes || P < 0 || F <= 0) return GVF_EINVAL;
    *bytes = gvf_align_up((size_t)F * (size_t)(P > 0 ? P : 1) * BWD_ACC * sizeof(float), 256) +   // accumulators [F][P][BWD_ACC]
             gvf_align_up((3 * (size_t)F + 1) * sizeof(int32_t), 256);                             // slice grouping of the frames
    return GVF_OK;
}

extern "C" int gvf_rast_backward_batched(const GvfRastSettings* st, const GvfRastFrame* frames_host, int F,
                                         const GvfGaussianActivation* act, int P, int M, const float* xyz_raw,
                                         const float* features_dc, const float* scaling_raw, const float* rotation_raw,
                                         const float* opacity_raw, const float* delta, int n_delta, const void* workspace,
                                         size_t workspace_bytes, int64_t max_rendered, const float* dL_dcolor,
                                         const float* dL_dalpha, const float* dL_ddepth, void* scratch, size_t scratch_bytes,
                                         float* dL_dxyz_raw, float* dL_dfeatures_dc, float* dL_dscaling_raw,
                                         float* dL_drotation_raw, float* dL_dopacity_raw, float* dL_ddelta, void* stream_) {
    // every argument check comes before the first HIP call
    if (!st || !frames_host || !act || !workspace || !dL_dcolor || F <= 0 || P < 0 || n_delta < 0) return GVF_EINVAL;
    const int H = st->image_height, W = st->image_width;
    if (H <= 0 || W <= 0 || st->sh_degree < 0 || st->sh_degree > 3) return GVF_EINVAL;
    if (st->mode != GVF_RAST_MODE_MIP) return GVF_EINVAL;
    if (max_rendered < 0 || max_rendered > 0xFFFFFFFFll) return GVF_EINVAL;
    if (act->scaling_activation != 0 && act->scaling_activation != 1) return GVF_EINVAL;
    for (int f = 0; f < F; ++f) {
        const int di = frames_host[f].delta_index;
        if (di >= 0 && (delta == nullptr || di >= n_delta)) return GVF_EINVAL;
    }
    if (P > 0) {
        if (!xyz_raw || !features_dc || !scaling_raw || !rotation_raw || !opacity_raw) return GVF_EINVAL;
        if (M < (st->sh_degree + 1) * (st->sh_degree + 1) || M > MAX_SH_COEFFS) return GVF_EINVAL;
    }
    size_t need = 0;
    gvf_rast_backward_batched_scratch_bytes(P, F, &need);
    if (!scratch || scratch_bytes < need) return GVF_ENOSPC;
    if ((((uintptr_t)workspace) & 255) != 0 || (((uintptr_t)scratch) & 15) != 0) return GVF_EINVAL;
    Workspace w = carve(const_cast<void*>(workspace), workspace_bytes, P, F, H, W, max_rendered);   // the forward call's carve
    if (!w.ok) return GVF_ENOSPC;
    if (P == 0) return GVF_OK;
    // frames grouped by delta slice (slices in order of first use, as the forward's plan groups them; no limit on their number here):
    // [F] frames | [ns + 1] starts | [ns] delta indices
    std::vector<int32_t> slices, frame_slice;
    group_slices(frames_host, F, delta != nullptr, 0, slices, frame_slice);
    const int ns = (int)slices.size();
    const std::vector<int32_t> tab = slice_table(slices, frame_slice);

    hipStream_t stream = (hipStream_t)stream_;
    (void)hipGetLastError();
    float* acc = (float*)scratch;
    const size_t acc_bytes = (size_t)F * P * BWD_ACC * sizeof(float);
    int32_t* groups = reinterpret_cast<int32_t*>((char*)scratch + gvf_align_up(acc_bytes, 256));
    if (hipMemsetAsync(acc, 0, acc_bytes, stream) != hipSuccess) return GVF_ELAUNCH;
    if (dL_ddelta != nullptr && n_delta > 0 &&          // slices no frame selects: exact zeros
        hipMemsetAsync(dL_ddelta, 0, (size_t)n_delta * P * 14 * sizeof(float), stream) != hipSuccess) return GVF_ELAUNCH;
    for (size_t k0 = 0; k0 < tab.size(); k0 += 256) {
        IntChunk c;
        const int cnt = (int)(tab.size() - k0 < 256 ? tab.size() - k0 : 256);
        for (int k = 0; k < cnt; ++k) c.v[k] = tab[k0 + (size_t)k];
        hipLaunchKernelGGL(upload_ints_kernel, dim3(1), dim3(256), 0, stream, c, cnt, groups + k0);
    }
    if (max_rendered > 0) launch_blend_backward(stream, *st, P, F, w, nullptr, dL_dcolor, dL_dalpha, dL_ddepth, acc);
    GVF_CHECK_LAUNCH();
    BwdBatchedParams bp;
    bp.P = P; bp.M = M; bp.H = H; bp.W = W; bp.mode = st->mode; bp.F = F; bp.nslices = ns;
    bp.kernel_size = st->kernel_size; bp.scale_modifier = st->scale_modifier; bp.act = *act;
#define GVF_ACT_BWD(D_)                                                                                                            \
    hipLaunchKernelGGL(activation_backward_kernel<D_>, dim3((P + PRE_THREADS - 1) / PRE_THREADS), dim3(PRE_THREADS), 0, stream, bp, \
                       w.frames, groups, xyz_raw, features_dc, scaling_raw, rotation_raw, opacity_raw, delta, acc, dL_dxyz_raw,      \
                       dL_dfeatures_dc, dL_dscaling_raw, dL_drotation_raw, dL_dopacity_raw, dL_ddelta)
    switch (st->sh_degree) {
        case 0: GVF_ACT_BWD(0); break;
        case 1: GVF_ACT_BWD(1); break;
        case 2: GVF_ACT_BWD(2); break;
        default: GVF_ACT_BWD(3); break;
    }
#undef GVF_ACT_BWD
    GVF_CHECK_LAUNCH();
    return GVF_OK;
}

