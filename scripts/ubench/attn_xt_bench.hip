// attn_xt_bench.hip -- standalone check + timing of csrc/attn_xt.hip (tiled-cache cross attention) on the DiT's shapes.
//   hipcc --offload-arch=gfx950 -O3 -std=c++17 <attn flags> [-DXT_RING_STAGES=..] [-DXT_TILES_PER_STAGE=..] [-DXT_TIMING] attn_xt_bench.hip -o attn_xt_bench_<tag>
// Checks sampled (frame, head, query) rows against a float64 host reference built from the SAME bf16 operands
// (so the difference is the kernel's own arithmetic: bf16 probabilities, fp32 accumulation, bf16 output), then times it.
#include "../../gvfdiffusion_amd/csrc/attn_xt.hip"
#include <cmath>
#include <cstdio>
#include <cstring>
#include <random>
#include <vector>

static unsigned short h_f2bf(float f) {
    unsigned u; memcpy(&u, &f, 4);
    u += 0x7fffu + ((u >> 16) & 1u);
    return (unsigned short)(u >> 16);
}
static float h_bf2f(unsigned short h) { unsigned u = ((unsigned)h) << 16; float f; memcpy(&f, &u, 4); return f; }

#define CK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { printf("HIP error %s at %d\n", hipGetErrorString(e_), __LINE__); return 1; } } while (0)

static int run_case(const char* name, int n_outer, int n_inner, int Lq, int Lk, int H, bool shared_kv, float k_gain, int force_exact, int iters) {
    const int C = H * 32;
    const long long M = (long long)n_outer * n_inner * Lq;
    const int n_sets = shared_kv ? n_outer : n_outer * n_inner;
    const int n_tiles = (Lk + 63) / 64;
    std::mt19937 rng(1234);
    std::normal_distribution<float> nd(0.f, 1.f);
    std::vector<unsigned short> hq(M * C);
    for (auto& v : hq) v = h_f2bf(nd(rng));
    std::vector<float> hkv((size_t)n_sets * Lk * 2 * C);
    for (size_t i = 0; i < hkv.size(); ++i) hkv[i] = nd(rng) * (((i / C) & 1) ? 1.f : k_gain);
    const float scale = 1.0f / sqrtf(32.f), ksc = scale * 1.4426950408889634f;

    unsigned short *dq, *dout; float* dkv; uint4 *dkt, *dvt;
    const size_t tile_bytes = (size_t)n_sets * H * n_tiles * 4096;
    CK(hipMalloc(&dq, hq.size() * 2)); CK(hipMalloc(&dout, hq.size() * 2)); CK(hipMalloc(&dkv, hkv.size() * 4));
    CK(hipMalloc(&dkt, tile_bytes)); CK(hipMalloc(&dvt, tile_bytes));
    CK(hipMemcpy(dq, hq.data(), hq.size() * 2, hipMemcpyHostToDevice));
    CK(hipMemcpy(dkv, hkv.data(), hkv.size() * 4, hipMemcpyHostToDevice));
    CK(hipMemset(dout, 0xff, hq.size() * 2));
    int* dfb; CK(hipMalloc(&dfb, 4)); CK(hipMemset(dfb, 0, 4));
    int rc = gvf_attn_pack_kv_bf16(dkv, 1, 2 * C, 0, C, n_sets, Lk, H, ksc, nullptr, dkt, dvt, nullptr);
    if (rc) { printf("pack rc %d\n", rc); return 1; }
    const int64_t qs[4] = {(int64_t)n_inner * Lq * C, (int64_t)Lq * C, C, 32};
    rc = gvf_attn_tiled_fwd_bf16(dq, dkt, dvt, dout, n_outer, n_inner, Lq, Lk, H, qs, qs, shared_kv ? 1 : n_inner, shared_kv ? 0 : 1, nullptr, 0, force_exact, dfb, nullptr);
    if (rc) { printf("attn rc %d\n", rc); return 1; }
    CK(hipDeviceSynchronize());
    std::vector<unsigned short> hout(hq.size());
    CK(hipMemcpy(hout.data(), dout, hout.size() * 2, hipMemcpyDeviceToHost));

    // reference on sampled rows
    double num = 0, den = 0, maxabs = 0;
    int nan_count = 0;
    const int n_samples = 96;
    for (int sidx = 0; sidx < n_samples; ++sidx) {
        const int o = sidx % n_outer, in = (sidx * 7) % n_inner, h = (sidx * 5) % H;
        const int qi = (sidx * 37 + (sidx % 3 == 0 ? Lq - 1 - sidx : 0)) % Lq;
        const long long row = ((long long)o * n_inner + in) * Lq + qi;
        const int set = shared_kv ? o : o * n_inner + in;
        std::vector<double> s(Lk);
        double m = -1e300;
        for (int k = 0; k < Lk; ++k) {
            double acc = 0;
            for (int d = 0; d < 32; ++d) {
                const float kq = h_bf2f(h_f2bf(hkv[((size_t)set * Lk + k) * 2 * C + h * 32 + d] * ksc));
                acc += (double)h_bf2f(hq[row * C + h * 32 + d]) * kq;
            }
            s[k] = acc; m = acc > m ? acc : m;
        }
        double l = 0, ov[32] = {0};
        for (int k = 0; k < Lk; ++k) {
            const double p = exp2(s[k] - m);
            l += p;
            for (int d = 0; d < 32; ++d) ov[d] += p * h_bf2f(h_f2bf(hkv[((size_t)set * Lk + k) * 2 * C + C + h * 32 + d]));
        }
        for (int d = 0; d < 32; ++d) {
            const double ref = ov[d] / l, got = h_bf2f(hout[row * C + h * 32 + d]);
            if (!(got == got)) ++nan_count;
            num += (got - ref) * (got - ref); den += ref * ref;
            maxabs = fabs(got - ref) > maxabs ? fabs(got - ref) : maxabs;
        }
    }
    const double rel = sqrt(num / (den + 1e-300));
    int fb = 0; CK(hipMemcpy(&fb, dfb, 4, hipMemcpyDeviceToHost));

#ifdef XT_TIMING
    {   // s_memtime stamps of the steady-state loop: per wave (loop ticks, ticks spent in its barriers incl. the DMA drain in front of them, tiles)
        const long long nwg = (long long)((Lq + 255) / 256) * H * n_inner * n_outer;
        long long* ddbg; CK(hipMalloc(&ddbg, nwg * 64 * 8)); CK(hipMemset(ddbg, 0, nwg * 64 * 8));
        g_xt_dbg = ddbg;
        (void)gvf_attn_tiled_fwd_bf16(dq, dkt, dvt, dout, n_outer, n_inner, Lq, Lk, H, qs, qs, shared_kv ? 1 : n_inner, shared_kv ? 0 : 1, nullptr, 0, force_exact, dfb, nullptr);
        CK(hipDeviceSynchronize());
        g_xt_dbg = nullptr;
        std::vector<long long> hd(nwg * 64);
        CK(hipMemcpy(hd.data(), ddbg, nwg * 64 * 8, hipMemcpyDeviceToHost));
        double loop = 0, bar = 0, tiles = 0, pre = 0, post = 0; long long nw = 0;
        for (long long i = 0; i < nwg * 4; ++i) if (hd[i * 4 + 2] > 0) { loop += hd[i * 4]; bar += hd[i * 4 + 1]; tiles += hd[i * 4 + 2]; pre += hd[i * 4 + 3]; post += hd[(nwg * 4 + i) * 4]; ++nw; }
        if (nw) printf("    timing (%lld waves): %.0f ticks per tile in the steady-state loop, of which %.0f (%.1f %%) in its barriers; per workgroup: %.0f ticks before the loop "
                       "(queries, first stages, first phases), %.0f in it (%.0f tiles), %.0f after it (remainder tiles, last phases, guard, stores)\n", nw, loop / tiles, bar / tiles,
                       100.0 * bar / loop, pre / nw, loop / nw, tiles / nw, post / nw);
        {   // persistent workgroups: the first item boundary of every wave that had one (ticks after the first item's last phase)
            const long long grid = nwg < 512 ? nwg : 512;
            double acc[8] = {0}; long long n2 = 0;
            for (long long i = 0; i < grid * 4; ++i) {
                const long long* d = &hd[grid * 32 + i * 8];
                if (d[0] == 1) { for (int k = 1; k < 8; ++k) acc[k] += (double)d[k]; ++n2; }
            }
            if (n2) printf("    item boundary (%lld waves): guard barriers passed +%.0f, next item's stages + query rows requested +%.0f, stores issued +%.0f | next item: "
                           "query rows normalised +%.0f, stages landed (barrier) +%.0f, steady loop entered +%.0f, its last phase done +%.0f\n", n2, acc[1] / n2, acc[2] / n2,
                           acc[3] / n2, acc[4] / n2, acc[5] / n2, acc[6] / n2, acc[7] / n2);
        }
        (void)hipFree(ddbg);
    }
#endif
    hipEvent_t e0, e1; CK(hipEventCreate(&e0)); CK(hipEventCreate(&e1));
    for (int i = 0; i < 3; ++i) (void)gvf_attn_tiled_fwd_bf16(dq, dkt, dvt, dout, n_outer, n_inner, Lq, Lk, H, qs, qs, shared_kv ? 1 : n_inner, shared_kv ? 0 : 1, nullptr, 0, force_exact, dfb, nullptr);
    CK(hipEventRecord(e0));
    for (int i = 0; i < iters; ++i) (void)gvf_attn_tiled_fwd_bf16(dq, dkt, dvt, dout, n_outer, n_inner, Lq, Lk, H, qs, qs, shared_kv ? 1 : n_inner, shared_kv ? 0 : 1, nullptr, 0, force_exact, dfb, nullptr);
    CK(hipEventRecord(e1)); CK(hipDeviceSynchronize());
    float ms; CK(hipEventElapsedTime(&ms, e0, e1));
    const double us = ms * 1e3 / iters, tf = 4.0 * M * Lk * C / us / 1e6;
    printf("%-34s exact=%d gain=%5.1f : rel_l2 %.3e max_abs %.3e nan %d fallback_wgs %d | %8.1f us  %7.1f TFLOP/s (%.1f%% of 2.5 PF)\n", name, force_exact, k_gain, rel, maxabs,
           nan_count, fb, us, tf, tf / 25.0);
    (void)hipFree(dq); (void)hipFree(dout); (void)hipFree(dkv); (void)hipFree(dkt); (void)hipFree(dvt);
    return (rel < 1e-2 && nan_count == 0) ? 0 : 2;
}

int main(int argc, char** argv) {
    int bad = 0;
    const int iters = argc > 1 ? atoi(argv[1]) : 20;
    bad |= run_case("static cross B1 T24 Lk4096", 1, 24, 512, 4096, 16, true, 1.f, 0, iters);
    if (argc > 2) {                // timing-only runs (ablations): the three DiT shapes
        bad |= run_case("image cross  B1 T24 Lk1370", 1, 24, 512, 1370, 16, false, 1.f, 0, iters);
        bad |= run_case("spatial self B1 T24 Lk512 ", 24, 1, 512, 512, 16, false, 1.f, 0, iters);
        return bad;
    }
    bad |= run_case("static cross B1 T24 Lk4096", 1, 24, 512, 4096, 16, true, 1.f, 1, iters);
    bad |= run_case("image cross  B1 T24 Lk1370", 1, 24, 512, 1370, 16, false, 1.f, 0, iters);
    bad |= run_case("static cross B3 T24 Lk4096", 3, 24, 512, 4096, 16, true, 1.f, 0, iters);
    // range guard: logits far outside +-100 octaves on some rows -> exact fallback must kick in and stay accurate
    bad |= run_case("static cross, k x40 (fallback)", 1, 4, 512, 1000, 16, true, 40.f, 0, 3);
    bad |= run_case("ragged Lq 300 Lk 70", 2, 3, 300, 70, 4, false, 1.f, 0, 3);
    printf(bad ? "FAILED\n" : "ALL OK\n");
    return bad;
}
