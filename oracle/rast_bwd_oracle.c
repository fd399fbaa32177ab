/*
 * rast_bwd_oracle.c -- CPU restatement (plain C, DOUBLE precision) of the 3D-Gaussian-splatting rasteriser's
 * forward AND backward pass: the checker of gvf_rast_backward() (csrc/rast_bwd.hip).
 *
 * TEST INFRASTRUCTURE ONLY.  Nothing under gvfdiffusion_amd/ may import, link or call this file.
 *
 * PARITY STATUS: "parity unpinned" against the reference -- the operator's backward lives in the same two
 * third-party CUDA packages as its forward (see rast_oracle.c; setup.sh:111,220-227), absent from /root/reference,
 * which holds no gradient test for them.  The anchor is the reference's use of the operator as a differentiable
 * one: renderers/gaussian_render.py:198-220 (autograd through GaussianRasterizer), train_vae.py:321-352 (render
 * loss back-propagated into the Gaussians).  What pins THIS file is mathematics: tests/test_oracle_rast_bwd.py
 * checks every returned gradient against central finite differences of gvfo64_forward() below (double precision,
 * so the comparison is tight), and gvfo64_forward() against the float forward oracle (rast_oracle.c).
 *
 * Conventions taken over from the published upstream backward (3DGS backward.cu; they matter for parity of the
 * numbers a training run sees, and are the only places where the returned gradient is not the exact derivative):
 *   - alpha = min(0.99, opacity * G): the gradient passes THROUGH the clamp (treated as identity);
 *   - the view-space position (tx, ty) used in the EWA Jacobian is clamped to 1.3 tan(fov) * tz: a clamped
 *     coordinate gets no gradient, and the dependence of the clamp bound on tz is ignored;
 *   - the gradient of the screen-space mean is reported in NDC units (d/d(ndc) = d/d(pixel) * 0.5 * W resp. H),
 *     the quantity `screenspace_points.grad` holds upstream.
 * The backward is exported in its two stages, split at the accumulators: gvfo64_accumulators() (the blend's backward) and gvfo64_chain()
 * (the per-Gaussian chain rule, linear in the accumulators); gvfo64_backward() is their composition.  gvfo64_project() is the per-Gaussian
 * forward whose derivative the chain rule is.  tests/test_rast_bwd_conformance_gpu.py holds the device against each stage separately.
 * gvfo64_blend() is the forward's compositing alone, over given records and given per-tile lists: with gvfo64_project() the reference of the
 * forward's stage-wise conformance (tests/test_rast_fwd_conformance_gpu.py); its fp32 build has two forms, upstream's and the device's.
 * mip mode: the opacity compensation coef = sqrt(det0 / (det1 + 1e-6) + 1e-6) is differentiated exactly.
 */
#include <stdint.h>
#include <stdlib.h>
#include <string.h>
#include <tgmath.h>

/* One source, two builds.  Default: real = double, symbols gvfo64_* (the reference).  -DGVFO_F32 (with -fsingle-precision-constant and
 * -ffp-contract=off): real = float, every operation and constant rounded to single precision, symbols gvfo32_* -- the "fp32 yardstick",
 * the same formulas as a naive single-precision composition (what a correct fp32 kernel may be expected to reach).  tgmath.h picks
 * sqrtf / expf / ... from the operand type.  -DGVFO_MUTANTS (yardstick build only): a test-only switch that breaks one line of the chain
 * rule, or one decision of the blend, at a time, so that tests/test_rast_bwd_ref.py and tests/test_rast_fwd_ref.py can show that the
 * conformance bars catch each of them. */
#ifdef GVFO_F32
typedef float real;
#define SYM(n) gvfo32_##n
#else
typedef double real;
#define SYM(n) gvfo64_##n
#endif

#ifdef GVFO_MUTANTS
static int g_mutant = 0;
void SYM(set_mutant)(int m) { g_mutant = m; }
#define MUT(k) (g_mutant == (k))
#else
#define MUT(k) 0
#endif
/* mutants: 1 SH view-direction term of means3D dropped; 2 db[6][2] 4z -> 2z; 3 tx, ty terms of dtz dropped; 4 clamp multipliers ignored;
 * 5 depth path, y component dropped; 6 mip coefficient, dd1 term dropped; 7 first sign of gq[0] flipped;
 * blend(): 8 skip threshold 1/256 for 1/255; 9 alpha clamp 0.995 for 0.99; 10 the T-stop applied after compositing the splat instead of in
 * front of it; 11 every exp result times (1 + 3e-6) */

#define TILE 16
#define MODE_MIP 0
#define MODE_DILATE 1

static const real SH_C0 = 0.28209479177387814;
static const real SH_C1 = 0.4886025119029199;
static const real SH_C2[5] = {1.0925484305920792, -1.0925484305920792, 0.31539156525252005, -1.0925484305920792,
                                0.5462742152960396};
static const real SH_C3[7] = {-0.5900435899266435, 2.890611442640554, -0.4570457994644658, 0.3731763325901154,
                                -0.4570457994644658, 1.445305721320277, -0.5900435899266435};

typedef struct {
    int visible;
    real depth, x, y, ca, cb, cc, op, rgb[3];
    int x0, y0, x1, y1;
    /* intermediates kept for the backward pass */
    real pv[3], c6[6], A0[3], A1[3], cxx, cxy, cyy; /* cxx.. BEFORE the filter */
    real coef, tx, ty, tz, xmul, ymul, pw, ph[4];
    int clamped[3];
    int rad, flag;            /* integer 3-sigma radius; FLAG_* bits below */
    real dir[3], dlen;
} G64;

typedef struct {
    int P, M, deg, H, W, mode;
    const real *means3D, *shs, *colors_precomp, *opac, *scales, *rots, *cov3D;
    real tanfovx, tanfovy, kernel_size, scale_mod;
    const real *view, *proj, *campos, *bg;
    const real* txty_fixed;   /* project() only: clamped view coordinates held at these values (the "no gradient" convention) */
} Scene;

static void cov3d(const real* s, real mod, const real* q, real* c6) {
    real sx = mod * s[0], sy = mod * s[1], sz = mod * s[2];
    real r = q[0], x = q[1], y = q[2], z = q[3];
    real R[3][3] = {{1 - 2 * (y * y + z * z), 2 * (x * y - r * z), 2 * (x * z + r * y)},
                      {2 * (x * y + r * z), 1 - 2 * (x * x + z * z), 2 * (y * z - r * x)},
                      {2 * (x * z - r * y), 2 * (y * z + r * x), 1 - 2 * (x * x + y * y)}};
    real sc[3] = {sx, sy, sz}, L[3][3];
    for (int i = 0; i < 3; ++i) for (int j = 0; j < 3; ++j) L[i][j] = R[i][j] * sc[j];
    real S[3][3];
    for (int i = 0; i < 3; ++i) for (int j = 0; j < 3; ++j) {
        S[i][j] = 0;
        for (int k = 0; k < 3; ++k) S[i][j] += L[i][k] * L[j][k];
    }
    c6[0] = S[0][0]; c6[1] = S[0][1]; c6[2] = S[0][2]; c6[3] = S[1][1]; c6[4] = S[1][2]; c6[5] = S[2][2];
}

/* SH basis values b[16] for direction (x,y,z) */
static void sh_basis(int deg, real x, real y, real z, real* b) {
    b[0] = SH_C0;
    if (deg > 0) {
        b[1] = -SH_C1 * y; b[2] = SH_C1 * z; b[3] = -SH_C1 * x;
        if (deg > 1) {
            real xx = x * x, yy = y * y, zz = z * z, xy = x * y, yz = y * z, xz = x * z;
            b[4] = SH_C2[0] * xy; b[5] = SH_C2[1] * yz; b[6] = SH_C2[2] * (2 * zz - xx - yy); b[7] = SH_C2[3] * xz;
            b[8] = SH_C2[4] * (xx - yy);
            if (deg > 2) {
                b[9] = SH_C3[0] * y * (3 * xx - yy); b[10] = SH_C3[1] * xy * z; b[11] = SH_C3[2] * y * (4 * zz - xx - yy);
                b[12] = SH_C3[3] * z * (2 * zz - 3 * xx - 3 * yy); b[13] = SH_C3[4] * x * (4 * zz - xx - yy);
                b[14] = SH_C3[5] * z * (xx - yy); b[15] = SH_C3[6] * x * (xx - 3 * yy);
            }
        }
    }
}
/* d basis / d(x,y,z): db[k][3] */
static void sh_basis_grad(int deg, real x, real y, real z, real db[16][3]) {
    memset(db, 0, sizeof(real) * 48);
    if (deg > 0) {
        db[1][1] = -SH_C1; db[2][2] = SH_C1; db[3][0] = -SH_C1;
        if (deg > 1) {
            db[4][0] = SH_C2[0] * y; db[4][1] = SH_C2[0] * x;
            db[5][1] = SH_C2[1] * z; db[5][2] = SH_C2[1] * y;
            db[6][0] = SH_C2[2] * -2 * x; db[6][1] = SH_C2[2] * -2 * y; db[6][2] = SH_C2[2] * (MUT(2) ? 2 : 4) * z;
            db[7][0] = SH_C2[3] * z; db[7][2] = SH_C2[3] * x;
            db[8][0] = SH_C2[4] * 2 * x; db[8][1] = SH_C2[4] * -2 * y;
            if (deg > 2) {
                real xx = x * x, yy = y * y, zz = z * z;
                db[9][0] = SH_C3[0] * 6 * x * y; db[9][1] = SH_C3[0] * (3 * xx - 3 * yy);
                db[10][0] = SH_C3[1] * y * z; db[10][1] = SH_C3[1] * x * z; db[10][2] = SH_C3[1] * x * y;
                db[11][0] = SH_C3[2] * -2 * x * y; db[11][1] = SH_C3[2] * (4 * zz - xx - 3 * yy); db[11][2] = SH_C3[2] * 8 * y * z;
                db[12][0] = SH_C3[3] * -6 * x * z; db[12][1] = SH_C3[3] * -6 * y * z; db[12][2] = SH_C3[3] * (6 * zz - 3 * xx - 3 * yy);
                db[13][0] = SH_C3[4] * (4 * zz - 3 * xx - yy); db[13][1] = SH_C3[4] * -2 * x * y; db[13][2] = SH_C3[4] * 8 * x * z;
                db[14][0] = SH_C3[5] * 2 * x * z; db[14][1] = SH_C3[5] * -2 * y * z; db[14][2] = SH_C3[5] * (xx - yy);
                db[15][0] = SH_C3[6] * (3 * xx - 3 * yy); db[15][1] = SH_C3[6] * -6 * x * y;
            }
        }
    }
}

/* per-Gaussian flag byte of chain() / project() */
#define FLAG_NEAR    1   /* an input comparison of the chain rule sits within 1e-5 (relative) of its threshold: pv.z vs 0.2, |tx/tz| or |ty/tz| vs
                            1.3 tan(fov), an rgb channel vs the 0 clamp, mip det0 / det1 vs 1e-6 */
#define FLAG_CLAMPED 2   /* visible, and tx or ty is clamped (xmul or ymul is 0) */
#define FLAG_VISIBLE 4
static int near_thr(real v, real thr) { return fabs(v - thr) <= (real)1e-5 * fabs(thr); }

static int imin(int a, int b) { return a < b ? a : b; }
static int imax(int a, int b) { return a > b ? a : b; }

static void pre_one(const Scene* s, int i, G64* g) {
    memset(g, 0, sizeof(*g));
    const real* p = s->means3D + 3 * (size_t)i;
    const real* m = s->view;
    g->pv[0] = m[0] * p[0] + m[4] * p[1] + m[8] * p[2] + m[12];
    g->pv[1] = m[1] * p[0] + m[5] * p[1] + m[9] * p[2] + m[13];
    g->pv[2] = m[2] * p[0] + m[6] * p[1] + m[10] * p[2] + m[14];
    if (near_thr(g->pv[2], 0.2)) g->flag |= FLAG_NEAR;
    if (g->pv[2] <= 0.2) return;
    m = s->proj;
    for (int k = 0; k < 4; ++k) g->ph[k] = m[k] * p[0] + m[4 + k] * p[1] + m[8 + k] * p[2] + m[12 + k];
    g->pw = 1.0 / (g->ph[3] + 0.0000001);
    real projx = g->ph[0] * g->pw, projy = g->ph[1] * g->pw;
    if (s->cov3D) memcpy(g->c6, s->cov3D + 6 * (size_t)i, 6 * sizeof(real));
    else cov3d(s->scales + 3 * (size_t)i, s->scale_mod, s->rots + 4 * (size_t)i, g->c6);
    int H = s->H, W = s->W;
    real fx = (real)W / (2.0 * s->tanfovx), fy = (real)H / (2.0 * s->tanfovy);
    real limx = 1.3 * s->tanfovx, limy = 1.3 * s->tanfovy;
    real txtz = g->pv[0] / g->pv[2], tytz = g->pv[1] / g->pv[2];
    g->xmul = (txtz < -limx || txtz > limx) ? 0.0 : 1.0;
    g->ymul = (tytz < -limy || tytz > limy) ? 0.0 : 1.0;
    if (near_thr(fabs(txtz), limx) || near_thr(fabs(tytz), limy)) g->flag |= FLAG_NEAR;
    g->tx = fmin(limx, fmax(-limx, txtz)) * g->pv[2];
    g->ty = fmin(limy, fmax(-limy, tytz)) * g->pv[2];
    if (s->txty_fixed) {
        if (g->xmul == 0.0) g->tx = s->txty_fixed[2 * (size_t)i];
        if (g->ymul == 0.0) g->ty = s->txty_fixed[2 * (size_t)i + 1];
    }
    g->tz = g->pv[2];
    real J00 = fx / g->tz, J02 = -(fx * g->tx) / (g->tz * g->tz), J11 = fy / g->tz, J12 = -(fy * g->ty) / (g->tz * g->tz);
    for (int c = 0; c < 3; ++c) {
        real w0 = s->view[c * 4 + 0], w1 = s->view[c * 4 + 1], w2 = s->view[c * 4 + 2];
        g->A0[c] = J00 * w0 + J02 * w2;
        g->A1[c] = J11 * w1 + J12 * w2;
    }
    const real* c6 = g->c6;
    real S[3][3] = {{c6[0], c6[1], c6[2]}, {c6[1], c6[3], c6[4]}, {c6[2], c6[4], c6[5]}};
    real B0[3], B1[3];
    for (int c = 0; c < 3; ++c) {
        B0[c] = g->A0[0] * S[0][c] + g->A0[1] * S[1][c] + g->A0[2] * S[2][c];
        B1[c] = g->A1[0] * S[0][c] + g->A1[1] * S[1][c] + g->A1[2] * S[2][c];
    }
    g->cxx = B0[0] * g->A0[0] + B0[1] * g->A0[1] + B0[2] * g->A0[2];
    g->cxy = B0[0] * g->A1[0] + B0[1] * g->A1[1] + B0[2] * g->A1[2];
    g->cyy = B1[0] * g->A1[0] + B1[1] * g->A1[1] + B1[2] * g->A1[2];
    real cxx = g->cxx, cxy = g->cxy, cyy = g->cyy, k = s->mode == MODE_MIP ? s->kernel_size : 0.3;
    g->coef = 1.0;
    if (s->mode == MODE_MIP) {
        if (near_thr(cxx * cyy - cxy * cxy, 1e-6) || near_thr((cxx + k) * (cyy + k) - cxy * cxy, 1e-6)) g->flag |= FLAG_NEAR;
        real det0 = fmax(1e-6, cxx * cyy - cxy * cxy);
        real det1 = fmax(1e-6, (cxx + k) * (cyy + k) - cxy * cxy);
        g->coef = sqrt(det0 / (det1 + 1e-6) + 1e-6);
        if (det0 <= 1e-6 || det1 <= 1e-6) g->coef = 0.0;
    }
    cxx += k; cyy += k;
    real det = cxx * cyy - cxy * cxy;
    if (det == 0.0) return;
    g->ca = cyy / det; g->cb = -cxy / det; g->cc = cxx / det;
    real mid = 0.5 * (cxx + cyy);
    real lam1 = mid + sqrt(fmax(0.1, mid * mid - det)), lam2 = mid - sqrt(fmax(0.1, mid * mid - det));
    real rad = ceil(3.0 * sqrt(fmax(lam1, lam2)));
    g->rad = (int)rad;
    g->x = ((projx + 1.0) * (real)W - 1.0) * 0.5;
    g->y = ((projy + 1.0) * (real)H - 1.0) * 0.5;
    int gx = (W + TILE - 1) / TILE, gy = (H + TILE - 1) / TILE;
    g->x0 = imin(gx, imax(0, (int)((g->x - rad) / (real)TILE)));
    g->y0 = imin(gy, imax(0, (int)((g->y - rad) / (real)TILE)));
    g->x1 = imin(gx, imax(0, (int)((g->x + rad + (real)(TILE - 1)) / (real)TILE)));
    g->y1 = imin(gy, imax(0, (int)((g->y + rad + (real)(TILE - 1)) / (real)TILE)));
    if ((g->x1 - g->x0) * (g->y1 - g->y0) == 0) return;
    if (s->colors_precomp) {
        for (int c = 0; c < 3; ++c) g->rgb[c] = s->colors_precomp[3 * (size_t)i + c];
    } else {
        real d[3] = {p[0] - s->campos[0], p[1] - s->campos[1], p[2] - s->campos[2]};
        g->dlen = sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2]);
        for (int c = 0; c < 3; ++c) g->dir[c] = d[c] / g->dlen;
        real b[16];
        sh_basis(s->deg, g->dir[0], g->dir[1], g->dir[2], b);
        int nb = (s->deg + 1) * (s->deg + 1);
        const real* sh = s->shs + (size_t)i * s->M * 3;
        for (int c = 0; c < 3; ++c) {
            real r = 0, mag = 0.5;
            for (int kk = 0; kk < nb; ++kk) { r += b[kk] * sh[kk * 3 + c]; mag += fabs(b[kk] * sh[kk * 3 + c]); }
            r += 0.5;
            if (fabs(r) <= (real)1e-5 * mag) g->flag |= FLAG_NEAR;
            g->clamped[c] = r < 0.0;
            g->rgb[c] = r < 0.0 ? 0.0 : r;
        }
    }
    g->depth = g->pv[2];
    g->op = s->opac[i] * g->coef;
    g->visible = 1;
    g->flag |= FLAG_VISIBLE | ((g->xmul == 0.0 || g->ymul == 0.0) ? FLAG_CLAMPED : 0);
}

typedef struct { real depth; int id; } DI;
static int di_cmp(const void* a, const void* b) {
    const DI* x = (const DI*)a; const DI* y = (const DI*)b;
    /* the device orders by the float32 depth bits, then by id */
    float fx = (float)x->depth, fy = (float)y->depth;
    if (fx != fy) return fx < fy ? -1 : 1;
    return x->id < y->id ? -1 : (x->id > y->id ? 1 : 0);
}

/* per-pixel ordered candidate list: every visible Gaussian whose 3-sigma tile rect covers the pixel's tile */
static int pixel_list(const G64* g, int P, int px, int py, DI* list) {
    int tx = px / TILE, ty = py / TILE, n = 0;
    for (int i = 0; i < P; ++i)
        if (g[i].visible && tx >= g[i].x0 && tx < g[i].x1 && ty >= g[i].y0 && ty < g[i].y1) { list[n].depth = g[i].depth; list[n].id = i; ++n; }
    qsort(list, (size_t)n, sizeof(DI), di_cmp);
    return n;
}

static void make_scene(Scene* s, int P, int M, int deg, const real* means3D, const real* shs, const real* colors_precomp,
                       const real* opac, const real* scales, const real* rots, const real* cov3D, int H, int W,
                       real tanfovx, real tanfovy, real kernel_size, real scale_mod, int mode, const real* view,
                       const real* proj, const real* campos, const real* bg) {
    s->P = P; s->M = M; s->deg = deg; s->H = H; s->W = W; s->mode = mode;
    s->means3D = means3D; s->shs = shs; s->colors_precomp = colors_precomp; s->opac = opac; s->scales = scales; s->rots = rots;
    s->cov3D = cov3D; s->tanfovx = tanfovx; s->tanfovy = tanfovy; s->kernel_size = kernel_size; s->scale_mod = scale_mod;
    s->view = view; s->proj = proj; s->campos = campos; s->bg = bg; s->txty_fixed = NULL;
}

int SYM(forward)(int P, int M, int deg, const real* means3D, const real* shs, const real* colors_precomp,
                   const real* opac, const real* scales, const real* rots, const real* cov3D, int H, int W,
                   real tanfovx, real tanfovy, real kernel_size, real scale_mod, int mode, const real* view,
                   const real* proj, const real* campos, const real* bg, real* out_color, real* out_alpha,
                   real* out_depth) {
    Scene s;
    make_scene(&s, P, M, deg, means3D, shs, colors_precomp, opac, scales, rots, cov3D, H, W, tanfovx, tanfovy, kernel_size,
               scale_mod, mode, view, proj, campos, bg);
    G64* g = (G64*)malloc(sizeof(G64) * (size_t)(P > 0 ? P : 1));
    DI* list = (DI*)malloc(sizeof(DI) * (size_t)(P > 0 ? P : 1));
    for (int i = 0; i < P; ++i) pre_one(&s, i, &g[i]);
    for (int py = 0; py < H; ++py)
        for (int px = 0; px < W; ++px) {
            int n = pixel_list(g, P, px, py, list);
            real T = 1.0, C[3] = {0, 0, 0}, D = 0;
            for (int k = 0; k < n; ++k) {
                const G64* q = &g[list[k].id];
                real dx = q->x - (real)px, dy = q->y - (real)py;
                real power = -0.5 * (q->ca * dx * dx + q->cc * dy * dy) - q->cb * dx * dy;
                if (power > 0.0) continue;
                real alpha = fmin(0.99, q->op * exp(power));
                if (alpha < 1.0 / 255.0) continue;
                real test_T = T * (1.0 - alpha);
                if (test_T < 0.0001) break;
                for (int c = 0; c < 3; ++c) C[c] += q->rgb[c] * alpha * T;
                D += q->depth * alpha * T;
                T = test_T;
            }
            size_t pid = (size_t)py * W + px;
            for (int c = 0; c < 3; ++c) out_color[(size_t)c * H * W + pid] = C[c] + T * bg[c];
            if (out_alpha) out_alpha[pid] = 1.0 - T;
            if (out_depth) out_depth[pid] = D;
        }
    free(list); free(g);
    return 0;
}

#define SCENE_PARAMS                                                                                                          \
    int P, int M, int deg, const real *means3D, const real *shs, const real *colors_precomp, const real *opac, const real *scales, \
        const real *rots, const real *cov3D, int H, int W, real tanfovx, real tanfovy, real kernel_size, real scale_mod, int mode, \
        const real *view, const real *proj, const real *campos, const real *bg
#define SCENE_ARGS                                                                                                                   \
    P, M, deg, means3D, shs, colors_precomp, opac, scales, rots, cov3D, H, W, tanfovx, tanfovy, kernel_size, scale_mod, mode, view, \
        proj, campos, bg

/* The oracle's per-Gaussian forward: out[P][10] = x, y [pixels], conic a, b, c, opacity_eff, r, g, b, depth -- the quantities the blend
 * reads, in the order of the accumulators; zeros for an invisible Gaussian.  out_flag[P]: FLAG_* bits.  out_txty[P][2] (may be NULL): the
 * view coordinates after the clamp.  txty_fixed (may be NULL): clamped coordinates are held at these values instead of 1.3 tan(fov) tz,
 * which is the function whose derivative the chain rule reports ("a clamped coordinate gets no gradient"). */
int SYM(project)(SCENE_PARAMS, const real* txty_fixed, real* out, uint8_t* out_flag, real* out_txty) {
    Scene s;
    make_scene(&s, SCENE_ARGS);
    s.txty_fixed = txty_fixed;
    for (int i = 0; i < P; ++i) {
        G64 g;
        pre_one(&s, i, &g);
        real* o = out + 10 * (size_t)i;
        for (int k = 0; k < 10; ++k) o[k] = 0;
        if (g.visible) {
            o[0] = g.x; o[1] = g.y; o[2] = g.ca; o[3] = g.cb; o[4] = g.cc; o[5] = g.op;
            o[6] = g.rgb[0]; o[7] = g.rgb[1]; o[8] = g.rgb[2]; o[9] = g.depth;
        }
        if (out_flag) out_flag[i] = (uint8_t)g.flag;
        if (out_txty) { out_txty[2 * (size_t)i] = g.tx; out_txty[2 * (size_t)i + 1] = g.ty; }
    }
    return 0;
}

/* The blend on its own: the compositing of given per-Gaussian records over given per-tile lists -- the checker of the forward's blend
 * (tests/test_rast_fwd_conformance_gpu.py), separated from the projection and from the binning.
 *   rec[P][10]        the records in the order project() emits them: x, y [pixels], conic a, b, c, opacity_eff, r, g, b, depth
 *   ranges, ids       per tile t (row-major over the ceil(W/16) x ceil(H/16) grid) the list ids[ranges[t][0] .. ranges[t][1]), composited in
 *                     the order given.  ranges == NULL ("lists = NULL"): the function builds the lists itself from rects[P][4] = x0, y0, x1, y1
 *                     (tiles; an empty rect = an invisible Gaussian), sorted by fp32 depth bits, then id, as pixel_list() does
 *   subpixel_offset   [H*W][2] or NULL
 *   form              fp32 build only (the fp64 build ignores it).  0: upstream's expression, power = -0.5 (a dx^2 + c dy^2) - b dx dy,
 *                     alpha = op * expf(power).  1: the algorithm the device is documented to run (csrc/rast_common.h splat_cholesky /
 *                     splat_neg_exponent), in plain C with libm: the conic pre-scaled by CONIC_K1 / CONIC_K2, its Cholesky factor
 *                     in tile-relative coordinates, s1, s2 by fma, alpha = exp2(log2(op) - s1^2 - s2^2), a conic that is not positive definite
 *                     dropped, T - alpha T for T (1 - alpha), the sums by fma
 * Outputs (each may be NULL): color[3][H][W], alpha[H][W], depth[H][W]; the scales of their rounding error s_color[3][H][W] = sum rgb_c alpha T +
 * T_final bg_c, s_alpha = sum alpha T, s_depth = sum depth alpha T (absolute values throughout); flags[H][W], the PFLAG_* bits of the decisions
 * that sit at a threshold; power[(ranges[t][0] + k) * 256 + ly * 16 + lx] (explicit lists only): the exponent, in octaves (log2 G), of
 * entry k of tile t's list at the tile's pixel (lx, ly), zero outside the image -- what DESIGN's accuracy claim for the Cholesky form is
 * checked on.  Mutants 8 .. 11 (yardstick build only) break one blend decision each. */
#define PFLAG_ALPHA 1   /* an alpha within 2e-4 (relative) of the 1/255 skip threshold */
#define PFLAG_T     2   /* a test_T within 2e-4 (relative) of the 1e-4 termination threshold */
#define PFLAG_POWER 4   /* a power within 1e-6 of 0 */
#define PFLAG_CLAMP 8   /* an opacity * G within 2e-4 (relative) of the 0.99 clamp */

#ifdef GVFO_F32
typedef struct { float l11, l12, l22, c1, c2, lo; } Chol;
/* splat_cholesky + the staged log2(opacity) of csrc/rast_blend.hip, with libm where the device has hardware instructions */
static Chol chol_of(const float* r, float tile_x0, float tile_y0) {
    const float K1 = -0.7213475204444817f, K2 = -1.4426950408889634f;   /* CONIC_K1 = -0.5 log2(e), CONIC_K2 = -log2(e) */
    const float ap = r[2] * K1, bp = r[3] * K2, cp = r[4] * K1;          /* the record's a', b', c' */
    const float m11 = -ap, m12 = -0.5f * bp, m22 = -cp;
    const float il = 1.0f / sqrtf(m11);
    Chol c;
    c.l11 = m11 * il;
    c.l12 = m12 * il;
    const float d = m22 - c.l12 * c.l12;
    c.l22 = sqrtf(d);
    const int ok = m11 > 0.0f && d > 0.0f && m11 < INFINITY && d < INFINITY;
    if (!ok) { c.l11 = 0.0f; c.l12 = 0.0f; c.l22 = 0.0f; }
    const float xr = r[0] - tile_x0, yr = r[1] - tile_y0;
    c.c1 = ok ? fmaf(c.l11, xr, c.l12 * yr) : 0.0f;
    c.c2 = ok ? c.l22 * yr : 0.0f;
    c.lo = ok ? log2f(r[5]) : -INFINITY;
    return c;
}
#endif

int SYM(blend)(int P, const real* rec, const int32_t* ranges, const int32_t* ids, const int32_t* rects, const real* subpixel_offset,
               const real* bg, int H, int W, int form, real* out_color, real* out_alpha, real* out_depth, real* s_color, real* s_alpha,
               real* s_depth, uint8_t* out_flags, real* out_power) {
    const int gx = (W + TILE - 1) / TILE, gy = (H + TILE - 1) / TILE;
    const real thr = MUT(8) ? 1.0 / 256.0 : 1.0 / 255.0, clampv = MUT(9) ? 0.995 : 0.99, expmul = MUT(11) ? 1.0 + 3e-6 : 1.0;
    DI* built = ranges ? NULL : (DI*)malloc(sizeof(DI) * (size_t)(P > 0 ? P : 1));
#ifdef GVFO_F32
    int longest = P > 0 ? P : 1;                    /* (a given list may hold duplicates: it is what is being checked) */
    if (ranges) for (int t = 0; t < gx * gy; ++t) if (ranges[2 * t + 1] - ranges[2 * t] > longest) longest = ranges[2 * t + 1] - ranges[2 * t];
    Chol* ch = (Chol*)malloc(sizeof(Chol) * (size_t)longest);
#else
    (void)form;
#endif
    for (int ty = 0; ty < gy; ++ty)
        for (int tx = 0; tx < gx; ++tx) {
            const int t = ty * gx + tx;
            int n = 0, first = 0;
            if (ranges) { first = ranges[2 * t]; n = ranges[2 * t + 1] - first; }
            else {
                for (int i = 0; i < P; ++i) {
                    const int32_t* r = rects + 4 * (size_t)i;
                    if (tx >= r[0] && tx < r[2] && ty >= r[1] && ty < r[3]) { built[n].depth = rec[10 * (size_t)i + 9]; built[n].id = i; ++n; }
                }
                qsort(built, (size_t)n, sizeof(DI), di_cmp);
            }
#define ENTRY(k) (ranges ? (int)ids[first + (k)] : built[k].id)
#ifdef GVFO_F32
            if (form == 1) for (int k = 0; k < n; ++k) ch[k] = chol_of(rec + 10 * (size_t)ENTRY(k), (float)(tx * TILE), (float)(ty * TILE));
#endif
            for (int ly = 0; ly < TILE; ++ly)
                for (int lx = 0; lx < TILE; ++lx) {
                    const int px = tx * TILE + lx, py = ty * TILE + ly;
                    if (px >= W || py >= H) {
                        if (out_power && ranges) for (int k = 0; k < n; ++k) out_power[(size_t)(first + k) * 256 + ly * TILE + lx] = 0;
                        continue;
                    }
                    const size_t pid = (size_t)py * W + px;
                    real pxf = (real)px, pyf = (real)py;
                    if (subpixel_offset) { pxf += subpixel_offset[2 * pid]; pyf += subpixel_offset[2 * pid + 1]; }
                    real T = 1.0, C[3] = {0, 0, 0}, D = 0, SC[3] = {0, 0, 0}, SA = 0, SD = 0;
                    int fl = 0, stopped = 0;
                    for (int k = 0; k < n; ++k) {
                        const real* q = rec + 10 * (size_t)ENTRY(k);
                        real power_oct, araw;          /* log2 G, opacity * G */
                        int skip = 0;
#ifdef GVFO_F32
                        if (form == 1) {
                            const Chol* c = &ch[k];
                            const float pxr = pxf - (float)(tx * TILE), pyr = pyf - (float)(ty * TILE);
                            const float s1 = fmaf(-c->l11, pxr, fmaf(-c->l12, pyr, c->c1));
                            const float s2 = fmaf(-c->l22, pyr, c->c2);
                            power_oct = -fmaf(s2, s2, s1 * s1);
                            araw = exp2f(-fmaf(s2, s2, fmaf(s1, s1, -c->lo))) * expmul;
                        } else
#endif
                        {
                            const real dx = q[0] - pxf, dy = q[1] - pyf;
                            const real power = -0.5 * (q[2] * dx * dx + q[4] * dy * dy) - q[3] * dx * dy;
                            power_oct = power * (real)1.4426950408889634;
                            skip = power > 0.0;
                            araw = q[5] * (exp(power) * expmul);
                        }
                        if (out_power && ranges) out_power[(size_t)(first + k) * 256 + ly * TILE + lx] = power_oct;
                        if (stopped) continue;         /* (the exponents of the whole list are reported) */
                        if (fabs(power_oct) < (real)1e-6) fl |= PFLAG_POWER;
                        if (skip) continue;
                        if (fabs(araw - (real)(1.0 / 255.0)) < (real)2e-4 * (real)(1.0 / 255.0)) fl |= PFLAG_ALPHA;
                        if (fabs(araw - (real)0.99) < (real)2e-4 * (real)0.99) fl |= PFLAG_CLAMP;
                        const real alpha = fmin(clampv, araw);
                        if (alpha < thr) continue;
                        real w = alpha * T, test_T;
#ifdef GVFO_F32
                        if (form == 1) test_T = T - w; else
#endif
                            test_T = T * ((real)1.0 - alpha);
                        if (fabs(test_T - (real)0.0001) < (real)2e-4 * (real)0.0001) fl |= PFLAG_T;
                        if (test_T < (real)0.0001) { stopped = 1; if (!MUT(10)) continue; }
#ifdef GVFO_F32
                        if (form == 1) {
                            for (int c = 0; c < 3; ++c) C[c] = fmaf(q[6 + c], w, C[c]);
                            D = fmaf(q[9], w, D);
                        } else
#endif
                        {
                            for (int c = 0; c < 3; ++c) C[c] += q[6 + c] * alpha * T;
                            D += q[9] * alpha * T;
                        }
                        for (int c = 0; c < 3; ++c) SC[c] += fabs(q[6 + c]) * w;
                        SA += w; SD += fabs(q[9]) * w;
                        T = test_T;
                    }
                    const size_t hw = (size_t)H * W;
                    for (int c = 0; c < 3; ++c) {
#ifdef GVFO_F32
                        if (out_color) out_color[c * hw + pid] = form == 1 ? fmaf(T, bg[c], C[c]) : C[c] + T * bg[c];
#else
                        if (out_color) out_color[c * hw + pid] = C[c] + T * bg[c];
#endif
                        if (s_color) s_color[c * hw + pid] = SC[c] + T * fabs(bg[c]);
                    }
                    if (out_alpha) out_alpha[pid] = (real)1.0 - T;
                    if (out_depth) out_depth[pid] = D;
                    if (s_alpha) s_alpha[pid] = SA;
                    if (s_depth) s_depth[pid] = SD;
                    if (out_flags) out_flags[pid] = (uint8_t)fl;
                }
#undef ENTRY
        }
#ifdef GVFO_F32
    free(ch);
#endif
    free(built);
    return 0;
}

/* Stage 1, the blend's backward.  acc[P][10] = d/d(x, y) [pixels], d/d(conic a, b, c), d/d(opacity_eff), d/d(r, g, b), d/d(depth) of
 * L = sum(dL_dcolor * color) + sum(dL_dalpha * alpha) + sum(dL_ddepth * depth): the convention of the device's BWD_ACC.  acc_abs (may be
 * NULL): the same sums with every per-(pixel, splat) term replaced by its absolute value (the scale of the rounding error of any
 * summation order).  subpixel_offset[H*W][2] (may be NULL) moves each pixel's sample point.  out_radii[P] (may be NULL): the integer
 * 3-sigma radius of a visible Gaussian, else 0; out_rects[P][4] (may be NULL): its tile rectangle x0, y0, x1, y1. */
int SYM(accumulators)(SCENE_PARAMS, const real* subpixel_offset, const real* dL_dcolor, const real* dL_dalpha, const real* dL_ddepth,
                      real* acc, real* acc_abs, int32_t* out_radii, int32_t* out_rects) {
    Scene s;
    make_scene(&s, SCENE_ARGS);
    size_t Pn = (size_t)(P > 0 ? P : 1);
    G64* g = (G64*)malloc(sizeof(G64) * Pn);
    DI* list = (DI*)malloc(sizeof(DI) * Pn);
    real* alphas = (real*)malloc(sizeof(real) * Pn);
    real* Gs = (real*)malloc(sizeof(real) * Pn);
    int* used = (int*)malloc(sizeof(int) * Pn);
    memset(acc, 0, sizeof(real) * 10 * (size_t)P);
    if (acc_abs) memset(acc_abs, 0, sizeof(real) * 10 * (size_t)P);
    for (int i = 0; i < P; ++i) {
        pre_one(&s, i, &g[i]);
        if (out_radii) out_radii[i] = g[i].visible ? g[i].rad : 0;
        if (out_rects) {
            int32_t* r = out_rects + 4 * (size_t)i;
            r[0] = g[i].visible ? g[i].x0 : 0; r[1] = g[i].visible ? g[i].y0 : 0;
            r[2] = g[i].visible ? g[i].x1 : 0; r[3] = g[i].visible ? g[i].y1 : 0;
        }
    }
    for (int py = 0; py < H; ++py)
        for (int px = 0; px < W; ++px) {
            int n = pixel_list(g, P, px, py, list);
            size_t pid = (size_t)py * W + px;
            real pxf = (real)px, pyf = (real)py;
            if (subpixel_offset) { pxf += subpixel_offset[2 * pid]; pyf += subpixel_offset[2 * pid + 1]; }
            /* channels: r, g, b, depth, one (alpha_out = sum alpha_k T_k) with backgrounds bg, 0, 0 */
            real dch[5] = {dL_dcolor[pid], dL_dcolor[(size_t)H * W + pid], dL_dcolor[(size_t)2 * H * W + pid],
                           dL_ddepth ? dL_ddepth[pid] : (real)0.0, dL_dalpha ? dL_dalpha[pid] : (real)0.0};
            real bgc[5] = {bg[0], bg[1], bg[2], 0.0, 0.0};
            /* forward replay */
            real T = 1.0;
            int m = 0;
            for (int k = 0; k < n; ++k) {
                const G64* q = &g[list[k].id];
                real dx = q->x - pxf, dy = q->y - pyf;
                real power = -0.5 * (q->ca * dx * dx + q->cc * dy * dy) - q->cb * dx * dy;
                if (power > 0.0) continue;
                real Gv = exp(power);
                real alpha = fmin(0.99, q->op * Gv);
                if (alpha < 1.0 / 255.0) continue;
                real test_T = T * (1.0 - alpha);
                if (test_T < 0.0001) break;
                used[m] = list[k].id; alphas[m] = alpha; Gs[m] = Gv; ++m;
                T = test_T;
            }
            const real T_final = T;
            /* back to front.  suffix[ch] = sum_{j>k} c_j alpha_j T_j + T_final bg  (what lies behind splat k) */
            real suffix[5];
            for (int ch = 0; ch < 5; ++ch) suffix[ch] = T_final * bgc[ch];
            for (int k = m - 1; k >= 0; --k) {
                const int id = used[k];
                const G64* q = &g[id];
                const real alpha = alphas[k];
                T = T / (1.0 - alpha);                 /* transmittance in front of splat k */
                real cch[5] = {q->rgb[0], q->rgb[1], q->rgb[2], q->depth, 1.0};
                real dL_dalpha_k = 0.0, abs_dalpha_k = 0.0;
                for (int ch = 0; ch < 5; ++ch) {
                    /* out = ... + c_k alpha T + (1 - alpha) * [behind / (1 - alpha)] : d out / d alpha = c_k T - suffix / (1 - alpha) */
                    dL_dalpha_k += (cch[ch] * T - suffix[ch] / (1.0 - alpha)) * dch[ch];
                    if (acc_abs) abs_dalpha_k += (fabs(cch[ch] * T) + fabs(suffix[ch] / (1.0 - alpha))) * fabs(dch[ch]);
                    suffix[ch] += cch[ch] * alpha * T;
                }
                real* a = acc + 10 * (size_t)id;
                for (int c = 0; c < 3; ++c) a[6 + c] += alpha * T * dch[c];
                a[9] += alpha * T * dch[3];
                /* alpha = min(0.99, op G): gradient passes through the clamp (upstream) */
                const real Gv = Gs[k];
                const real dL_dG = q->op * dL_dalpha_k;
                a[5] += Gv * dL_dalpha_k;
                const real dx = q->x - pxf, dy = q->y - pyf;
                /* power = -0.5 (A dx^2 + C dy^2) - B dx dy */
                a[0] += dL_dG * Gv * (-q->ca * dx - q->cb * dy);
                a[1] += dL_dG * Gv * (-q->cc * dy - q->cb * dx);
                a[2] += dL_dG * Gv * (-0.5 * dx * dx);
                a[3] += dL_dG * Gv * (-dx * dy);
                a[4] += dL_dG * Gv * (-0.5 * dy * dy);
                if (acc_abs) {
                    real* b = acc_abs + 10 * (size_t)id;
                    const real aG = fabs(q->op) * abs_dalpha_k * Gv;
                    for (int c = 0; c < 3; ++c) b[6 + c] += fabs(alpha * T * dch[c]);
                    b[9] += fabs(alpha * T * dch[3]);
                    b[5] += Gv * abs_dalpha_k;
                    b[0] += aG * (fabs(q->ca * dx) + fabs(q->cb * dy));
                    b[1] += aG * (fabs(q->cc * dy) + fabs(q->cb * dx));
                    b[2] += aG * (0.5 * dx * dx);
                    b[3] += aG * fabs(dx * dy);
                    b[4] += aG * (0.5 * dy * dy);
                }
            }
        }
    free(used); free(Gs); free(alphas); free(list); free(g);
    return 0;
}

/* Stage 2, the per-Gaussian chain rule: the gradients gvfo64_backward() returns, from the accumulators it is given.  Linear in acc_in.
 * Outputs may be NULL.  g_means2D[P][2]: NDC convention (see header).  out_flag[P] (may be NULL): FLAG_* bits. */
int SYM(chain)(SCENE_PARAMS, const real* acc_in, real* g_means3D, real* g_means2D, real* g_shs, real* g_colors, real* g_opac,
               real* g_scales, real* g_rots, real* g_cov3D, uint8_t* out_flag) {
    Scene s;
    make_scene(&s, SCENE_ARGS);
    for (int i = 0; i < P; ++i) {
        G64 gi;
        pre_one(&s, i, &gi);
        const G64* q = &gi;
        if (out_flag) out_flag[i] = (uint8_t)gi.flag;
        const real* a = acc_in + 10 * (size_t)i;
        real gm[3] = {0, 0, 0}, gsc[3] = {0, 0, 0}, gq[4] = {0, 0, 0, 0}, gc6[6] = {0, 0, 0, 0, 0, 0}, gop = 0, gcol[3] = {0, 0, 0};
        real gm2[2] = {0, 0};
        if (q->visible) {
            const real* p = means3D + 3 * (size_t)i;
            /* screen-space mean: px = ((ndc + 1) W - 1) / 2 */
            gm2[0] = a[0] * 0.5 * (real)W; gm2[1] = a[1] * 0.5 * (real)H;
            {
                const real* m = proj;
                real mw = q->pw;
                real mul1 = q->ph[0] * mw * mw, mul2 = q->ph[1] * mw * mw;
                gm[0] += (m[0] * mw - m[3] * mul1) * gm2[0] + (m[1] * mw - m[3] * mul2) * gm2[1];
                gm[1] += (m[4] * mw - m[7] * mul1) * gm2[0] + (m[5] * mw - m[7] * mul2) * gm2[1];
                gm[2] += (m[8] * mw - m[11] * mul1) * gm2[0] + (m[9] * mw - m[11] * mul2) * gm2[1];
            }
            /* depth output: depth = view row 2 . p */
            gm[0] += view[2] * a[9]; if (!MUT(5)) gm[1] += view[6] * a[9]; gm[2] += view[10] * a[9];
            /* colour */
            if (colors_precomp) {
                for (int c = 0; c < 3; ++c) gcol[c] = a[6 + c];
            } else {
                real b[16], db[16][3];
                sh_basis(deg, q->dir[0], q->dir[1], q->dir[2], b);
                sh_basis_grad(deg, q->dir[0], q->dir[1], q->dir[2], db);
                int nb = (deg + 1) * (deg + 1);
                const real* sh = shs + (size_t)i * M * 3;
                real ddir[3] = {0, 0, 0};
                for (int c = 0; c < 3; ++c) {
                    real gr = q->clamped[c] ? 0.0 : a[6 + c];
                    for (int kk = 0; kk < nb; ++kk) {
                        if (g_shs) g_shs[((size_t)i * M + kk) * 3 + c] = b[kk] * gr;
                        for (int e = 0; e < 3; ++e) ddir[e] += db[kk][e] * sh[kk * 3 + c] * gr;
                    }
                }
                /* dir = d / |d| */
                real dot = ddir[0] * q->dir[0] + ddir[1] * q->dir[1] + ddir[2] * q->dir[2];
                if (!MUT(1)) for (int e = 0; e < 3; ++e) gm[e] += (ddir[e] - q->dir[e] * dot) / q->dlen;
            }
            /* opacity and the mip coefficient */
            gop = a[5] * q->coef;
            real gcxx = 0, gcxy = 0, gcyy = 0;   /* d/d(cov2D before the filter) */
            const real k = mode == MODE_MIP ? kernel_size : 0.3;
            if (mode == MODE_MIP && q->coef > 0.0) {
                real dcoef = a[5] * opac[i];
                real det0 = q->cxx * q->cyy - q->cxy * q->cxy, det1 = (q->cxx + k) * (q->cyy + k) - q->cxy * q->cxy;
                /* coef = sqrt(r + 1e-6), r = det0 / (det1 + 1e-6); neither det is clamped here (coef > 0) */
                real dr = dcoef * 0.5 / q->coef;
                real dd0 = dr / (det1 + 1e-6), dd1 = -dr * det0 / ((det1 + 1e-6) * (det1 + 1e-6));
                if (MUT(6)) dd1 = 0;
                gcxx += dd0 * q->cyy + dd1 * (q->cyy + k);
                gcyy += dd0 * q->cxx + dd1 * (q->cxx + k);
                gcxy += -2.0 * q->cxy * (dd0 + dd1);
            }
            /* conic = inverse of the filtered cov2D (a', b', c') */
            {
                real ap = q->cxx + k, bp = q->cxy, cp = q->cyy + k;
                real det = ap * cp - bp * bp, d2 = 1.0 / (det * det);
                real gA = a[2], gB = a[3], gC = a[4];
                gcxx += d2 * (-cp * cp * gA + bp * cp * gB - bp * bp * gC);
                gcxy += d2 * (2 * bp * cp * gA - (det + 2 * bp * bp) * gB + 2 * ap * bp * gC);
                gcyy += d2 * (-bp * bp * gA + ap * bp * gB - ap * ap * gC);
            }
            /* cov2D = [A0; A1] Sigma [A0; A1]^T */
            const real* c6 = q->c6;
            real S[3][3] = {{c6[0], c6[1], c6[2]}, {c6[1], c6[3], c6[4]}, {c6[2], c6[4], c6[5]}};
            real Gm[3][3];
            for (int r = 0; r < 3; ++r) for (int c = 0; c < 3; ++c)
                Gm[r][c] = gcxx * q->A0[r] * q->A0[c] + gcxy * q->A0[r] * q->A1[c] + gcyy * q->A1[r] * q->A1[c];
            gc6[0] = Gm[0][0]; gc6[3] = Gm[1][1]; gc6[5] = Gm[2][2];
            gc6[1] = Gm[0][1] + Gm[1][0]; gc6[2] = Gm[0][2] + Gm[2][0]; gc6[4] = Gm[1][2] + Gm[2][1];
            real dA0[3], dA1[3];
            for (int r = 0; r < 3; ++r) {
                real SA0 = S[r][0] * q->A0[0] + S[r][1] * q->A0[1] + S[r][2] * q->A0[2];
                real SA1 = S[r][0] * q->A1[0] + S[r][1] * q->A1[1] + S[r][2] * q->A1[2];
                dA0[r] = 2 * gcxx * SA0 + gcxy * SA1;
                dA1[r] = 2 * gcyy * SA1 + gcxy * SA0;
            }
            real dJ00 = 0, dJ02 = 0, dJ11 = 0, dJ12 = 0;
            for (int c = 0; c < 3; ++c) {
                real w0 = view[c * 4 + 0], w1 = view[c * 4 + 1], w2 = view[c * 4 + 2];
                dJ00 += dA0[c] * w0; dJ02 += dA0[c] * w2; dJ11 += dA1[c] * w1; dJ12 += dA1[c] * w2;
            }
            real fx = (real)W / (2.0 * tanfovx), fy = (real)H / (2.0 * tanfovy);
            real tz = q->tz, tz2 = 1.0 / (tz * tz), tz3 = tz2 / tz;
            real dtx = (MUT(4) ? (real)1 : q->xmul) * (-fx * tz2 * dJ02), dty = (MUT(4) ? (real)1 : q->ymul) * (-fy * tz2 * dJ12);
            real dtz = -fx * tz2 * dJ00 - fy * tz2 * dJ11 + 2 * fx * q->tx * tz3 * dJ02 + 2 * fy * q->ty * tz3 * dJ12;
            if (MUT(3)) dtz = -fx * tz2 * dJ00 - fy * tz2 * dJ11;
            /* t = W p + ... */
            gm[0] += view[0] * dtx + view[1] * dty + view[2] * dtz;
            gm[1] += view[4] * dtx + view[5] * dty + view[6] * dtz;
            gm[2] += view[8] * dtx + view[9] * dty + view[10] * dtz;
            /* Sigma = L L^T, L = R diag(mod s) */
            if (!cov3D) {
                const real* sv = scales + 3 * (size_t)i;
                const real* qq = rots + 4 * (size_t)i;
                real r = qq[0], x = qq[1], y = qq[2], z = qq[3];
                real R[3][3] = {{1 - 2 * (y * y + z * z), 2 * (x * y - r * z), 2 * (x * z + r * y)},
                                  {2 * (x * y + r * z), 1 - 2 * (x * x + z * z), 2 * (y * z - r * x)},
                                  {2 * (x * z - r * y), 2 * (y * z + r * x), 1 - 2 * (x * x + y * y)}};
                real sc[3] = {scale_mod * sv[0], scale_mod * sv[1], scale_mod * sv[2]};
                real Gs2[3][3] = {{gc6[0], 0.5 * gc6[1], 0.5 * gc6[2]}, {0.5 * gc6[1], gc6[3], 0.5 * gc6[4]}, {0.5 * gc6[2], 0.5 * gc6[4], gc6[5]}};
                real dLm[3][3], dR[3][3];
                for (int r2 = 0; r2 < 3; ++r2) for (int c = 0; c < 3; ++c) {
                    real v = 0;
                    for (int kk = 0; kk < 3; ++kk) v += 2 * Gs2[r2][kk] * R[kk][c] * sc[c];
                    dLm[r2][c] = v;
                }
                for (int c = 0; c < 3; ++c) {
                    real v = 0;
                    for (int r2 = 0; r2 < 3; ++r2) { v += dLm[r2][c] * R[r2][c]; dR[r2][c] = dLm[r2][c] * sc[c]; }
                    gsc[c] = scale_mod * v;
                }
                gq[0] = 2 * ((MUT(7) ? z : -z) * dR[0][1] + y * dR[0][2] + z * dR[1][0] - x * dR[1][2] - y * dR[2][0] + x * dR[2][1]);
                gq[1] = 2 * (y * dR[0][1] + z * dR[0][2] + y * dR[1][0] - 2 * x * dR[1][1] - r * dR[1][2] + z * dR[2][0] + r * dR[2][1] - 2 * x * dR[2][2]);
                gq[2] = 2 * (-2 * y * dR[0][0] + x * dR[0][1] + r * dR[0][2] + x * dR[1][0] + z * dR[1][2] - r * dR[2][0] + z * dR[2][1] - 2 * y * dR[2][2]);
                gq[3] = 2 * (-2 * z * dR[0][0] - r * dR[0][1] + x * dR[0][2] + r * dR[1][0] - 2 * z * dR[1][1] + y * dR[1][2] + x * dR[2][0] + y * dR[2][1]);
            }
            (void)p;
        }
        if (g_means3D) for (int e = 0; e < 3; ++e) g_means3D[3 * (size_t)i + e] = gm[e];
        if (g_means2D) { g_means2D[2 * (size_t)i] = gm2[0]; g_means2D[2 * (size_t)i + 1] = gm2[1]; }
        if (g_colors) for (int e = 0; e < 3; ++e) g_colors[3 * (size_t)i + e] = gcol[e];
        if (g_opac) g_opac[i] = gop;
        if (g_scales) for (int e = 0; e < 3; ++e) g_scales[3 * (size_t)i + e] = gsc[e];
        if (g_rots) for (int e = 0; e < 4; ++e) g_rots[4 * (size_t)i + e] = gq[e];
        if (g_cov3D) for (int e = 0; e < 6; ++e) g_cov3D[6 * (size_t)i + e] = gc6[e];
        if (g_shs && (!q->visible || colors_precomp)) for (int kk = 0; kk < M * 3; ++kk) g_shs[(size_t)i * M * 3 + kk] = 0.0;
        if (g_shs && q->visible && !colors_precomp) {
            int nb = (deg + 1) * (deg + 1);
            for (int kk = nb; kk < M; ++kk) for (int c = 0; c < 3; ++c) g_shs[((size_t)i * M + kk) * 3 + c] = 0.0;
        }
    }
    return 0;
}

/* Gradients of  L = sum(dL_dcolor * color) + sum(dL_dalpha * alpha) + sum(dL_ddepth * depth)  w.r.t. every input: the composition of the
 * two stages.  Outputs may be NULL.  g_means2D[P][2]: NDC convention (see header). */
int SYM(backward)(SCENE_PARAMS, const real* dL_dcolor, const real* dL_dalpha, const real* dL_ddepth, real* g_means3D, real* g_means2D,
                  real* g_shs, real* g_colors, real* g_opac, real* g_scales, real* g_rots, real* g_cov3D) {
    real* acc = (real*)malloc(sizeof(real) * 10 * (size_t)(P > 0 ? P : 1));
    SYM(accumulators)(SCENE_ARGS, NULL, dL_dcolor, dL_dalpha, dL_ddepth, acc, NULL, NULL, NULL);
    SYM(chain)(SCENE_ARGS, acc, g_means3D, g_means2D, g_shs, g_colors, g_opac, g_scales, g_rots, g_cov3D, NULL);
    free(acc);
    return 0;
}
