"""fp64 reference and per-element error bound of the small operators of the denoise step and of the motion VAE: the fp32 "small projections"
of csrc/elem.hip (gvf_dit_timestep_embed_f32, gvf_dit_modulation_f32, gvf_dit_input_layer_f32, gvf_dit_final_layer_f32), the bf16 timestep
embedder (gvf_dit_timestep_embed_bf16), gvf_split3_bf16, and csrc/vae.hip's gvf_vae_embed and gvf_geglu.  Built on tests/gemm_ref.py and
tests/rowblock_ref.py, whose counts are reused wherever the operation is the same.  Every model returns (reference, bound); for a 16-bit
output the bound is the interval form of gemm_ref: the stored value lies in [R16(a - e), R16(a + e)].

Rounding points and the count behind every term (U = 2^-24, one fp32 rounding; 1 ulp = 2 U; first order, 1e-3 added for the second):

  * dot product over an LDS vector (dot8_f32 / te_dot8: first and second Linear of the timestep embedder, the adaLN GEMV): a lane takes
    ceil(K / 256) float4 groups; in a group four products (1 rounding each), (a + b) + (c + d) (depth 2), one add to the lane's sum; then the
    64-lane tree (6).  A term passes through at most 1 + 2 + ceil(K / 256) + 6 roundings: e_dot = (ceil(K / 256) + 9) U S, S = sum |w x|
    (fused multiply-adds only remove roundings).  The bias add is one more: U |out|.
  * SiLU v / (1 + __expf(-v)): rowblock_ref.cast_model's term, relative ((1 - s)(2 |v| + 4) + 3) U (argument rounding 2 |v| U of e, __expf
    4 U, 1 + e and the division one each); an input error e_v passes with |silu'| <= 1.1.
  * timestep embedder, sinusoid: the phase argument fl(fl(nlp j) / half) is computed here in exact fp32 steps (numpy float32; the division is
    correctly rounded on the device, no fast-math), nlp = (float)(-log((double)max_period)).  f = expf(arg): 3 ulp = 6 U relative; a = fl(t f):
    one more: the phase is off by |t f| 7 U, and that IS the error of cos / sin (slope 1); cosf / sinf add 4 ulp = 8 U of their value.
    At t = 999 the phase term dominates everything else in the kernel: |t f| 7 U = 4.2e-4 on the lowest frequencies (13.9 = sum_j f_j of them
    matter at freq_dim 256), a few 1e-4 of the embedding against 1e-5 at t = 12.5.  No kernel in fp32 can do better: the argument itself is
    only known to 6e-8 relative.  The sharpness condition (tests/test_smallops_ref.py) is therefore checked on the rows where the phase term
    is no larger than the 4 ulp of cosf / sinf themselves, |t f| 7 U <= 8 U, i.e. |t| <= 1 (every f <= 1); the detection threshold at
    t = 12.5 and at t = 999 / 1000 is printed there.  The hidden vector h is not observable, so the chain's bound carries |W2| e_a, which grows
    like sqrt(C) (3 .. 6 1e-4 of t_emb at C >= 192): as rowblock_ref does for its hidden units, each stage is also held on its own by a probe
    (timestep_probe): W2 = identity makes t_emb = silu(h) (f32) / R_bf16(silu(h)) (bf16) observable; W0 = 0 makes h = b0 exact, so t_emb carries
    the second Linear's own error only; and silu(t_emb) is checked from the kernel's OWN t_emb (silu() with e = 0).
    f32 form: h = W0 s + b0 (e_dot(F) + |W0| e_s + U |h|), a = silu(h), t_emb = W2 a + b2 (e_dot(C) + |W2| e_a + U |t_emb|), out = silu(t_emb).
    bf16 form: s16 = R_bf16(s), a16 = R_bf16(silu(h)): each is known to an interval [R(v - e), R(v + e)] only; the reference takes the
    correctly rounded value and the distance to the farther end goes through the next Linear as |W| amb (gemm_ref's a_err).  t_emb (fp32) is
    checked against that bound, the 16-bit output against [R(silu(t_emb) - e), R(silu(t_emb) + e)].  Products of two bf16 values are exact in
    fp32; they are still counted.
  * modulation: e_dot(C) + U |out|.
  * input_layer: Cin fused multiply-adds in order, + b, + pos as pos + (acc + b): rowblock_ref.stream_update's input-layer term
    (2 Cin + 1) U T, T = |pos| + |b| + sum_k |x_k w_k| (two roundings per multiply-add covers the unfused form; the first add, to zero, is
    exact, so + b and + pos fit in the + 1 ... + 2 of that count).
  * final_layer: two-pass LayerNorm over up to 8 values per lane, rowblock_ref.ln_band's reasoning (sum d = 0 exactly, so the common shift
    of the mean enters the sum of squares as K dm^2 only): ((p + p) + p) + p of four pairs (depth 4), the tree (6): depth_s = 10; one more
    for the squares: depth_q = 11; a true division by (float)C (one rounding of mean and of variance); rsqrtf 3 U with var + eps
    (rowblock_ref's count).  adaLN as fl(fl(v rstd) fl(1 + sc)) + sh: |1 + sc| e_y + 2 U |y (1 + sc)| + U |a|.  NP dot products: product,
    pair, three adds in the lane (depth 5) and the 6 exchanges of the butterfly: 11 U S + |W| e_a, bias U |out|.
  * split3: exact.  hi = R_bf16(x), lo = R_bf16(x - hi) (the difference is exact in fp32), bit for bit; [hi | lo | hi] (mode 0) or
    [hi | hi | lo] (mode 1); +0 from cols to pad64(cols).
  * vae_embed: Linear as qdim fused multiply-adds (fmaf in the source, in the order of k) + b: one rounding of each partial sum,
    U (sum_k |acc_k| + |acc + b|) with the partial sums themselves (the order is fixed by the source).  Phase fl(p omega) in an exact fp32 step; the
    hardware sine / cosine by the contract the kernel's comment states: 1e-6 absolute for |phase| <= 0.5 rad (a claim under test).  Each wave
    LayerNorm: ni = ceil(C / 64) values per lane in sequence (the first add, to zero, is exact), the tree: depth_s = ni + 5, depth_q one more, division by (float)C, rsqrtf
    3 U; an input known to e_x only moves y by rstd (e_x + mean e_x + |y| mean(|y| e_x)) (first order in e_x / sigma, a factor 1 + 4 max(e_x) / sigma for the next).
    The bound of a LayerNorm is kept in two parts: what is common to a row (rstd (e_mean + mean e_x): ONE number added to every element) and the
    element-wise rest.  Their sum bounds the fp32 output (+ U |s| for the add); the third LayerNorm (eps_prenorm) subtracts the row's mean
    again and is blind to the common part (ln_band's sum d = 0 argument, one stage further): only the element-wise part is its e_x.  Then
    the 16-bit interval.  final_layer's dot products see the common part of their LayerNorm through |sum_c w_c (1 + sc_c)|, not sum |.|.
  * geglu: R16(a gelu_erf(g)) from the 16-bit inputs: gemm_ref's GEGLU term 8 U |a| (|g| + |gelu(g)|) (erff and the 1 + erf cancellation),
    plus |a| 2^-126 for an fp32 intermediate in the subnormal range (rowblock_ref.cast_model's allowance).

Accuracy figures of the transcendentals.  No accuracy table ships with the ROCm tree on the build machine (none found under its
documentation), so: __expf 4 U, erff inside gemm_ref's 8 U term and rsqrtf 3 U (with the rounding of its argument) are the counts
tests/rowblock_ref.py and tests/gemm_ref.py already commit to; expf 3 ulp and sinf / cosf 4 ulp are the limits of the OpenCL C full-profile
table that the device math library (built without fast-math, gvfdiffusion_amd/_build.py: the library routines, not the native instructions)
is specified to meet, quoted from memory of that specification; __sinf / __cosf 1e-6 absolute from the comment in csrc/vae.hip.  None was
fitted to the kernels.

Measured on the MI355X (tests/test_smallops_conformance_gpu.py; largest |err| / bound over all cases of a kernel, no element outside):
  final_layer 0.04 (the LayerNorm depths are worst cases, its errors add like a square root); input_layer 0.22; modulation 0.26;
  timestep_embed_f32: t_emb 0.03, silu(t_emb) 0.02 against the chain, 0.45 from its own t_emb (the SiLU term alone), probes 0.05 / 0.04;
  timestep_embed_bf16: t_emb 0.23, first-Linear probe 1.00 (it IS a bf16 store), second-Linear probe 0.05;
  vae_embed: fp32 embedding 0.15 (0.07 at 768 x 14, the same for the register and the LDS kernel) -- the 1e-6 of the hardware sine / cosine,
  most of that bound, holds; every 16-bit output (timestep_embed_bf16, vae_embed, geglu) 1.00 by construction -- the store is within its
  interval, whose far end is what the bound measures; split3 bit-exact.  Share of vae_embed outputs whose interval spans more than one 16-bit
  value (the reference alone, plain cases): 1.5 .. 2.0 % (bf16) / 8.9 .. 11.3 % (fp16); near-zero weights 0.5 % / 5 %; a common bias of 100
  sigma 4.8 % / 24 %, with the embedding's bound at 1.4 .. 2.6 1e-4 of the row's RMS.
Everything here runs on torch CPU tensors in float64; pass .cpu() copies of device tensors."""
import math

import numpy as np
import torch

import gemm_ref as G
import rowblock_ref as R
from gemm_ref import U32, r16, _round_bound, excess            # noqa: F401  (re-exported for the tests)

SILU_LIP = 1.1                       # max |d/dx silu(x)| = 1.0998 at x = 2.4
SECOND = 1.0 + 1e-3
BF16, F16, F64 = torch.bfloat16, torch.float16, torch.float64
EXP_U, SINCOS_U, HW_SINCOS_ABS = 6.0, 8.0, 1e-6


def pad64(k):
    return (k + 63) // 64 * 64


def dot_depth(K):
    return (K + 255) // 256 + 9


def linear(W, v, b=None, e_v=None):
    """(out, bound) of out[i][n] = W[n] . v[i] + b[n] by dot8_f32 / te_dot8; e_v: what v is known to."""
    W, v = W.double(), v.double()
    out = v @ W.T
    if b is not None:
        out = out + b.double()
    e = dot_depth(W.shape[1]) * U32 * (v.abs() @ W.abs().T) + U32 * out.abs()
    if e_v is not None:
        e = e + e_v @ W.abs().T
    return out, e * SECOND


def silu(x, e):
    """(silu(x), bound) of v / (1 + __expf(-v)) for v within e of x (rowblock_ref.cast_model's term)."""
    s = torch.sigmoid(x)
    g = x * s
    rel = ((1.0 - s) * (2.0 * x.abs() + 4.0) + 3.0) * U32
    return g, SILU_LIP * e + (g.abs() + SILU_LIP * e) * rel + 2.0 ** -126 + g.abs() * (x < -88.0)


def _amb16(v, e, dt):
    """(R16(v), distance to the farther end of [R16(v - e), R16(v + e)])."""
    c = r16(v, dt)
    return c, torch.maximum(r16(v + e, dt) - c, c - r16(v - e, dt))


# ---- timestep embedder ------------------------------------------------------------------------------------------------------------------

def neg_log_period(max_period):
    return np.float32(-math.log(float(np.float32(max_period))))


def frequencies_arg(F, max_period):
    """fl(fl(nlp j) / half), j < F / 2, in exact fp32 steps."""
    half = F // 2
    j = np.arange(half, dtype=np.float32)
    return ((neg_log_period(max_period) * j).astype(np.float32) / np.float32(half)).astype(np.float32)


def sinusoid(t, F, max_period=10000.0):
    """(value, bound) of [cos(t f) | sin(t f)], (B, F)."""
    f = torch.from_numpy(np.exp(frequencies_arg(F, max_period).astype(np.float64)))
    a = t.double()[:, None] * f[None]
    val = torch.cat([torch.cos(a), torch.sin(a)], 1)
    e = torch.cat([a.abs(), a.abs()], 1) * (EXP_U + 1.0) * U32 + SINCOS_U * U32 * val.abs()
    return val, e * SECOND


def timestep_embed_f32(t, F, w0, b0, w2, b2, max_period=10000.0):
    """((t_emb, bound), (silu(t_emb), bound)), each (B, C)."""
    s, e_s = sinusoid(t, F, max_period)
    h, e_h = linear(w0, s, b0, e_s)
    a, e_a = silu(h, e_h)
    te, e_te = linear(w2, a, b2, e_a)
    out, e_out = silu(te, e_te)
    return (te, e_te), (out, e_out)


def timestep_embed_bf16(t, F, w0, b0, w2, b2, max_period=10000.0):
    """w0 (C, F), w2 (C, C) bf16.  ((t_emb, bound), (silu(t_emb), bound of the bf16 store))."""
    s, e_s = sinusoid(t, F, max_period)
    s16, amb_s = _amb16(s, e_s, BF16)
    h, e_h = linear(w0, s16, b0, amb_s)
    a, e_a = silu(h, e_h)
    a16, amb_a = _amb16(a, e_a, BF16)
    te, e_te = linear(w2, a16, b2, amb_a)
    out, e_out = silu(te, e_te)
    return (te, e_te), (out, _round_bound(out, e_out, BF16))


# ---- modulation, input_layer ------------------------------------------------------------------------------------------------------------

def modulation(s, w, bias=None):
    return linear(w, s, bias)


def pos_rows(M, rpg, period):
    r = torch.arange(M)
    return (r // rpg) * period + (r % rpg) % period


def input_layer(x, w_t, bias=None, pos=None, period=0, rpg=0):
    """x (M, Cin), w_t (Cin, C), pos (>= groups * period, C) or None."""
    M, C = x.shape[0], w_t.shape[1]
    rs = torch.zeros((M, C)) if pos is None else pos[pos_rows(M, rpg, period)]
    return R.stream_update(rs, in_x=x, in_wt=w_t, in_b=torch.zeros(C) if bias is None else bias)


# ---- two-pass wave LayerNorm --------------------------------------------------------------------------------------------------------------

def layernorm(x, eps, depth_s, depth_q, e_x=None):
    """(y, e_elem, e_common) of (x - mean) rstd computed in two passes with the given summation depths and a true division by (float)K; x fp64
    (M, K).  rowblock_ref.ln_model's "elem" form with the depths as arguments and an optional (element-wise) input error e_x, the bound split
    in two: e_common (M, 1) bounds ONE number per row that is added to every element (rstd times the error of the mean), e_elem the rest.
    A consumer that subtracts the row's mean again (the next LayerNorm) is blind to the common part, and a dot product sees it through
    |sum_c w_c| instead of sum_c |w_c|: ln_band's sum d = 0 argument, one stage further."""
    K = x.shape[1]
    mean = x.mean(1, keepdim=True)
    d = x - mean
    var = (d * d).mean(1, keepdim=True)
    rstd = 1.0 / torch.sqrt(var + eps)
    y = d * rstd
    e_mean = depth_s * U32 * x.abs().sum(1, keepdim=True) / K + U32 * mean.abs()
    Q = ((d.abs() + e_mean) ** 2).sum(1, keepdim=True)
    e_q = (depth_q + 2.1) * U32 * Q + K * e_mean ** 2
    d_r = 0.5 * (e_q / K + U32 * var) / (var + eps) + 3.0 * U32
    e_el = d.abs() * rstd * d_r + rstd * U32 * (d.abs() + e_mean) + U32 * y.abs()
    e_com = rstd * e_mean
    if e_x is not None:
        second = 1.0 + 4.0 * (e_x * rstd).max(1, keepdim=True).values           # the next order in e_x / sigma
        e_el = e_el + second * rstd * (e_x + y.abs() * (y.abs() * e_x).mean(1, keepdim=True))
        e_com = e_com + second * rstd * e_x.mean(1, keepdim=True)
    return y, e_el * SECOND, e_com * SECOND


def final_layer(x, w, bias=None, shift=None, scale=None, rpg=1, eps=1e-6):
    """x (M, C) fp32, w (Cout, C), shift / scale (groups, >= C) or None."""
    M, C = x.shape
    y, e, e_com = layernorm(x.double(), eps, 10, 11)
    sc = torch.ones((M, C), dtype=F64)
    if scale is not None:
        sc, sh = 1.0 + R.group_rows(scale, M, rpg, C), R.group_rows(shift, M, rpg, C)
        a = y * sc + sh
        e = sc.abs() * e + 2.0 * U32 * (y * sc).abs() + U32 * a.abs()
        y = a
    W = w.double()
    out = y @ W.T
    if bias is not None:
        out = out + bias.double()
    return out, (11.0 * U32 * (y.abs() @ W.abs().T) + e @ W.abs().T + e_com * (sc @ W.T).abs() + U32 * out.abs()) * SECOND


# ---- split3 -----------------------------------------------------------------------------------------------------------------------------------

def split3(x, mode):
    """bf16 (rows, 3 pad64(cols)), exact."""
    rows, cols = x.shape
    Kp = pad64(cols)
    hi = x.to(BF16)
    lo = (x - hi.float()).to(BF16)
    out = torch.zeros((rows, 3 * Kp), dtype=BF16)
    for i, part in enumerate((hi, lo, hi) if mode == 0 else (hi, hi, lo)):
        out[:, i * Kp:i * Kp + cols] = part
    return out


# ---- vae_embed --------------------------------------------------------------------------------------------------------------------------------

def point_embed_map(C):
    """channel -> (axis, is_sin, frequency index): [sin(p_0 w) | cos(p_0 w) | sin(p_1 w) | cos(p_1 w) | sin(p_2 w) | cos(p_2 w)]."""
    E = C // 6
    c = torch.arange(C)
    axis = c // (2 * E)
    j = c - axis * 2 * E
    return axis, j < E, torch.where(j < E, j, j - E)


def vae_embed(q, W, b, omega, eps_embed, eps_prenorm, dt):
    """q (P, qdim), W (C, qdim), b (C,), omega (C / 6,), all fp32.  ((embedding fp32, bound), (out16 value, bound of the 16-bit store), amb)."""
    C, qdim = W.shape
    qd, Wd = q.double(), W.double()
    part = torch.cumsum(qd[:, None, :] * Wd[None], 2)              # the accumulator after each fmaf (P, C, qdim), in the source's order of k
    lin = part[..., -1] + b.double()
    e_lin = U32 * (part.abs().sum(2) + lin.abs())
    axis, is_sin, fi = point_embed_map(C)
    ph = (q[:, axis] * omega[fi][None]).double()                     # fl(p omega): fp32 tensors, one rounding, as the kernel's
    pe = torch.where(is_sin[None], torch.sin(ph), torch.cos(ph))
    e_pe = torch.full_like(pe, HW_SINCOS_ABS)
    ni = (C + 63) // 64
    y1, e1, c1 = layernorm(lin, eps_embed, ni + 5, ni + 6, e_lin)
    y2, e2, c2 = layernorm(pe, eps_embed, ni + 5, ni + 6, e_pe)
    s = y1 + y2
    e_s = (e1 + e2 + U32 * (s.abs() + c1 + c2)) * SECOND           # element-wise part; c1 + c2 is common to the row and LN_pre subtracts it again
    y3, e3, c3 = layernorm(s, eps_prenorm, ni + 5, ni + 6, e_s)
    e3 = e3 + c3
    return (s, e_s + c1 + c2), (y3, _round_bound(y3, e3, dt)), r16(y3 + e3, dt) - r16(y3 - e3, dt)


# ---- geglu -------------------------------------------------------------------------------------------------------------------------------------

def geglu(x16):
    """x16 (rows, 2 F) 16-bit -> (value a gelu_erf(g) in fp64, E, lo, hi, nan_ok): the store lies in [lo, hi] = [R16(v - E), R16(v + E)]; NaN
    where the expression is NaN (NaN operands, 0 * inf, -inf gates: 0.5 * -inf * (1 + -1)).  nan_ok: an infinite value times a gelu whose
    fp32 value may be zero (|gelu| within its own error term 8 U (|g| + |gelu|): gates below -5.4, where erff returns -1): inf * 0 = NaN and
    inf * tiny = inf are both fp32 evaluations of the expression."""
    dt = x16.dtype
    F = x16.shape[1] // 2
    a, g = x16[:, :F].double(), x16[:, F:].double()
    gel = G.gelu_erf(g)
    v = a * gel
    e_gel = 8.0 * U32 * (g.abs() + gel.abs()) + 2.0 ** -126
    E = a.abs() * e_gel
    E = torch.where(torch.isfinite(E), E, torch.zeros_like(E))
    return v, E, r16(v - E, dt), r16(v + E, dt), torch.isinf(a) & (gel.abs() <= e_gel)


def geglu_check(out16, x16):
    """(n_bad, worst |err| / bound over the elements whose interval is finite) -- no element is exempt: an element whose expression is NaN
    must be NaN, every other one must lie in its interval (infinities compare as numbers, -0 == +0 only where the interval holds 0)."""
    v, E, lo, hi, nan_ok = geglu(x16)
    o = out16.double()
    nan = torch.isnan(v)
    ok = torch.where(nan, torch.isnan(o), ((o >= lo) & (o <= hi)) | (nan_ok & torch.isnan(o)))
    fin = torch.isfinite(lo) & torch.isfinite(hi) & ~nan
    bnd = torch.maximum((hi - v).abs(), (lo - v).abs())
    ratio = ((o - v).abs() / bnd.clamp_min(1e-300))[fin]
    return int((~ok).sum()), float(ratio.max()) if ratio.numel() else 0.0


# ---- test data: the GPU matrix (tests/test_smallops_conformance_gpu.py) and its CPU-sized part (tests/test_smallops_ref.py) ------------------
# Every listed value of every axis of the matrix occurs in at least one case, with the combinations the issue names (both NP at C = 512, the
# grid wraps, 768 x 13 / 768 x 16); the full cross product would be thousands of launches against an fp64 reference for no further code path.

NAN = float("nan")


def _gen(seed):
    g = torch.Generator().manual_seed(seed)
    return g, (lambda *s, sc=1.0: torch.randn(s, generator=g) * sc)


def adversarial_rows(x, first=0):
    """The rows of the LayerNorm tests: a common offset of 100 sigma (3 rows), constant rows (3), one huge element per 29 (2)."""
    n = x.shape[0] - first
    if n >= 3:
        x[first:first + 3] += 200.0
    for r, v in zip(range(first + 3, min(first + 6, x.shape[0])), (3.0, -0.37, 0.0)):
        x[r] = v
    if n >= 8:
        x[first + 6:first + 8, 1::29] = 1e4
    return x


# C, Cout, M, rpg, modulation, bias, adversarial
FINAL_CASES = [(4, 1, 1, 1, True, True, False), (64, 5, 3, 2, True, False, False), (192, 14, 5, 7, True, True, False), (256, 16, 5, 1, False, True, False),
               (260, 17, 3, 2, True, True, False), (320, 31, 5, 3, True, False, False), (512, 16, 5, 5, False, False, False), (512, 14, 40, 16, True, True, True),
               (512, 32, 4097, 1000, True, True, True), (512, 14, 12291, 4097, True, True, False), (320, 32, 12291, 1, True, True, False)]


def make_final(C, Cout, M, rpg, mod, bias, adv, seed=0):
    g, rn = _gen(7000 + 13 * C + Cout + M + seed)
    groups = (M + rpg - 1) // rpg
    x = rn(M, C) * 2 + 0.5
    d = dict(C=C, Cout=Cout, M=M, rpg=rpg, eps=1e-6, adv_rows=0, w=rn(Cout, C, sc=1 / math.sqrt(C)), bias=rn(Cout, sc=0.1) if bias else None, mod=None, shift=None, scale=None)
    if adv:
        adversarial_rows(x, 8)
        d["adv_rows"] = (8, 16)
    d["x"] = x
    if mod:
        ld = 4 * C + 12                                            # [4 | shift C | C + 4 | scale C | C + 4]: mod_ld > 4 C, NaN in every gap
        m = torch.full((groups, ld), NAN)
        m[:, 4:4 + C] = rn(groups, C, sc=0.3)
        m[:, 2 * C + 8:3 * C + 8] = rn(groups, C, sc=0.3)
        if adv:
            m[-1, 2 * C + 8:2 * C + 8 + C // 2] = -1.0             # 1 + scale = 0 in half of the last group's columns
        d.update(mod=m, mod_ld=ld, shift_off=4, scale_off=2 * C + 8, shift=m[:, 4:], scale=m[:, 2 * C + 8:])
    return d


# C, Cin, M, pos (None | (rpg, period)), bias
INPUT_CASES = [(1, 1, 1, None, True), (64, 7, 15, (5, 5), True), (255, 14, 16, (6, 3), True), (256, 16, 17, None, False), (257, 17, 1000, (48, 16), True),
               (511, 23, 17, (7, 7), False), (512, 24, 1000, (250, 125), True), (512, 14, 1000, (96, 24), True)]


def make_input(C, Cin, M, pos, bias, seed=0):
    g, rn = _gen(8000 + 7 * C + Cin + M + seed)
    d = dict(C=C, Cin=Cin, M=M, x=rn(M, Cin), w_t=rn(Cin, C, sc=0.3), bias=rn(C, sc=0.1) if bias else None, pos=None, rpg=0, period=0)
    if pos is not None:
        rpg, period = pos
        d.update(rpg=rpg, period=period, pos=rn((M + rpg - 1) // rpg * period, C))
    return d


# C, N, B, bias
MODULATION_CASES = [(4, 1, 1, True), (252, 31, 2, True), (256, 32, 5, False), (260, 33, 1, True), (512, 7 * 512 + 3, 2, True), (1024, 7 * 1024 + 3, 5, True),
                    (8, 65536 + 37, 1, True)]


def make_modulation(C, N, B, bias, seed=0):
    g, rn = _gen(9000 + C + N + B + seed)
    return dict(C=C, N=N, B=B, s=rn(B, C), w=rn(N, C, sc=1 / math.sqrt(C)), bias=rn(N, sc=0.1) if bias else None)


T_VALUES = [0.0, 1e-3, 1.0, 12.5, 999.0, 1000.0]
T_PLAIN = 3                                                        # the first three: |t| <= 1 (module docstring)
# F, C, biases, t_emb
TIMESTEP_F32_CASES = [(4, 4, True, True), (64, 64, False, True), (256, 192, True, False), (256, 512, True, True), (1024, 1020, True, True), (1024, 1024, False, False),
                      (64, 1024, True, True)]
TIMESTEP_BF16_CASES = [(2, 1, True, True), (6, 3, True, True), (64, 64, False, True), (256, 190, True, False), (258, 512, True, True), (1024, 1023, True, True),
                       (256, 1024, True, True)]


def make_timestep(F, C, biases, t_emb, dt=None, seed=0):
    g, rn = _gen(10000 + F + 3 * C + seed)
    w0, w2 = rn(C, F, sc=1 / math.sqrt(F)), rn(C, C, sc=1 / math.sqrt(C))
    if dt is not None:
        w0, w2 = w0.to(dt), w2.to(dt)
    return dict(F=F, C=C, t=torch.tensor(T_VALUES), w0=w0, w2=w2, b0=rn(C, sc=0.1) if biases else None, b2=rn(C, sc=0.1) if biases else None, want_t_emb=t_emb)


def timestep_probe(d, kind):
    """"first": W2 = identity, b2 = 0 (t_emb IS the rounded silu(h)); "second": W0 = 0 and a bias b0 of order 1 (h = b0 exactly)."""
    p = dict(d, want_t_emb=True)
    C = d["C"]
    if kind == "first":
        p.update(w2=torch.eye(C).to(d["w2"].dtype), b2=None)
    else:
        g, rn = _gen(10500 + C)
        p.update(w0=torch.zeros_like(d["w0"]), b0=rn(C))
    return p


# cols, rows, ld_src - cols, mode
SPLIT3_CASES = [(1, 5, 0, 0), (3, 7, 0, 1), (63, 9, 0, 0), (64, 33, 0, 1), (64, 33, 3, 0), (65, 10, 4, 1), (1024, 37, 0, 0), (1024, 6, 1, 1), (65, 131100, 0, 0)]


def make_split3(cols, rows, seed=0):
    g, rn = _gen(11000 + cols + rows + seed)
    x = rn(rows, cols) * torch.exp2(torch.randint(-20, 20, (rows, cols), generator=g).float())
    sp = torch.tensor([0.0, -0.0, 2.0 ** -149, -2.0 ** -140, 2.0 ** -127, 2.0 ** -126, 1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -8, -(1.0 + 2.0 ** -8 + 2.0 ** -23),
                       1.0 + 2.0 ** -8 - 2.0 ** -24, 3.3895313892515355e38, -3.3895313892515355e38, 3.38e38, 3.4028234663852886e38, 2.0 ** 127, 1.00390625, 0.99609375 + 2.0 ** -9])
    flat = x.view(-1)
    n = min(flat.numel(), sp.numel())
    flat[:n] = sp[:n]
    if flat.numel() > 2 * sp.numel():
        flat[-sp.numel():] = -sp
    return x


# C, qdim, P, kind ("plain" | "encoder" | "tiny" | "bias"), out_embed
VAE_CASES = [(6, 3, 1, "plain", True), (96, 13, 63, "plain", False), (192, 14, 64, "plain", True), (390, 16, 65, "plain", True), (768, 13, 255, "plain", True),
             (768, 16, 256, "plain", False), (768, 14, 257, "plain", True), (390, 14, 1000, "plain", False), (96, 3, 4099, "plain", True),
             (768, 14, 1000, "encoder", True), (192, 14, 65, "tiny", True), (768, 14, 63, "bias", True), (390, 13, 64, "bias", True)]
VAE_ADVERSARIAL = ("tiny", "bias")


def make_vae(C, qdim, P, kind, seed=0):
    g, rn = _gen(12000 + C + 5 * qdim + P + seed)
    q = rn(P, qdim)
    q[:, :3] = torch.rand((P, 3), generator=g) - 0.5
    if P >= 3:
        q[0, :3] = torch.tensor([0.5, -0.5, 0.0])
    W, b = rn(C, qdim, sc=1 / math.sqrt(qdim)), rn(C, sc=0.1)
    if kind == "encoder":
        W[:, :3] = 0.0
    if kind == "tiny":                                             # the variance of the Linear is far below eps_embed: eps decides
        W, b = W * 1e-4, b * 1e-4
    if kind == "bias":
        b = b + 100.0
    E = C // 6
    omega = (1.0 / 10000 ** (torch.arange(E, dtype=F64) / (E / 2.0))).float()
    return dict(C=C, qdim=qdim, P=P, kind=kind, q=q, W=W, b=b, omega=omega, eps_embed=1e-5, eps_prenorm=1e-6)


# F, rows, ld_in - 2 F, ld_out - F
GEGLU_CASES = [(8, 1, 0, 0), (8, 777, 8, 16), (264, 1, 8, 8), (264, 777, 16, 8), (3072, 777, 0, 0), (3072, 12288, 0, 0)]
GEGLU_VALUES = [1.0, -0.37, 3.5, 1e-3, -250.0, 0.0, -0.0, float("inf"), float("-inf"), NAN, 6e4, -1e-7]


def make_geglu(F, rows, dt, seed=0):
    g, rn = _gen(13000 + F + rows + seed)
    return (rn(rows, 2 * F) * 1.5).to(dt)


def make_geglu_all_gates(dt):
    """(len(GEGLU_VALUES), 2 * 65536): row r pairs the value GEGLU_VALUES[r] with every 16-bit pattern as the gate."""
    gates = (torch.arange(65536) - 32768).to(torch.int16).view(dt)
    vals = torch.tensor(GEGLU_VALUES).to(dt)
    return torch.cat([vals[:, None].expand(-1, 65536), gates[None].expand(len(GEGLU_VALUES), -1)], 1).contiguous()
