"""fp64 reference and per-element error bound of the row-block launch (csrc/rowblock.hip, gvf_rowblock_fused) and of the unfused
LayerNorm it is compared with elsewhere (csrc/elem.hip: gvf_layernorm_modulate), built on tests/gemm_ref.py.

Only x, hb_out, out3 (and the K / V^T tiles) of a launch are observable, so the stages are checked one at a time FROM THE KERNEL'S OWN
OBSERVABLE INPUT wherever there is one, and only what is left gets a bound propagated through an unobservable 16-bit intermediate:

  stage            reference                                   input taken from               bound
  stream update    rs + g (A W1^T + b1), rs = x | x_in | + in   the launch's inputs            single stage, fp32 noise
  LayerNorm        R16(LN(x) mul + add)                         the KERNEL'S x                 single stage: ln_band()
  last projection  R16(hb W3^T + b3)                            the KERNEL'S hb_out            single stage (gemm_ref STORE_16)
                                                                or the kernel's x through the LayerNorm band (a_err), when the launch has
                                                                no hb_out (temporal launches refuse it)
  hidden units     R16(gelu(hb Wfc1^T + b))                     probe launch: Wfc2 = identity, x = 0, gate_m = 1: x' IS h, exactly
  MLP update       x1 + g_m (h Wfc2^T + b_fc2)                  x1 = the x of the same launch with gate_m = 0 (bit exact: x1 + 0 * finite)
                                                                propagated: LayerNorm band -> hidden ambiguity -> |Wfc2|
  temporal update  x1 + g_t (o Wout^T + b_out)                  x1 likewise (t_gate = 0); propagated: LayerNorm band -> q / k / v ambiguity
                                                                -> scores -> P -> o -> |Wout|

Rounding points of the kernel and the terms of each bound (U = 2^-24; every factor is a count of fp32 roundings, first order):

  * stream update (stream_update): the MFMA part is gemm_ref's RESID model: (ceil(K1 / 32) + 2) U (S + |b1|) for the accumulator, scaled by
    |g|, plus 2 U (|rs| + |g v|) for the multiply and the add.  K1 = 0 (no closing projection): acc = 0, b = 0, g = 1 and the update is
    rs + 1 * (0 + 0) = rs exactly (bound 0).  input_layer (in_x, Cin <= 16): rs += b_in (one rounding), then Cin multiply-adds per column,
    fused or not (two roundings each at most), every partial sum at most T = |rs| + |b_in| + sum_k |in_x_k W_k|: (2 Cin + 1) U T.
  * LayerNorm (ln_band, kernel "rowblock" = rb_layernorm): two passes.  sum: 16 values per lane ((a + b) + (c + d) per column tile, added
    to the lane's sum: depth 6), two lane exchanges, 8 per-wave partials added in sequence: depth 16 at most -> e_mean = 16 U sum|x| / 512
    (the product with 1 / 512 is exact).  d' = fl(x - mean') = d - dm + rho, |dm| <= e_mean, |rho| <= U |d'|.  sum of squares: because
    sum d = 0 exactly the common shift dm enters as K dm^2 only (no cancellation term 2 dm sum d): e_q = 28 U Q + K e_mean^2 + 2.1 U Q with
    Q = sum (|d| + e_mean)^2 (one rounding per square, 16 sequential adds per lane, two exchanges, 8 partials: depth 28 at most).  var + eps
    one rounding, rsqrtf about one ulp: relative error of rstd d_r = e_q / (2 K (var + eps)) + 3 U.  y = fl(fl(d' rstd') mul) + add, fused or
    not, mul = fl(ln_w fl(1 + scale)) (2 U), add = fl(fl(ln_b fl(1 + scale)) + shift) (2 U |ln_b (1 + scale)| + U |add|):
        e_a = |mul| (|d| rstd d_r + rstd (e_mean + U |d|) + U |y|) + 2 U |y mul| + e_add + U |y mul| + U |a|
    and the 16-bit store is round-to-nearest-even: the stored value lies in [R16(a - e_a), R16(a + e_a)].
    Kernel "elem" (ln_mod_kernel / ln_mod_generic_kernel): per-lane sums (depth C / 256 + 2 for the float4 form, ceil(C / 64) for the generic
    one; one more for the squares), a 64-lane tree (depth 6), a true division by (float)C (one more rounding of the mean and of the variance), and the
    affine and adaLN steps applied one after the other: y1 = fl(fl(y0 w) + b), y2 = fl(fl(y1 fl(1 + scale)) + shift).
    Width on the data of test_rowblock_launch_equals_the_unfused_launches (M = 96, N(0,1) * 2 + 0.5 rows, adaLN): the share of elements whose
    interval spans two 16-bit values is 0.32 % (bf16) / 1.94 % (fp16), against 0.37 % / 2.36 % for gemm_ref.ln_operand's one-pass form
    (tests/test_rowblock_ref.py::test_two_pass_band_is_narrower_than_the_one_pass_band prints both): narrower by the cancellation term only --
    what is left is the worst-case depth of the two sums (16 U sum|x| / 512 on the mean alone is 13 U against a true error of 1 .. 2 U) acting on
    the elements near zero, whose 16-bit cells are small.  On the adversarial data of make_case(adv=True) 4 % (bf16) / 9 %
    (fp16) of a 96-row case, very unevenly: rows with a common offset of 100 sigma 12 .. 15 % / about 50 % (e_mean grows with |mean|), rows
    with one huge element under 1.5 %, constant rows all of their elements, but within a bound of at most 2.3e-2 on values of order 1 at
    |c| = 12 (|c| rstd e_mean = 1e-3 |c|: the constant must stay small for that row to check more than finiteness).
  * hidden units (hidden_units): pre = hb Wfc1^T + b with gemm_ref's accumulation error (+ the LayerNorm ambiguity a_err when hb is not
    observable); rb_gelu_tanh(x) = x rcp(1 + exp2(c0 (x + c1 x^2 x))): the exponent z is formed with 5 roundings of same-signed terms plus the
    rounded constant (6 U |z|, i.e. a relative 6 ln2 |z| U = 12 |u| U of e = 2^z, u = sqrt(2 / pi)(x + 0.044715 x^3)), v_exp_f32 and v_rcp_f32
    one ulp each (2 U), 1 + e and the product one rounding each; de / e moves the sigmoid s by (1 - s) de / e:
        relative ((1 - s) (12 |u| + 2) + 4) U,   E = 1.13 e_pre + |gelu| rel,   stored value in [R16(g - E), R16(g + E)]
    (gemm_ref's GELU_16 form with this kernel's error terms).
  * MLP update (mlp_update): h_amb = distance from R16(g) to the farther end of that interval; acc2 runs over hidden / 32 k-steps across the
    slices: gemm_ref RESID with K = hidden and a_err = h_amb |Wfc2|^T.
  * last projection (projection): gemm_ref STORE_16 (K = 512), a_err = amb |W3|^T when fed through the LayerNorm band.
  * temporal section (temporal_update): see that function; the rounding points are attn_ref's "small" path (q, k, v rounded to 16 bit, RMS
    norm in fp32 on the rounded values, argument fl(fl(s c) - fl(m c)), l from the unrounded p, P = R16(p)) except that the inverse norm is the
    hardware rsq of max(ss, 1e-24) times sqrt(32) (attn: division by max(sqrt(ss), 1e-12)), the normalisation is o = R16(fl(N) rcp(l))
    (attn: the same form), and q / k / v are themselves only known to an interval (they come from the LayerNorm band), which attn_ref's
    model() has no input for -- so the section carries its own interval arithmetic, with attn_ref's counts.

Measured on the MI355X (tests/test_rowblock_conformance_gpu.py, tests/test_elem_conformance_gpu.py; largest |err| / bound over all cases, bf16 and
fp16): stream update 0.49 (K1 = 128 .. 512), 0.34 (input_layer); phase-1 stream of the MLP / temporal launches 0.50; MLP update 0.72 (hidden
512, where the fp32 terms are most of the bound), 0.52 at hidden 2048; temporal update 0.03 (its bound is the widest: see temporal_update);
every 16-bit output (hb_out, out3, the two probes, gvf_layernorm_modulate, gvf_cast_pad) 1.00 by construction -- the store is within its
interval, whose far end is what the bound measures -- with no element outside.  Widths are recorded where each function is defined.  Row mapping of the temporal section: local row tok * T + frame of a
block <-> stream row group * rpg + frame * N + tok; a group's padding rows are its phantom tokens and are read by nobody.
Everything here runs on torch CPU tensors in float64; pass .cpu() copies of device tensors."""
import math

import torch

import gemm_ref as G
from gemm_ref import U32, GELU_LIP, r16, _round_bound, excess, accumulation_error       # noqa: F401  (re-exported for the tests)

C = 512
BM = 48
SQRT_2_PI = math.sqrt(2.0 / math.pi)
LOG2E = 1.4426950408889634


def group_rows(v, M, rpg, n=C):
    """(groups, >= n) per-group vectors -> fp64 (M, n), row m = v[m // rpg]; None -> None."""
    if v is None:
        return None
    return v[:, :n].double()[torch.arange(M) // rpg]


def residual_source(x0, x_in=None, period=0, rpg=0):
    """The fp32 residual tile the kernel starts from: x0 (M, 512), or x_in[(row / rpg) * period + (row % rpg) % period]."""
    if x_in is None:
        return x0
    M = x0.shape[0]
    r = torch.arange(M)
    return x_in[(r // rpg) * period + (r % rpg) % period]


# ---- stream update ----------------------------------------------------------------------------------------------------------------------

def stream_update(rs, a16=None, w16=None, b1=None, gate=None, rpg=1, in_x=None, in_wt=None, in_b=None):
    """(reference, bound) of x' = rs + g (a W1^T + b1) [rs += in_x W_in^T + b_in first, when a16 is None].  rs fp32 (M, 512); gate fp32
    (groups, >= 512) or None; in_wt fp32 (Cin, 512) = W_in^T."""
    if a16 is not None:
        assert in_x is None
        return G.model(a16, w16, b1, G.EPI_RESID_F32, gate=gate, rpg=rpg, x0=rs)
    r = rs.double()
    if in_x is None:
        return r, torch.zeros_like(r)
    b = torch.zeros(C, dtype=torch.float64) if in_b is None else in_b.double()
    ref = r + b + in_x.double() @ in_wt.double()
    T = r.abs() + b.abs() + in_x.double().abs() @ in_wt.double().abs()
    return ref, (2 * in_x.shape[1] + 1) * U32 * T


# ---- LayerNorm ------------------------------------------------------------------------------------------------------------------------

def ln_model(X, eps, ln_w=None, ln_b=None, shift=None, scale=None, rpg=1, kernel="rowblock"):
    """(a, e_a): the fp64 value LN(X) mul + add before the 16-bit store and the bound on the kernel's fp32 value (module docstring).
    X fp32 (M, K); ln_w, ln_b fp32 (K,); shift, scale fp32 (groups, >= K)."""
    x = X.double()
    M, K = x.shape
    mean = x.mean(1, keepdim=True)
    d = x - mean
    var = (d * d).mean(1, keepdim=True)
    rstd = 1.0 / torch.sqrt(var + eps)
    y = d * rstd
    one, zero = torch.ones((1, K), dtype=torch.float64), torch.zeros((1, K), dtype=torch.float64)
    w = one if ln_w is None else ln_w.double()[None]
    b = zero if ln_b is None else ln_b.double()[None]
    sc = one if scale is None else 1.0 + group_rows(scale, M, rpg, K)
    sh = zero if shift is None else group_rows(shift, M, rpg, K)
    sum_abs = x.abs().sum(1, keepdim=True)
    if kernel == "rowblock":
        assert K == C
        depth_s, depth_q, div = 16, 28, 0.0
    else:
        if K % 256 == 0 and K <= 1024:            # float4 form: (a + b) + (c + d) resp. (a a + b b) + (c c + d d), added to the lane's sum, the tree
            depth_s, depth_q, div = K // 256 + 8, K // 256 + 9, 1.0
        else:                                     # one value per lane and pass, the tree
            depth_s, depth_q, div = (K + 63) // 64 + 6, (K + 63) // 64 + 7, 1.0
    e_mean = depth_s * U32 * sum_abs / K + div * U32 * mean.abs()
    e_d = e_mean + U32 * d.abs()
    Q = ((d.abs() + e_mean) ** 2).sum(1, keepdim=True)
    e_q = (depth_q + 2.1) * U32 * Q + K * e_mean ** 2
    d_r = 0.5 * (e_q / K + div * U32 * var) / (var + eps) + 3.0 * U32
    e_y = d.abs() * rstd * d_r + rstd * e_d + U32 * y.abs()
    if kernel == "rowblock":
        mul, add = w * sc, b * sc + sh
        a = y * mul + add
        e_mul = (2.0 * U32 * mul.abs()) if scale is not None else 0.0 * mul
        e_add = (2.0 * U32 * (b * sc).abs() + U32 * add.abs()) if scale is not None else 0.0 * add
        e_a = mul.abs() * e_y + y.abs() * e_mul + e_add + U32 * (y * mul).abs() + U32 * a.abs()
    else:
        a, e_a = y, e_y
        if ln_w is not None:
            a1 = a * w + b
            e_a = w.abs() * e_a + U32 * (a * w).abs() + U32 * a1.abs()
            a = a1
        if scale is not None:
            a2 = a * sc + sh
            e_a = sc.abs() * e_a + 2.0 * U32 * (a * sc).abs() + U32 * a2.abs()
            a = a2
    return a, e_a * (1.0 + 1e-3)                      # (second-order terms)


def ln_band(X, dt, eps, ln_w=None, ln_b=None, shift=None, scale=None, rpg=1, kernel="rowblock"):
    """As gemm_ref.ln_operand: (a16, amb, bound) -- the correctly rounded 16-bit LayerNorm output (dtype dt), the width
    R16(a + e_a) - R16(a - e_a) of the set of 16-bit values the kernel may store (0 for almost every element), and the bound on
    |stored - a16| (the distance from a16 to the farther end of that set)."""
    a, e_a = ln_model(X, eps, ln_w, ln_b, shift, scale, rpg, kernel)
    a16 = r16(a, dt)
    hi, lo = r16(a + e_a, dt), r16(a - e_a, dt)
    return a16.to(dt), hi - lo, torch.maximum(hi - a16, a16 - lo)


def ambiguous_share(amb):
    return float((amb > 0).double().mean())


# ---- projections ----------------------------------------------------------------------------------------------------------------------

def projection(hb16, w16, bias, amb=None):
    """(reference, bound) of R16(hb W^T + b), K = 512; amb: the LayerNorm ambiguity of hb (ln_band) when hb is not the kernel's own."""
    a_err = None if amb is None else amb @ w16.double().abs().T
    return G.model(hb16, w16, bias, G.EPI_STORE_16, a_err=a_err)


def _gelu_rb(pre, e):
    """(gelu, E): rb_gelu_tanh of a pre-activation known to within e."""
    g = G.gelu_tanh(pre)
    u = SQRT_2_PI * (pre + 0.044715 * pre ** 3)
    s = torch.sigmoid(2.0 * u)
    rel = ((1.0 - s) * (12.0 * u.abs() + 2.0) + 4.0) * U32
    return g, GELU_LIP * e + g.abs() * rel


def hidden_units(hb16, wfc1, b_fc1, amb=None):
    """(reference, bound, h_lo, h_hi) of h = R16(gelu(hb Wfc1^T + b)): the bound is on |stored - R16-free gelu| as gemm_ref's GELU_16; h_lo, h_hi
    are the ends of the set of 16-bit values the kernel may hold."""
    dt = hb16.dtype
    a, w = hb16.double(), wfc1.double()
    b = torch.zeros(w.shape[0], dtype=torch.float64) if b_fc1 is None else b_fc1.double()
    pre = a @ w.T + b
    e = accumulation_error(a.shape[1], a.abs() @ w.abs().T, b.abs())
    if amb is not None:
        e = e + amb @ w.abs().T
    g, E = _gelu_rb(pre, e)
    lo, hi = r16(g - E, dt), r16(g + E, dt)
    return g, torch.maximum((hi - g).abs(), (lo - g).abs()), lo, hi                    # (= _round_bound(g, E, dt))


def mlp_update(x1, hb16, amb, wfc1, b_fc1, wfc2, b_fc2, gate_m, rpg):
    """(reference, bound) of x1 + g_m (h Wfc2^T + b_fc2) with h from the LayerNorm band (hb16, amb) of x1.
    Width on the data of test_rowblock_launch_equals_the_unfused_launches (M = 96, hidden 2048): median bound 4.8e-4 (bf16) / 9.7e-4 (fp16)
    against 1.2e-5 of fp32 noise alone and the 7e-4 / 1.3e-3 that gemm_ref.ln_operand's band gives (tests/test_rowblock_ref.py prints them);
    2.7e-4 / 4.5e-4 at hidden 512.  A dropped k-step of mlp.0 or mlp.2 and a skipped or doubled slice are outside it in 50 .. 95 % of the
    elements; a single hidden unit one 16-bit step off is inside it (the hidden-unit probe holds that stage)."""
    dt = hb16.dtype
    g, _, lo, hi = hidden_units(hb16, wfc1, b_fc1, amb)
    h = r16(g, dt)
    h_amb = torch.maximum(hi - h, h - lo)
    return G.model(h.to(dt), wfc2, b_fc2, G.EPI_RESID_F32, gate=gate_m, rpg=rpg, x0=x1, a_err=h_amb @ wfc2.double().abs().T)


# ---- temporal section --------------------------------------------------------------------------------------------------------------------

def token_rows(B, T, N, rpg):
    """Stream rows of the (sample, frame, token) grid, (B * T * N,) in that order: sample * rpg + frame * N + token.  The other rows of a group
    (rpg - T * N of them) are its padding = the phantom tokens of its last block."""
    b, f, n = torch.meshgrid(torch.arange(B), torch.arange(T), torch.arange(N), indexing="ij")
    return (b * rpg + f * N + n).reshape(-1)


def c32(scale):
    """scale * log2 e as rowblock_launch forms it in fp32."""
    return float(torch.tensor(scale, dtype=torch.float32) * torch.tensor(LOG2E, dtype=torch.float32))


def _interval16(p, E, dt):
    """(R16(p), largest distance from it to a 16-bit value the kernel may hold) for an fp32 value within E of p."""
    c = r16(p, dt)
    return c, torch.maximum((r16(p + E, dt) - c).abs(), (r16(p - E, dt) - c).abs())


def _rms16(x, dx, g, dt):
    """R16(x / |x| sqrt(32) g) over the last dimension (32) of operands known to within dx, and its ambiguity: first-order propagation of dx
    (d(x_i / |x|) = dx_i / |x| - x_i (x . dx) / |x|^3; 5 % for the second order: |dx| / |x| <= 2^-8) plus 11 U |a| for the fp32 arithmetic: the
    sum of squares has 8 squares and 7 adds per lane and two exchanges (depth 11 at most, half of it in the root), v_rsq_f32 one ulp (2 U), the
    products with sqrt(32), the value and the gain one rounding each: 5.5 + 2 + 3 (attn_ref counts (D / 2 + 8) U = 24 U for attn.hip's form)."""
    if g is None:
        return x, dx
    nrm = x.norm(dim=-1, keepdim=True).clamp_min(1e-12)
    gg = g.double().reshape(1, 1, -1, 1, 32).abs() * math.sqrt(32.0)
    a = x / nrm * g.double().reshape(1, 1, -1, 1, 32) * math.sqrt(32.0)
    first = gg * (dx / nrm + x.abs() * (x.abs() * dx).sum(-1, keepdim=True) / nrm ** 3)
    return _interval16(a, 1.05 * first + 11.0 * U32 * a.abs(), dt)


def temporal_update(x1, d):
    """(rows, reference, bound) of the stream after the temporal section, x1 + g_t (o Wout^T + b_out), on the token rows of the launch.
    x1 (M, 512): the kernel's own phase-1 stream (the launch with t_gate = 0).  d: the case (T, N, B, rpg, ln1, wqkv (1536, 512) rows
    [q | k | v], bqkv, gq, gk, t_scale, wout, bout, t_gate).  Interval arithmetic, in the order of the kernel:
      hb: LayerNorm band of x1;  q, k, v = R16(hb W^T + b): gemm_ref's accumulation error + amb |W|^T -> (value, ambiguity);  RMS norm: _rms16;
      s = q . k: (32 / 16 + 2) U sum |q k| for the one MFMA + the operands' ambiguity;  m = max over the token's T keys, off by at most the largest
      score error;  argument fl(fl(s c) - fl(m c)): E = c (e_s + e_m) + 2 U (|s c| + |m c|) + U |arg|;  p = 2^arg by v_exp_f32 (2 U): relative
      e = 2^E (1 + 2 U) - 1;  P in [R16(p (1 - e)), R16(p (1 + e))], and 0 where the fp16 store may flush (p below 2^-14);  l: fp32 sum of the
      unrounded p over at most 12 adds per lane and two exchanges: sum p e + 16 U l;  N = sum P v by two MFMAs: the ambiguity of P and v +
      6 U sum P |v|;  o = R16(N rcp(l)): (E_N + |o| E_l) / (l - E_l) + 3 U |o|;  to_out: gemm_ref RESID with a_err = o_amb |Wout|^T.
    Width on the data of tests/test_rowblock_temporal_gpu.py (tests/test_rowblock_ref.py prints it): median bound 8.5e-2 (bf16) / 6.5e-2 (fp16)
    at T = 6 -- a worst case that is far from the 1e-5 of fp32 noise: one ambiguous LayerNorm output in 300 makes about a tenth of the q / k / v
    elements ambiguous by one 16-bit step, and the interval method adds their effects linearly through the scores, P, o and |Wout|.  At that
    width a key admitted, dropped or paired with the wrong v (effect 0.8 .. 0.9), a dropped k-step of to_out and a row written to the wrong
    place are outside the bound in the rows they touch; rounding-level faults of the interior (l from rounded P, a truncating pack of P or o,
    exchanged gains) are inside it and are held by the attention-output probe instead (check_attention_probe), which resolves P, l and o to
    single 16-bit steps: 0.4 .. 2 % (bf16) / 3 .. 13 % (fp16) of its outputs may hold more than one 16-bit value without gains, up to 16 % /
    64 % with RMS gains at T = 24 (the fp32 norm leaves a normalised q or k element in 1500 (bf16) / 200 (fp16) ambiguous, and 24 x 32 of
    them meet in every softmax).  Its second form (make_temporal_probe(real_qkv=True): eight random entries per row of to_qkv) rounds q, k
    and v genuinely; 17 % (bf16) / 81 % (fp16) of its outputs may then hold more than one value at T = 6, and a truncating pack of q, k or v is
    still outside the bound in every row of the token it acts on."""
    rows, X, o16, do, back = _temporal_attention(x1, d)
    ref, bnd = G.model(back(o16).to(d["dt"]), d["wout"], d.get("bout"), G.EPI_RESID_F32, gate=d.get("t_gate"), rpg=d["T"] * d["N"], x0=X,
                       a_err=back(do) @ d["wout"].double().abs().T)
    return rows, ref, bnd


def _temporal_attention(x1, d):
    """(token rows, their x1, R16(o) and its ambiguity as (B, N, H, T, 32), the map back to rows) -- see temporal_update."""
    dt, T, N, B, rpg = d["dt"], d["T"], d["N"], d["B"], d["rpg"]
    rows = token_rows(B, T, N, rpg)
    X = x1[rows]
    a16, amb, _ = ln_band(X, dt, d.get("eps", 1e-6), *_ln_args(d.get("ln1")), rpg=T * N)
    a, w = a16.double(), d["wqkv"].double()
    b = torch.zeros(3 * C, dtype=torch.float64) if d.get("bqkv") is None else d["bqkv"].double()
    pre = a @ w.T + b
    e = accumulation_error(C, a.abs() @ w.abs().T, b.abs()) + amb @ w.abs().T
    x16, dx = _interval16(pre, e, dt)
    heads = lambda t, i: t.view(B, T, N, 3, C // 32, 32)[:, :, :, i].permute(0, 2, 3, 1, 4)          # (B, N, H, T, 32)
    q, dq = _rms16(heads(x16, 0), heads(dx, 0), d.get("gq"), dt)
    k, dk = _rms16(heads(x16, 1), heads(dx, 1), d.get("gk"), dt)
    v, dv = heads(x16, 2), heads(dx, 2)
    c = c32(d.get("t_scale") or 32 ** -0.5)
    kT, dkT = k.transpose(-1, -2), dk.transpose(-1, -2)
    s = q @ kT
    big = (q.abs() + dq) @ (kT.abs() + dkT)
    e_s = dq @ kT.abs() + q.abs() @ dkT + dq @ dkT + 4.0 * U32 * big
    m = s.max(-1, keepdim=True).values
    e_m = e_s.max(-1, keepdim=True).values
    arg = (s - m) * c
    E = c * (e_s + e_m) + 2.0 * U32 * c * (s.abs() + m.abs()) + U32 * arg.abs()
    p = torch.exp2(arg)
    ep = torch.exp2(E) * (1.0 + 2.0 * U32) - 1.0
    P = r16(p, dt)
    lo, hi = r16(p * (1.0 - ep), dt), r16(p * (1.0 + ep), dt)
    if dt == torch.float16:
        lo = torch.where(p * (1.0 - ep) < 2.0 ** -14, torch.zeros_like(lo), lo)
    dP = torch.maximum(hi - P, P - lo)
    l = p.sum(-1, keepdim=True)
    E_l = (p * ep).sum(-1, keepdim=True) + 16.0 * U32 * l
    Nn = P @ v
    E_N = dP @ v.abs() + (P + dP) @ dv + 6.0 * U32 * (P @ v.abs())
    o = Nn / l
    E_o = (E_N + o.abs() * E_l) / (l - E_l) + 3.0 * U32 * o.abs()
    o16, do = _interval16(o, E_o, dt)
    back = lambda t: t.permute(0, 3, 1, 2, 4).reshape(B * T * N, C)                                  # (B, T, N, H * 32)
    return rows, X, o16, do, back


def check_attention_probe(d, x):
    """The attention-output probe (make_temporal_probe): rows whose LayerNorm output is unambiguous (every row a signed permutation of one
    vector of 16-bit values with mean 0, ln_w = its standard deviation: hb IS that row, in the middle of its rounding cell), gate1 = 0 (x1 = x0
    exactly), Wout = identity, b_out = 0, t_gate = 1: x = x0 + o, one fp32 rounding away from the 16-bit attention output itself.  Bound: the
    ambiguity of o from the fp32 arithmetic alone (q / k / v are ambiguous only where their own accumulation error crosses a rounding
    boundary) + 2 U (|x0| + |o|).  Returns ((mask, worst), share of o elements whose interval spans more than one 16-bit value, LayerNorm share)."""
    rows, X, o16, do, back = _temporal_attention(d["x0"], d)
    _, amb, _ = ln_band(X, d["dt"], d.get("eps", 1e-6), *_ln_args(d.get("ln1")), rpg=d["T"] * d["N"])
    o, e = back(o16), back(do)
    ref = X.double() + o
    bnd = e + 2.0 * U32 * (X.double().abs() + o.abs() + e)
    return _stage(x[rows], ref, bnd), float((e > 0).double().mean()), ambiguous_share(amb)


def check_temporal(d, x1, x, out3):
    """{stage: (mask, worst)} of a temporal launch on its token rows (padding rows = phantom tokens are read by nobody: finite is all that is
    asked of them); x1 = the x of the same launch with t_gate = 0."""
    rows = token_rows(d["B"], d["T"], d["N"], d["rpg"])
    pad = torch.ones(d["M"], dtype=torch.bool)
    pad[rows] = False
    assert torch.isfinite(x[pad]).all() and torch.isfinite(out3[pad].float()).all() and torch.isfinite(x1[pad]).all()
    rs = d["x0"][rows]
    ref, bnd = stream_update(rs, d["a"][rows], d["w1"], d.get("b1"), d.get("gate1"), d["T"] * d["N"])
    res = {"x1": _stage(x1[rows], ref, bnd)}
    _, ref, bnd = temporal_update(x1, d)
    res["x"] = _stage(x[rows], ref, bnd)
    res["x_bound_median"] = float(bnd.median())
    a16, amb, _ = ln_band(x[rows], d["dt"], d.get("eps", 1e-6), *_ln_args(d.get("t_ln")), rpg=d["T"] * d["N"])
    res["amb_share"] = ambiguous_share(amb)
    ref, bnd = projection(a16, d["w3"], d.get("b3"), amb)
    res["out3"] = _stage(out3[rows], ref, bnd)
    return res


# ---- gvf_cast_pad ----------------------------------------------------------------------------------------------------------------------

def cast_model(v, dt, act):
    """(reference, bound) of gvf_cast_pad's R16(act(v)).  act 0: the cast alone, exact (bound = the rounding itself, nothing else).  act 1:
    SiLU as v / (1 + __expf(-v)): the exponential's argument -v log2 e carries one rounding (relative |v| ln2 ... counted as 2 |v| U of e),
    __expf about 2 ulp (4 U), 1 + e one rounding, the IEEE division one: relative ((1 - s)(2 |v| + 4) + 3) U.  Where __expf overflows to
    infinity (v < -88) the kernel stores v / inf = -0 against an exact value of at most 5.5e-37 in magnitude (a bf16 subnormal at worst): the
    whole value is allowed as error there, and 2^-126 everywhere for an fp32 quotient that is flushed."""
    x = v.double()
    if act == 0:
        return x, _round_bound(x, torch.zeros_like(x), dt)
    s = torch.sigmoid(x)
    g = x * s
    E = g.abs() * ((1.0 - s) * (2.0 * x.abs() + 4.0) + 3.0) * U32 + 2.0 ** -126 + g.abs() * (x < -88.0)
    return g, _round_bound(g, E, dt)


# ---- whole launches, stage by stage -------------------------------------------------------------------------------------------------------
# A case is a dict of CPU tensors: dt, M, rpg, x0 (M, 512) fp32, a (M, K1) / w1 (512, K1) 16-bit or None, b1, gate1 (groups, >= 512), x_in / period,
# in_x / in_wt / in_b, ln1 (dict of ln_w, ln_b, shift, scale), eps, hidden, wfc1, bfc1, wfc2, bfc2, gate_m, ln2, w3 (N3, 512), b3.  Missing = None.

def _ln_args(ln):
    ln = ln or {}
    return ln.get("ln_w"), ln.get("ln_b"), ln.get("shift"), ln.get("scale")


def _stage(out, ref, bnd):
    assert torch.isfinite(ref).all() and torch.isfinite(bnd).all(), "a case whose reference or bound is not finite checks nothing"
    d = (out.double() - ref).abs()
    bad = ~(d <= bnd)                                  # NaN counts as outside (as gemm_ref.excess, which this is, keeping the mask)
    ratio = d.div_(bnd.clamp_min(1e-300))
    return bad, float(torch.nan_to_num(ratio, nan=float("inf")).max()) if ratio.numel() else 0.0


def check_phase1(d, x):
    """The stream after the first update (a plain launch's x; an MLP / temporal launch's x with a zero second gate) against fp64 of the inputs."""
    rs = residual_source(d["x0"], d.get("x_in"), d.get("period", 0), d["rpg"])
    ref, bnd = stream_update(rs, d.get("a"), d.get("w1"), d.get("b1"), d.get("gate1"), d["rpg"], d.get("in_x"), d.get("in_wt"), d.get("in_b"))
    return _stage(x, ref, bnd)


def check_ln_projection(d, ln, x, hb, out3, res):
    """hb against the LayerNorm band of the kernel's x, out3 against the projection of the kernel's hb (or of the band when hb is None)."""
    dt = d["dt"]
    a16, amb, bnd_hb = ln_band(x, dt, d.get("eps", 1e-6), *_ln_args(ln), rpg=d["rpg"])
    res["amb_share"] = ambiguous_share(amb)
    if hb is not None:
        res["hb"] = _stage(hb, a16.double(), bnd_hb)
    if out3 is not None:
        ref, bnd = projection(hb, d["w3"], d.get("b3")) if hb is not None else projection(a16, d["w3"], d.get("b3"), amb)
        res["out3"] = _stage(out3, ref, bnd)
    return res


def check_plain(d, x, hb=None, out3=None):
    """{stage: (mask of elements outside the bound, worst |err| / bound)} of a launch without MLP / temporal section."""
    return check_ln_projection(d, d.get("ln1"), x, hb, out3, {"x": check_phase1(d, x)})


def check_mlp(d, x1, x, hb=None, out3=None):
    """As check_plain for an MLP launch; x1 = the x of the same launch with gate_m = 0."""
    res = {"x1": check_phase1(d, x1)}
    a16, amb, _ = ln_band(x1, d["dt"], d.get("eps", 1e-6), *_ln_args(d.get("ln1")), rpg=d["rpg"])
    ref, bnd = mlp_update(x1, a16, amb, d["wfc1"], d.get("bfc1"), d["wfc2"], d.get("bfc2"), d.get("gate_m"), d["rpg"])
    res["x"] = _stage(x, ref, bnd)
    res["x_bound_median"] = float(bnd.median())
    if hb is None and out3 is None:
        return res
    return check_ln_projection(d, d.get("ln2"), x, hb, out3, res)


def check_hidden_probe(d, x):
    """The probe launch (x0 = 0, no closing projection or a zero gate1, hidden = 512, Wfc2 = identity, b_fc2 = 0, gate_m = 1): x IS the hidden
    units.  The LayerNorm of a zero row is `add` exactly (d = 0, y = 0, fl(0 * mul + add) = add), one rounding to 16 bit: no ambiguity
    beyond e_add."""
    z = torch.zeros_like(d["x0"])
    a16, amb, _ = ln_band(z, d["dt"], d.get("eps", 1e-6), *_ln_args(d.get("ln1")), rpg=d["rpg"])
    ref, bnd, _, _ = hidden_units(a16, d["wfc1"], d.get("bfc1"), amb)
    return _stage(x, ref, bnd)


# ---- test data ----------------------------------------------------------------------------------------------------------------------------

def make_case(dt, M=96, rpg=48, K1=128, hidden=0, N3=512, ln1="adaln", ln2="adaln", gate1=True, seed=0, in_cin=0, x_in=False, period=0, b1=True, adv=False, lda_pad=0, in_b=True, b3=True):
    """The data of test_rowblock_launch_equals_the_unfused_launches (tests/test_dit_gpu.py), as a rowblock_ref case.  adv: adversarial rows in
    the first block (a common offset of 100 standard deviations; constant rows; one huge element), scale = -1 (mul = 0) in half of the
    columns of the last group and a zero gate1 in the other half."""
    g = torch.Generator().manual_seed(1000 * seed + M + N3 + hidden)
    groups = M // rpg
    rn = lambda *s: torch.randn(s, generator=g)
    mod = rn(groups, 6 * C + 8) * 0.3
    lw, lb = 1 + 0.1 * rn(C), 0.1 * rn(C)
    lns = {"adaln": lambda o: dict(shift=mod[:, o:], scale=mod[:, o + C:]), "affine": lambda o: dict(ln_w=lw, ln_b=lb),
           "both": lambda o: dict(ln_w=lw, ln_b=lb, shift=mod[:, o:], scale=mod[:, o + C:]), "none": lambda o: {}}
    d = dict(dt=dt, M=M, rpg=rpg, eps=1e-6, x0=rn(M, C) * 2 + 0.5, mod=mod, hidden=hidden, lda_pad=lda_pad)
    if adv:
        d["x0"][0:8] = d["x0"][0:8] + 200.0
        d["x0"][8:12] = torch.tensor([3.0, -0.37, 0.0, 12.0])[:, None]        # (|c| rstd e_mean = 1e-3 |c|: a constant of 1e3 would make the band vacuous)
        d["x0"][12:16, 5::97] = 1e4
        mod[-1, 2 * C:2 * C + C // 2] = -1.0
        mod[-1, 4 * C:4 * C + C // 2] = -1.0
        mod[-1, C // 2:C] = 0.0
    if K1:
        d.update(a=rn(M, K1).to(dt), w1=(rn(C, K1) / math.sqrt(K1)).to(dt), b1=0.1 * rn(C) if b1 else None, gate1=mod[:, 0:] if gate1 else None)
    if in_cin:
        d.update(in_x=rn(M, in_cin), in_wt=rn(in_cin, C) / math.sqrt(in_cin), in_b=0.1 * rn(C) if in_b else None)
    if x_in:
        d.update(x_in=rn(groups * period, C) * 2, period=period)
    d["ln1"] = lns[ln1](C)
    if hidden:
        d.update(wfc1=(rn(hidden, C) / math.sqrt(C)).to(dt), wfc2=(rn(C, hidden) / math.sqrt(hidden)).to(dt), bfc1=0.1 * rn(hidden), bfc2=0.1 * rn(C),
                 gate_m=mod[:, 5 * C:], ln2=lns[ln2](3 * C))
    if N3:
        d.update(w3=(rn(N3, C) / math.sqrt(C)).to(dt), b3=0.1 * rn(N3) if b3 else None)
    return d


def make_probe(dt, groups=40, seed=0):
    """The hidden-unit probe: x = 0, no closing projection, hidden = 512, Wfc2 = identity, b_fc2 = 0, gate_m = 1; one distinct row per group of
    48, its adaLN shift scaled so that the pre-activations spread from about 1e-3 to about 8 in magnitude."""
    g = torch.Generator().manual_seed(77 + seed)
    M = groups * BM
    mag = torch.logspace(-3, math.log10(8.0), groups)[:, None]
    shift = torch.randn((groups, C), generator=g) * mag
    scale = torch.randn((groups, C), generator=g) * 0.3
    wfc1 = (torch.randn((C, C), generator=g) / math.sqrt(C)).to(dt)
    bfc1 = torch.randn((C,), generator=g) * 1e-3
    return dict(dt=dt, M=M, rpg=BM, eps=1e-6, x0=torch.zeros((M, C)), ln1=dict(shift=shift, scale=scale), hidden=C, wfc1=wfc1, bfc1=bfc1,
                wfc2=torch.eye(C).to(dt), bfc2=None, gate_m=None, want_hb=False)


def make_temporal(dt, B, T, N, rms=True, adaln=True, seed=0, gate=True, t_ln="affine"):
    """The data of tests/test_rowblock_temporal_gpu.py as a case: groups of rows_per_group = whole 48-row blocks of 48 / T tokens, the token
    rows in front, finite padding behind."""
    g = torch.Generator().manual_seed(1000 * T + N + seed)
    tpb = BM // T
    rpg = (N + tpb - 1) // tpb * BM
    M = B * rpg
    rn = lambda *s, sc=1.0: torch.randn(s, generator=g) * sc
    mod = rn(B, 9 * C, sc=0.3)
    lw, lb = 1 + 0.1 * rn(C), 0.1 * rn(C)
    return dict(dt=dt, M=M, B=B, T=T, N=N, rpg=rpg, eps=1e-6, x0=rn(M, C) * 2 + 0.5, mod=mod, a=rn(M, C).to(dt), w1=rn(C, C, sc=1 / math.sqrt(C)).to(dt),
                b1=rn(C, sc=0.1), gate1=mod[:, 0:] if adaln else None, ln1=dict(shift=mod[:, C:], scale=mod[:, 2 * C:]) if adaln else dict(ln_w=lw, ln_b=lb),
                wqkv=rn(3 * C, C, sc=1.5 / math.sqrt(C)).to(dt), bqkv=rn(3 * C, sc=0.1), wout=rn(C, C, sc=1 / math.sqrt(C)).to(dt), bout=rn(C, sc=0.1),
                gq=(1 + 0.2 * rn(C)) if rms else None, gk=(1 + 0.2 * rn(C)) if rms else None, t_gate=mod[:, 3 * C:] if gate else None,
                t_ln=dict(**(dict(ln_w=lw, ln_b=lb) if t_ln in ("affine", "both") else {}), **(dict(shift=mod[:, 4 * C:], scale=mod[:, 5 * C:]) if t_ln in ("adaln", "both") else {})),
                w3=rn(C, C, sc=1 / math.sqrt(C)).to(dt), b3=rn(C, sc=0.1), t_scale=32 ** -0.5)


def make_temporal_probe(dt, B, T, N, rms=True, seed=0, real_qkv=False):
    """See check_attention_probe.  real_qkv: a to_qkv of eight random entries per row, with make_temporal's bias, so that q, k and v are genuinely rounded -- ambiguous
    only where their own accumulation bound crosses a rounding boundary; the scores are then less sharp and o is resolved to one or two 16-bit
    steps instead of one."""
    d = make_temporal(dt, B, T, N, rms=rms, adaln=False, seed=seed, gate=False)
    g = torch.Generator().manual_seed(4242 + seed + T)
    z = torch.randn((C // 2,), generator=g)
    z = (z + 0.25 * torch.sign(z)).to(dt).float()                 # no tiny values: every element sits well inside its rounding cell
    base = torch.cat([z, -z])
    # to_qkv = three signed permutations and no bias: q, k, v ARE 16-bit values (+- h_i, exact in the fp32 accumulator and far from every rounding
    # boundary -- a sum of two would sit on ties), so the scores are sharp and P, l, o are resolved to single 16-bit steps.  (The rounding of
    # q / k / v themselves is what real_qkv is for.)
    wq = torch.zeros((3 * C, C))
    for i in range(3):
        wq[torch.arange(C) + C * i, torch.randperm(C, generator=g)] = torch.where(torch.rand((C,), generator=g) < 0.5, -1.0, 1.0)
    if real_qkv:                                  # eight random entries per row: sum |a w| / |a . w| is about 3 instead of 16, a sixth of the ambiguity
        keep = torch.zeros((3 * C, C), dtype=torch.bool)
        keep[torch.arange(3 * C)[:, None], torch.stack([torch.randperm(C, generator=g)[:8] for _ in range(3 * C)])] = True
        d["wqkv"] = (torch.randn((3 * C, C), generator=g) * (1.5 / math.sqrt(8.0)) * keep).to(dt)
    else:
        d.update(wqkv=wq.to(dt), bqkv=None)
    d["x0"] = torch.stack([base[torch.randperm(C, generator=g)] for _ in range(d["M"])])
    sd = float(torch.sqrt((base.double() ** 2).mean() + d["eps"]))
    d.update(ln1=dict(ln_w=torch.full((C,), sd), ln_b=torch.zeros(C)), gate1=torch.zeros((B, C)), mod=None, wout=torch.eye(C).to(dt), bout=None, t_gate=None)
    return d
