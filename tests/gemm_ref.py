"""fp64 reference and per-element error bound of the GEMM family (csrc/gemm.hip, csrc/gemm8.hip; include/gvf_dit.h).

reference() computes, on the CPU in float64, what an epilogue of gvf_gemm computes from the same 16-bit operands: every product of two
16-bit values is exact in float64, and a sum of K <= 2^20 of them is exact to K 2^-53 relative -- far below every term of the bound.
bound() says how far the kernel's output may lie from it, from the arithmetic the kernel does:

  * accumulation: the MFMA v_mfma_f32_16x16x32 adds 32 exact products to the fp32 accumulator per k-step, ceil(K / 32) steps; each
    step is counted as one fp32 rounding of a partial sum whose magnitude is at most S = sum_k |a_k w_k|, one more rounding adds the
    bias, and one more is slack for the MFMA's internal reduction order:
        e_acc = (ceil(K / 32) + 2) * 2^-24 * (S + |bias|)
    (measured on the MI355X, fp32 outputs of tests/test_gemm_conformance_gpu.py: |err| / bound at most 0.51 at K = 32, where the output's
    own rounding and the bias add are two of the three counted roundings, 0.11 at K = 2048, 0.03 at K = 512 -- a worst case that random-
    sign rounding errors, adding up like a square root, stay well inside);
  * fp32 epilogue arithmetic: GELU-tanh through __expf (relative (8 |u| + 6) 2^-24 for u = sqrt(2/pi)(x + 0.044715 x^3): exp's
    argument -2u is formed to ~4 ulp and __expf adds ~2 ulp; |gelu'| <= 1.13 carries e_acc through), erff in GEGLU (a few ulp: 8 2^-24
    relative to |v| (|g| + |gelu(g)|)), the residual update x0 + g v (two roundings, fused or not: 2 2^-24 (|x0| + |g v|));
  * 16-bit outputs: the kernel rounds its fp32 value, which lies within E of the exact pre-rounding value p, to nearest even.  Rounding
    is monotone, so the stored value lies in [R(p - E), R(p + E)] with R = round-to-16-bit; the bound is the distance from p to the
    farther end.  That is at most half an ulp of the output plus E (the textbook form) but exact about where the rounding may go: a
    store that truncates (or rounds the wrong way) lands outside it whenever p's fraction is on the far side of the half ulp.

Layout conventions are the kernel's: w is [N][K] (nn.Linear), the GEGLU projection's rows come in 64-row groups of 32 value rows then
their 32 gate rows (dit_ops.geglu_interleave), gate row g applies to output rows [g rpg, (g + 1) rpg).  Everything here runs on torch
CPU tensors; pass .cpu() copies of device tensors."""
import math

import torch

U32 = 2.0 ** -24                     # unit roundoff of fp32
GELU_LIP = 1.13                      # max |d/dx gelu(x)| (tanh and erf forms: 1.1289 at x = +-2.42)

EPI_STORE_16, EPI_GELU_16, EPI_STORE_F32, EPI_RESID_F32, EPI_GEGLU_16 = 0, 1, 2, 3, 4     # include/gvf_dit.h


def r16(x: torch.Tensor, dt) -> torch.Tensor:
    """The 16-bit value (as float64) the kernel stores for x: x is first an fp32 value, then rounded to nearest even in `dt`.  Monotone
    non-decreasing in x (so R(p - E) <= R(p') <= R(p + E) for every p' within E of p)."""
    return x.to(torch.float32).to(dt).to(torch.float64)


def _round_bound(p: torch.Tensor, E: torch.Tensor, dt) -> torch.Tensor:
    """Largest |R(p') - p| over fp32 values p' with |p' - p| <= E, R = rounding to `dt`; dt None: fp32 output, E itself."""
    if dt is None:
        return E
    return torch.maximum((r16(p + E, dt) - p).abs(), (r16(p - E, dt) - p).abs())


def gelu_tanh(x: torch.Tensor) -> torch.Tensor:
    return 0.5 * x * (1.0 + torch.tanh(math.sqrt(2.0 / math.pi) * (x + 0.044715 * x ** 3)))


def gelu_erf(x: torch.Tensor) -> torch.Tensor:
    return 0.5 * x * (1.0 + torch.erf(x / math.sqrt(2.0)))


def _gate_rows(gate, M, N, rpg):
    """gate (groups, >= N) -> the fp64 (M, N) matrix whose row m is gate[m // rpg]; None -> ones."""
    if gate is None:
        return torch.ones((M, N), dtype=torch.float64)
    idx = torch.arange(M) // rpg
    return gate[:, :N].double()[idx]


def accumulation_error(K: int, S: torch.Tensor, bias_abs: torch.Tensor) -> torch.Tensor:
    """e_acc of the module docstring: fp32 accumulation of ceil(K / 32) MFMA k-steps plus the bias add (+ one for the MFMA's reduction)."""
    return ((K + 31) // 32 + 2) * U32 * (S + bias_abs)


def model(a16, w16, bias, epilogue, gate=None, rpg=1, x0=None, a_err=None):
    """(reference, bound) as float64 tensors of the output's shape (M, N) -- (M, N / 2) for GEGLU.

    a16 (M, K), w16 (N, K): the 16-bit operands (their dtype is the output's 16-bit type); bias fp32 (N,) or None; gate fp32 (groups, >= N)
    or None with rows_per_group rpg; x0 fp32 (M, N): the residual stream before a RESID_F32 update.  a_err (M, N) float64, optional: an
    extra absolute error of the accumulator (an A operand that is only known to within some amount, see ln_operand)."""
    dt = a16.dtype
    a, w = a16.double(), w16.double()
    M, K = a.shape
    N = w.shape[0]
    acc = a @ w.T
    S = a.abs() @ w.abs().T
    b = torch.zeros(N, dtype=torch.float64) if bias is None else bias.double()
    pre = acc + b
    e = accumulation_error(K, S, b.abs())
    if a_err is not None:
        e = e + a_err
    if epilogue == EPI_STORE_16:
        return pre, _round_bound(pre, e, dt)
    if epilogue == EPI_STORE_F32:
        return pre, e
    if epilogue == EPI_GELU_16:
        g = gelu_tanh(pre)
        u = math.sqrt(2.0 / math.pi) * (pre + 0.044715 * pre ** 3)
        E = GELU_LIP * e + g.abs() * (8.0 * u.abs() + 6.0) * U32
        return g, _round_bound(g, E, dt)
    if epilogue == EPI_RESID_F32:
        assert x0 is not None
        gm = _gate_rows(gate, M, N, rpg)
        x = x0.double()
        ref = x + gm * pre
        return ref, gm.abs() * e + 2.0 * U32 * (x.abs() + (gm * pre).abs())
    if epilogue == EPI_GEGLU_16:
        assert N % 64 == 0
        q = pre.view(M, N // 64, 2, 32)
        v, g = q[:, :, 0].reshape(M, N // 2), q[:, :, 1].reshape(M, N // 2)
        ev = e.view(M, N // 64, 2, 32)[:, :, 0].reshape(M, N // 2)
        eg = e.view(M, N // 64, 2, 32)[:, :, 1].reshape(M, N // 2)
        # value and gate are rounded to the operand type first (the rounding the stored projection would have had): the kernel's v16 lies
        # in [R(v - ev), R(v + ev)], g16 likewise; the reference takes the correctly rounded ones
        v16, g16 = r16(v, dt), r16(g, dt)
        dv = r16(v + ev, dt) - r16(v - ev, dt)
        dg = r16(g + eg, dt) - r16(g - eg, dt)
        gel = gelu_erf(g16)
        ref = v16 * gel
        vmax = torch.maximum(r16(v + ev, dt).abs(), r16(v - ev, dt).abs())
        E = dv * (gel.abs() + GELU_LIP * dg) + vmax * GELU_LIP * dg + 8.0 * U32 * vmax * (g16.abs() + dg + gel.abs())
        return ref, _round_bound(ref, E, dt)
    raise ValueError(f"epilogue {epilogue}")


def reference(a16, w16, bias, epilogue, gate=None, rpg=1, x0=None):
    return model(a16, w16, bias, epilogue, gate, rpg, x0)[0]


def bound(a16, w16, bias, epilogue, gate=None, rpg=1, x0=None):
    return model(a16, w16, bias, epilogue, gate, rpg, x0)[1]


def excess(out: torch.Tensor, ref: torch.Tensor, bnd: torch.Tensor):
    """(number of elements outside the bound, largest |out - ref| / bound over the elements with a non-zero bound)."""
    d = (out.double() - ref).abs()
    bad = ~(d <= bnd)                                  # NaN counts as outside
    ratio = d / bnd.clamp_min(1e-300)
    return int(bad.sum()), float(torch.nan_to_num(ratio, nan=float("inf")).max()) if ratio.numel() else 0.0


# ---- row statistics of the residual epilogue (gvf_gemm_resid_stats) -------------------------------------------------------------------

def stats_bound(x: torch.Tensor):
    """Bounds on |sum_parts(sum) - sum_n x_n| and |sum_parts(sq) - sum_n x_n^2| for a row x of the UPDATED fp32 stream: each part is a 64-column
    slice summed by a depth-6 tree (two adds in a lane, four shuffles), one more rounding for the squares; the host adds the parts in fp64."""
    xd = x.double()
    return 6.0 * U32 * xd.abs().sum(-1), 7.0 * U32 * (xd * xd).sum(-1)


# ---- the LayerNorm-folded A operand of gvf_gemm_ln ------------------------------------------------------------------------------------

def ln_operand(X, n_part, dt, eps, ln_w=None, ln_b=None, shift=None, scale=None, rpg=1):
    """(a16, amb): the correctly rounded 16-bit operand R(LN(X) s + t) (fp64 statistics of the fp32 stream X (M, K)) and, per element, the
    width R(a + eps_a) - R(a - eps_a) of the set of 16-bit values the kernel's fp32 computation may round to.  eps_a follows the kernel's
    arithmetic (csrc/gemm.hip, ALN): row sums from n_part partial (sum, sum of squares) pairs -- depth-6 trees, then added in fp32 --,
    mean = sum / K, var = sq / K - mean^2, rstd = rsqrtf(var + eps) (~1 ulp), y = fma(x, rstd, -mean rstd), z = fma(y, s, t) with
    s = ln_w (1 + scale), t = ln_b (1 + scale) + shift in fp32.  Almost every amb is 0; the rest are one 16-bit step."""
    x = X.double()
    M, K = x.shape
    mean = x.mean(1, keepdim=True)
    var = ((x - mean) ** 2).mean(1, keepdim=True)
    rstd = 1.0 / torch.sqrt(var + eps)
    s = torch.ones((1, K), dtype=torch.float64) if ln_w is None else ln_w.double()[None]
    t = torch.zeros((1, K), dtype=torch.float64) if ln_b is None else ln_b.double()[None]
    es = 0.0 * s
    et = 0.0 * t
    if scale is not None:
        g = torch.arange(M) // rpg
        sc = 1.0 + scale.double()[g, :K]
        sh = shift.double()[g, :K]
        s, t = s * sc, t * sc + sh
        es = 2.0 * U32 * s.abs()
        et = 3.0 * U32 * (t.abs() + sh.abs())
    y = (x - mean) * rstd
    a = y * s + t
    # error of the kernel's fp32 intermediates (first order; the factors are rounding counts)
    sum_abs, sq = x.abs().sum(1, keepdim=True), (x * x).sum(1, keepdim=True)
    e_mean = (7 + n_part) * U32 * sum_abs / K
    q = sq / K
    e_var = (9 + n_part) * U32 * q + 2.0 * mean.abs() * e_mean + e_mean ** 2 + 2.0 * U32 * (q + mean * mean)
    d_r = 0.5 * e_var / (var + eps) + 3.0 * U32                 # relative error of rstd
    e_y = (x.abs() + mean.abs()) * rstd * d_r + rstd * e_mean + 2.0 * U32 * (x.abs() + mean.abs()) * rstd
    e_a = s.abs() * e_y + y.abs() * es + et + U32 * (y * s).abs() + U32 * a.abs()
    a16 = r16(a, dt)
    amb = r16(a + e_a, dt) - r16(a - e_a, dt)
    return a16.to(dt), amb
