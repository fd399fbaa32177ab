"""fp64 reference and per-element error bound of the attention family: gvf_attn_fwd / gvf_attn_varlen_fwd (csrc/attn.hip) and the tiled
K/V caches (csrc/attn_xt.hip, csrc/attn_xt64.hip).

model() computes, on the CPU in float64, what one (sequence, head) problem of a kernel path computes from the same 16-bit operands, with the
path's own rounding points, and bound() says how far the kernel's output may lie from it.  The paths differ in exactly those points:

  path      exp2 argument a_j of key j (log2 domain)                        stored probability    denominator
  "stream"  fl(fma(s_j, c, -m_t)): s_j = q.k_j, c = fl32(scale * log2 e),     P_j = R16(2^a_j),      sum of the UNROUNDED 2^a_j,
            m_t = the running maximum of s c after key tile t (64 keys),       rescaled by            rescaled alike
            the query's own, updated once per tile                            2^(m_t - m_last)
  "small"   fl(fl(s_j c) - fl(m c)), m = max over all keys (Lk <= 32)          R16(2^a_j)             unrounded
  "kvres"   q.K'_j with K' = R16(fl32(c k)) staged once (k RMS-normalised      R16(2^a_j)             unrounded
            and rounded first when gains are given); bf16: no maximum at all;
            fp16: minus a shift = max of the scores against the first key
            tile, zero-padded keys included.  A 32-query wave whose
            denominator leaves (2^-100, 2^100) (bf16) / (2^-6, 2^15) (fp16)
            redoes its tile exactly: "stream" on K' with c = 1
  "xt",     q.K'_j against the cache of attn_pack_kv* (K' = R16(fl32(c k)),   R16(2^a_j)             fp32 sum of the ROUNDED
  "xt64"    gains folded into the one rounding); fp16 minus the first tile's                         P_j (the matrix pipe's
            maximum in the cache's key order (attn_xt's bounded mode: none).                          row sums); the exact
            Exact re-run per 256-query workgroup (xt) / 64-query wave pass                            re-run sums unrounded p
            (xt64) when the denominator leaves (l_min, 2^100): model_tiled()

q and k are RMS-normalised in fp32 when gains are given (x / max(|x|, 1e-12) * sqrt(D) * g) and rounded to 16 bit before the product; the
reference takes the correctly rounded R16(a) of the fp64 value a, and the set of 16-bit values the kernel's fp32 arithmetic may round to,
[R16(a - e_a), R16(a + e_a)] with e_a = (D / 2 + 8) 2^-24 |a|, enters the score error (almost always a single value).

The bound follows gemm_ref's interval method:

  * score / argument error E_j (absolute, fp32): the MFMA contraction over D in D / 16 steps of 16 exact products counted as
    (D / 16 + 2) 2^-24 sum_d |q_d k_d| (one rounding per step, one for the reduction order inside the MFMA, one spare), scaled by c, plus
    the error of the kernel's maximum (the same bound at the largest score, plus the rounding of m c), plus the fma / subtraction
    roundings 2^-24 |a_j|, plus the ambiguity of normalised operands;
  * stored probability: the kernel's fp32 p_j lies within a relative e_j = 2^E_j (1 + 2 2^-24) - 1 of 2^a_j (v_exp_f32: about 1 ulp), so
    the value it stores lies in [R16(p_j (1 - e_j)), R16(p_j (1 + e_j))]; the term's numerator error is the distance from R16(p_j) to the
    farther end (times the rescale), widened by the relative error of the maximum (which rescales a whole tile; it cancels between
    numerator and denominator except where it moves a rounding) and, for "stream", 4 2^-24 per rescale.  A term near no rounding boundary
    therefore contributes fp32-level slack only: a key dropped, duplicated or exchanged with non-negligible P moves the numerator far
    outside.  Probabilities in the range where the hardware may flush (fp16 below 2^-14, bf16 below 2^-125) may also be stored as zero;
  * accumulation: P.V over ceil(Lk / 16) MFMA steps and up to 2 rescales per tile, (4 n_tiles + 2 n_tiles + 3) 2^-24 sum_j P_j |v_j|;
    the denominator: 32 sequential adds per lane and tile, one per tile into the running sum, one per rescale, the lane exchange:
    (34 + 2 n_tiles) 2^-24 sum_j p_j, plus sum_j p_j e_j;
  * epilogue: o = N / L with |N' - N| <= E_N, |L' - L| <= E_L: |o' - o| <= (E_N + |o| E_L) / (L - E_L) + 3 2^-24 |o| (the reciprocal and
    the product), then the 16-bit store: the stored value lies in [R(o - E), R(o + E)] (gemm_ref._round_bound).

Operands are torch CPU tensors: q (P, Lq, D), k and v (P, Lk, D) of one 16-bit dtype (P independent problems), gains fp32 (P, D) or None.
Pass .cpu() copies of device tensors."""
import math

import torch

from gemm_ref import U32, _round_bound, excess, r16       # noqa: F401  (excess: re-exported for the tests)

KT = 64                              # keys per staged tile (csrc/attn.hip)
LOG2E = 1.4426950408889634
KVRES_RANGE = {torch.bfloat16: (2.0 ** -100, 2.0 ** 100), torch.float16: (2.0 ** -6, 2.0 ** 15)}


def c32(scale: float) -> float:
    """scale_log2e as launch_attn forms it: fp32 scale times the fp32 log2(e), rounded to fp32."""
    return float(torch.tensor(scale, dtype=torch.float32) * torch.tensor(LOG2E, dtype=torch.float32))


def rms_operand(x16: torch.Tensor, g, dt):
    """(reference, ambiguity) of the RMS-normalised operand R16(x / max(|x|, 1e-12) sqrt(D) g): the correctly rounded value of the fp64
    result and the largest distance to another 16-bit value the kernel's fp32 arithmetic may produce.  g None: x itself, no ambiguity."""
    x = x16.double()
    if g is None:
        return x, torch.zeros_like(x)
    D = x.shape[-1]
    a = x / x.norm(dim=-1, keepdim=True).clamp_min(1e-12) * math.sqrt(D) * g.double()[:, None, :]
    e = (D / 2 + 8) * U32 * a.abs()
    ref = r16(a, dt)
    return ref, torch.maximum((r16(a + e, dt) - ref).abs(), (r16(a - e, dt) - ref).abs())


def prescaled_keys(k16, gk, c, dt):
    """(K', ambiguity) of the K/V-resident kernel's staged keys: R16(fl32(c k)), k normalised and rounded first when gains are given."""
    kn, amb = rms_operand(k16, gk, dt)
    kp = r16(kn * c, dt)
    if gk is None:
        return kp, torch.zeros_like(kp)
    lo, hi = r16((kn - amb) * c, dt), r16((kn + amb) * c, dt)
    return kp, torch.maximum((hi - kp).abs(), (lo - kp).abs())


def _scores(q, qa, k, ka):
    """fp64 scores, and the fp32 error bound of the kernel's MFMA contraction over D plus the operands' ambiguity."""
    D = q.shape[-1]
    s = q @ k.transpose(-1, -2)
    S = q.abs() @ k.abs().transpose(-1, -2)
    e = (D // 16 + 2) * U32 * S
    if bool((qa > 0).any()) or bool((ka > 0).any()):
        e = e + qa @ (k.abs() + ka).transpose(-1, -2) + q.abs() @ ka.transpose(-1, -2)
    return s, e


def _tile_max(t, Lk):
    """(P, Lq, n_tiles) maximum of t over each 64-key tile."""
    nt = (Lk + KT - 1) // KT
    tp = torch.full(t.shape[:-1] + (nt * KT,), -math.inf, dtype=t.dtype)
    tp[..., :Lk] = t
    return tp.view(t.shape[:-1] + (nt, KT)).amax(-1)


def _combine(t, et, em, M_key, r, v, dt, n_tiles, eps_r, extra_arg=None, den_rounded=False):
    """(reference, bound) from the exp2 arguments t - M_key (P, Lq, Lk), their error et + em (em: the maximum's, which also rescales the
    tile), the rescale factors r of each key, V (P, Lk, D)."""
    a = t - M_key
    p = torch.exp2(a)
    delta = et + em + U32 * a.abs()
    if extra_arg is not None:
        delta = delta + extra_arg
    e = torch.expm1(math.log(2.0) * delta) + 2.0 * U32
    ed = torch.expm1(math.log(2.0) * em)
    P = r16(p, dt)
    hi = r16(p * (1.0 + e), dt) * (1.0 + ed)
    lo = r16(p * (1.0 - e), dt) * (1.0 - ed)
    dP = torch.maximum(hi - P, P - lo)
    tiny = 2.0 ** -14 if dt == torch.float16 else 2.0 ** -125
    dP = torch.where(p < tiny, torch.maximum(dP, hi), dP)             # may be flushed to zero
    dP = (dP + P * eps_r) * r
    W = P * r
    w = (P if den_rounded else p) * r
    av = v.abs()
    N = W @ v
    E_N = dP @ av + (6 * n_tiles + 3) * U32 * ((W + dP) @ av)
    L = w.sum(-1, keepdim=True)
    E_L = ((dP if den_rounded else w * (e + eps_r)) + (34 + 2 * n_tiles) * U32 * w).sum(-1, keepdim=True)
    o = N / L
    E = (E_N + o.abs() * E_L) / (L - E_L).clamp_min(1e-300) + 3.0 * U32 * o.abs()
    return o, E, L


def _running_max(t, et, Lk):
    """(M, em) per 64-key tile (P, Lq, n_tiles): the running maximum of t after each tile, and how far the kernel's fp32 maximum of the
    perturbed arguments t_j + err_j (|err_j| <= et_j) may lie from it -- between max(t - et) and max(t + et) -- plus its own rounding."""
    M = torch.cummax(_tile_max(t, Lk), dim=-1).values
    hi = torch.cummax(_tile_max(t + et, Lk), dim=-1).values
    lo = torch.cummax(_tile_max(t - et, Lk), dim=-1).values
    return M, torch.maximum(hi - M, M - lo) + U32 * M.abs()


def _stream(t, et, v, dt, Lk):
    """The running-maximum softmax of attn_fwd_kernel's tile64 on exp2 arguments t = s c (error et)."""
    nt = (Lk + KT - 1) // KT
    M, em = _running_max(t, et, Lk)                                    # (P, Lq, nt)
    M_key = M.repeat_interleave(KT, dim=-1)[..., :Lk]
    em = em.repeat_interleave(KT, dim=-1)[..., :Lk]
    r = torch.exp2(M_key - M[..., -1:])
    return _combine(t, et, em, M_key, r, v, dt, nt, 4.0 * U32 * nt)


def model(q16, k16, v16, path, scale=None, gq=None, gk=None, fallback=None):
    """(reference, bound) as float64 (P, Lq, D) of the 16-bit output.  path: "stream", "small" or "kvres" (module docstring).
    fallback (kvres only): None follows the kernel's range guard per 32-query wave; True / False force the exact / fast model."""
    dt = q16.dtype
    D = q16.shape[-1]
    Lk = k16.shape[-2]
    c = c32(D ** -0.5 if scale is None else scale)
    q, qa = rms_operand(q16, gq, dt)
    v = v16.double()
    if path in ("stream", "small"):
        k, ka = rms_operand(k16, gk, dt)
        s, es = _scores(q, qa, k, ka)
        t, et = s * c, es * c
        if path == "stream":
            o, E, _ = _stream(t, et, v, dt, Lk)
        else:
            assert D == 32 and Lk <= 32 and q16.shape[-2] <= 32
            M, em = _running_max(t, et, Lk)
            o, E, _ = _combine(t, et, em, M, torch.ones_like(t), v, dt, 1, 0.0, extra_arg=U32 * t.abs())
        return o, _round_bound(o, E, dt)
    assert path == "kvres"
    kp, ka = prescaled_keys(k16, gk, c, dt)
    t, et = _scores(q, qa, kp, ka)
    if dt == torch.float16:
        M, em = _first_tile_shift(t, et, Lk)
    else:
        M = torch.zeros(t.shape[:-1] + (1,), dtype=t.dtype)
        em = torch.zeros_like(M)
    return _max_free(t, et, em, M, v, dt, Lk, KVRES_RANGE[dt], 32, False, fallback, dt)


def _first_tile_shift(t, et, Lk):
    """The fp16 shift of the max-free paths: the maximum of each query's scores against the first key tile (keys past Lk, staged as zeros,
    score 0 and take part), and its error."""
    M, em = _running_max(t[..., :KT], et[..., :KT], min(Lk, KT))
    if Lk < KT:
        em = torch.where(M < 0.0, (M + em).clamp_min(0.0), em)
        M = M.clamp_min(0.0)
    return M, em


def _max_free(t, et, em, M, v, dt, Lk, rng, group, den_rounded, fallback, out_dt):
    """P = R16(2^(t - M)) without a running maximum; a group of `group` consecutive queries whose denominator leaves the open interval rng
    is recomputed exactly (the running-maximum model on the same arguments, unrounded denominator).  Near a threshold either may hold."""
    o_f, E_f, L = _combine(t, et, em, M, torch.ones_like(t), v, dt, (Lk + KT - 1) // KT, 0.0, den_rounded=den_rounded)
    o_x, E_x, _ = _stream(t, et, v, dt, Lk)
    lo_t, hi_t = rng
    Lq = t.shape[-2]
    nw = (Lq + group - 1) // group
    Lw = torch.nn.functional.pad(L[..., 0], (0, nw * group - Lq), value=1.0).view(L.shape[0], nw, group).nan_to_num(math.inf)
    if fallback is None:
        bad = ((Lw <= lo_t * 1.001) | (Lw >= hi_t * 0.999)).any(-1)
        sure = ((Lw <= lo_t * 0.999) | (Lw >= hi_t * 1.001)).any(-1)
        bad = bad.repeat_interleave(group, dim=-1)[:, :Lq, None]
        sure = sure.repeat_interleave(group, dim=-1)[:, :Lq, None]
    else:
        bad = sure = torch.full(L.shape, bool(fallback))
    o = torch.where(sure, o_x, o_f)
    E = torch.where(sure, E_x, torch.where(bad, torch.maximum(E_f, (o_x - o_f).abs() + E_x), E_f))
    return o, _round_bound(o, E, out_dt)


# ---- the tiled K/V caches of the cross attentions (csrc/attn_xt.hip, csrc/attn_xt64.hip) ------------------------------------------------

TILED_GROUP = {"xt": 256, "xt64": 64}       # queries that fall back together: a workgroup (attn_xt), a wave pass (attn_xt64)


def tiled_keys(k, gk, scale, dt):
    """(K', ambiguity, V') of the cache image attn_pack_kv* writes from kv rows k / v (fp32 or 16-bit, (P, L, D)): K' = R16(fl32(k c)) with
    c = fl32(scale log2 e) -- or, with gains (attn_xt), R16 of the fp32 k / |k| sqrt(D) g c: one rounding."""
    c = float(torch.tensor(scale * LOG2E, dtype=torch.float32))
    x = k.double()
    if gk is None:
        return r16(x * c, dt), torch.zeros_like(x)
    D = x.shape[-1]
    a = x / x.norm(dim=-1, keepdim=True).clamp_min(1e-12) * math.sqrt(D) * gk.double()[:, None, :] * c
    e = (D / 2 + 8) * U32 * a.abs()
    kp = r16(a, dt)
    return kp, torch.maximum((r16(a + e, dt) - kp).abs(), (r16(a - e, dt) - kp).abs())


def model_tiled(q16, k, v, path, scale=None, gq=None, gk=None, shift=None, out_f32=False, fallback=None):
    """(reference, bound) of attention_tiled (path "xt", head_dim 32) / attention_tiled64 ("xt64", head_dim 64) against the cache packed
    from kv rows k, v (P, Lk, D) in the order the cache holds them (apply a key order first).  Max-free: P = R16(2^s) of the pre-scaled
    scores, fp16 minus the first key tile's maximum (shift=False: attention_tiled's bounded mode, no shift); the denominator is the fp32 sum
    of the ROUNDED P (the matrix pipe sums the same 16-bit values the numerator multiplies).  A group of queries whose denominator leaves
    (l_min, 2^100) takes the exact path: running maximum on the same K', unrounded denominator.  out_f32: fp32 output (attn_xt)."""
    dt = q16.dtype
    D = q16.shape[-1]
    Lk = k.shape[-2]
    shift = dt == torch.float16 if shift is None else shift
    q, qa = rms_operand(q16, gq, dt)
    kp, ka = tiled_keys(k, gk, D ** -0.5 if scale is None else scale, dt)
    t, et = _scores(q, qa, kp, ka)
    if shift:
        M, em = _first_tile_shift(t, et, Lk)
    else:
        M = torch.zeros(t.shape[:-1] + (1,), dtype=t.dtype)
        em = torch.zeros_like(M)
    l_min = 2.0 ** -6 if shift else (2.0 ** -15 if dt == torch.float16 else 7.8886e-31)
    return _max_free(t, et, em, M, r16(v.double(), dt), dt, Lk, (l_min, 1.2676e30), TILED_GROUP[path], True, fallback,
                     None if out_f32 else dt)


def reference(*args, **kw):
    return model(*args, **kw)[0]


def bound(*args, **kw):
    return model(*args, **kw)[1]


def fp32_softmax(q16, k16, v16, scale=None, gq=None, gk=None):
    """The whole-tensor yardstick of the older tests: an fp32 softmax of the (normalised) operands."""
    dt = q16.dtype
    D = q16.shape[-1]
    q = rms_operand(q16, gq, dt)[0].float()
    k = rms_operand(k16, gk, dt)[0].float()
    a = torch.softmax((q @ k.transpose(-1, -2)) * (D ** -0.5 if scale is None else scale), dim=-1)
    return (a @ v16.float()).double()
