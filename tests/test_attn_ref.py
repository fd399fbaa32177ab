"""The fp64 reference and error bound of the attention family (tests/attn_ref.py) checked on the CPU before any GPU test relies on them: an fp32
emulation of each path of csrc/attn.hip (exact 16-bit products, fp32 accumulation per 16-deep MFMA step, the path's maximum / shift, v_exp
in fp32, 16-bit probabilities, the path's denominator, reciprocal and 16-bit store) lies inside the bound, in tile order and with another
legal summation order inside the MFMA; and each of the small bugs the bound exists to catch lands outside it: the last valid key of a
partial tile dropped, two V rows exchanged across a tile boundary, probabilities truncated instead of rounded, the denominator of the other
rounding point, keys rounded before the pre-scale, one RMS gain channel ignored."""
import math

import pytest
import torch

import attn_ref as A

DTYPES = [torch.bfloat16, torch.float16]


def _r32(x):
    return x.to(torch.float32).double()


def _truncate16(x32: torch.Tensor, dt) -> torch.Tensor:
    """fp32 -> dt rounded toward zero (a conversion that drops the low bits instead of rounding)."""
    r = x32.to(dt)
    over = r.double().abs() > x32.double().abs()
    bits = r.view(torch.int16).clone()
    bits[over] -= 1
    return bits.view(dt)


def _rms32(x16, g, dt, skip_channel=None):
    """The kernels' fused MultiHeadRMSNorm in fp32: x / max(sqrt(sum x^2), 1e-12) * sqrt(D) * g, rounded to dt."""
    if g is None:
        return x16
    x = x16.float()
    D = x.shape[-1]
    g = g.clone()
    if skip_channel is not None:
        g[:, skip_channel] = 1.0
    inv = torch.tensor(math.sqrt(D), dtype=torch.float32) / torch.sqrt((x * x).sum(-1, keepdim=True)).clamp_min(1e-12)
    return (x * inv * g[:, None, :]).to(dt)


def _mfma(a, b, split):
    """fp32 a @ b^T (16-bit operands as float64) over 16-deep MFMA steps: each step's exact sum added to the fp32 accumulator; split: the
    step's 16 products reduced as two rounded halves of 8 (another order the matrix pipe may use)."""
    acc = torch.zeros(a.shape[:-1] + (b.shape[-2],), dtype=torch.float64)
    for s in range(0, a.shape[-1], 16):
        if split:
            h0 = _r32(a[..., s:s + 8] @ b[..., s:s + 8].transpose(-1, -2))
            h1 = _r32(a[..., s + 8:s + 16] @ b[..., s + 8:s + 16].transpose(-1, -2))
            acc = _r32(acc + _r32(h0 + h1))
        else:
            acc = _r32(acc + a[..., s:s + 16] @ b[..., s:s + 16].transpose(-1, -2))
    return acc


def _pv(o, P16, v, split):
    """o (fp32) += P16 @ v over 16-key MFMA steps."""
    for j in range(0, P16.shape[-1], 16):
        o = _r32(o + _mfma_step(P16[..., j:j + 16], v[..., j:j + 16, :], split))
    return o


def _mfma_step(P, v, split):
    if not split:
        return P @ v
    return _r32(P[..., :8] @ v[..., :8, :]) + _r32(P[..., 8:] @ v[..., 8:, :])


def _store_p(p32, dt, trunc):
    return (_truncate16(p32, dt) if trunc else p32.to(dt)).double()


def _exp2(x):
    return torch.exp2(x.to(torch.float32)).double()


def _epilogue(o, l, dt):
    return (o * _r32(1.0 / l)).to(torch.float32).to(dt)


def emulate_stream(q, k, v, Lk, c, dt, split=False, trunc=False, den_rounded=False, drop_last=False):
    """attn_fwd_kernel on normalised 16-bit operands q (P, Lq, D), k / v (P, Lk, D) as float64, c = scale log2 e in fp32."""
    s = _mfma(q, k, split)
    valid = torch.arange(Lk) < (Lk - 1 if drop_last else Lk)
    nt = (Lk + A.KT - 1) // A.KT
    m = torch.full(s.shape[:-1] + (1,), -math.inf, dtype=torch.float64)
    l = torch.zeros_like(m)
    o = torch.zeros(q.shape[:-1] + (v.shape[-1],), dtype=torch.float64)
    for t in range(nt):
        j0, j1 = t * A.KT, min(Lk, (t + 1) * A.KT)
        st = s[..., j0:j1].masked_fill(~valid[j0:j1], -math.inf)
        mloc = _r32(st.amax(-1, keepdim=True) * c)
        m_new = torch.maximum(m, mloc)
        alpha = _exp2(_r32(m - m_new)).nan_to_num(0.0)
        l, o, m = _r32(l * alpha), _r32(o * alpha), m_new
        p = _exp2(_r32(st * c - m)).masked_fill(~valid[j0:j1], 0.0)
        l = _r32(l + p.float().sum(-1, keepdim=True).double())
        P16 = _store_p(p, dt, trunc)
        if den_rounded:
            l = _r32(l + P16.sum(-1, keepdim=True) - p.float().sum(-1, keepdim=True).double())
        o = _pv(o, P16, v[..., j0:j1, :], split)
    return _epilogue(o, l, dt)


def emulate_small(q, k, v, c, dt, split=False, trunc=False, den_rounded=False, drop_last=False):
    """attn_small_kernel: one maximum over all keys, exp2f(fl(s c) - fl(m c))."""
    Lk = k.shape[-2]
    s = _mfma(q, k, split)
    valid = torch.arange(Lk) < (Lk - 1 if drop_last else Lk)
    s = s.masked_fill(~valid, -math.inf)
    ms = _r32(s.amax(-1, keepdim=True) * c)
    p = _exp2(_r32(_r32(s * c) - ms))
    P16 = _store_p(p, dt, trunc)
    l = _r32((P16 if den_rounded else p).float().sum(-1, keepdim=True).double())
    o = _pv(torch.zeros(q.shape[:-1] + (v.shape[-1],), dtype=torch.float64), P16, v, split)
    return _epilogue(o, l, dt)


def emulate_kvres(q, kn, v, c, dt, split=False, trunc=False, den_rounded=False, drop_last=False, round_first=False):
    """attn_kvres_kernel: K' = R16(fl32(c k)) staged once, no maximum (fp16: minus the first tile's maximum, zero-padded keys included), the
    range guard per 32-query wave and the exact re-run on K' with c = 1.  round_first: the scores of the unscaled keys, scaled afterwards."""
    Lk = kn.shape[-2]
    kp = kn if round_first else kn.float().mul(torch.tensor(c, dtype=torch.float32)).to(dt).double()
    s = _mfma(q, kp, split)
    if round_first:
        s = _r32(s * c)
    valid = torch.arange(Lk) < (Lk - 1 if drop_last else Lk)
    if dt == torch.float16:
        sh = s[..., :A.KT].amax(-1, keepdim=True)
        if Lk < A.KT:
            sh = sh.clamp_min(0.0)
        s = _r32(s - sh)
    p = _exp2(s).masked_fill(~valid, 0.0)
    P16 = _store_p(p, dt, trunc)
    l = torch.zeros(p.shape[:-1] + (1,), dtype=torch.float64)
    o = torch.zeros(q.shape[:-1] + (v.shape[-1],), dtype=torch.float64)
    for t in range(0, Lk, A.KT):
        l = _r32(l + (P16 if den_rounded else p)[..., t:t + A.KT].float().sum(-1, keepdim=True).double())
        o = _pv(o, P16[..., t:t + A.KT], v[..., t:t + A.KT, :], split)
    out = _epilogue(o, l, dt)
    lo, hi = A.KVRES_RANGE[dt]
    Lq = q.shape[-2]
    bad = ~((l > lo) & (l < hi))[..., 0]
    nw = (Lq + 31) // 32
    wave = torch.nn.functional.pad(bad, (0, nw * 32 - Lq)).view(bad.shape[0], nw, 32).any(-1).repeat_interleave(32, -1)[:, :Lq]
    if bool(wave.any()):
        ex = emulate_stream(q, kp, v, Lk, 1.0, dt, split, trunc, den_rounded, drop_last)
        out = torch.where(wave[..., None], ex, out)
    return out


def emulate_tiled(q, k32, v32, gk, scale, dt, group, shift, split=False, trunc=False, den_unrounded=False, drop_last=False):
    """attn_xt / attn_xt64 on the cache attn_pack_kv* packs from fp32 kv rows: K' = R16(fl32(k c)) (gains: k fl32(c sqrt(D) / |k|) g), V' =
    R16(v); P = R16(2^s), fp16 minus the first tile's maximum; the denominator sums the ROUNDED P; a group whose denominator leaves the
    range re-runs exactly.  den_unrounded: the denominator of the unrounded p (the other paths' rounding point)."""
    Lk = k32.shape[-2]
    c = torch.tensor(scale * A.LOG2E, dtype=torch.float32)
    if gk is None:
        kp = (k32 * c).to(dt).double()
    else:
        D = k32.shape[-1]
        mul = c * torch.tensor(math.sqrt(D), dtype=torch.float32) / torch.sqrt((k32 * k32).sum(-1, keepdim=True)).clamp_min(1e-12)
        kp = (k32 * mul * gk[:, None, :]).to(dt).double()
    v = v32.to(dt).double()
    s = _mfma(q, kp, split)
    valid = torch.arange(Lk) < (Lk - 1 if drop_last else Lk)
    if shift:
        sh = s[..., :A.KT].amax(-1, keepdim=True)
        if Lk < A.KT:
            sh = sh.clamp_min(0.0)
        s = _r32(s - sh)
    p = _exp2(s).masked_fill(~valid, 0.0)
    P16 = _store_p(p, dt, trunc)
    l = torch.zeros(p.shape[:-1] + (1,), dtype=torch.float64)
    o = torch.zeros(q.shape[:-1] + (v.shape[-1],), dtype=torch.float64)
    for t in range(0, Lk, A.KT):
        l = _r32(l + (p if den_unrounded else P16)[..., t:t + A.KT].float().sum(-1, keepdim=True).double())
        o = _pv(o, P16[..., t:t + A.KT], v[..., t:t + A.KT, :], split)
    out = _epilogue(o, l, dt)
    lo = 2.0 ** -6 if shift else (2.0 ** -15 if dt == torch.float16 else 7.8886e-31)
    Lq = q.shape[-2]
    bad = ~((l > lo) & (l < 1.2676e30))[..., 0]
    nw = (Lq + group - 1) // group
    grp = torch.nn.functional.pad(bad, (0, nw * group - Lq)).view(bad.shape[0], nw, group).any(-1).repeat_interleave(group, -1)[:, :Lq]
    if bool(grp.any()):
        out = torch.where(grp[..., None], emulate_stream(q, kp, v, Lk, 1.0, dt, split, trunc, False, drop_last), out)
    return out


def run_tiled(path, q16, k32, v32, gq, gk, shift=None, **mut):
    dt = q16.dtype
    D = q16.shape[-1]
    shift = dt == torch.float16 if shift is None else shift
    out = emulate_tiled(_rms32(q16, gq, dt).double(), k32, v32, gk, D ** -0.5, dt, A.TILED_GROUP[path], shift, **mut)
    ref, bnd = A.model_tiled(q16, k32, v32, path, gq=gq, gk=gk, shift=shift)
    return out, ref, bnd


TILED = [("xt", 300, 1370, 32), ("xt", 40, 77, 32), ("xt", 64, 4097, 32), ("xt64", 130, 512, 64), ("xt64", 70, 33, 64)]


def _tiled_problem(dt, path, Lq, Lk, D, seed):
    g = torch.Generator().manual_seed(seed)
    q16 = (1.5 * torch.randn((2, Lq, D), generator=g)).to(dt)
    k32, v32 = 1.5 * torch.randn((2, Lk, D), generator=g), torch.randn((2, Lk, D), generator=g)
    gains = path == "xt"                                  # attn_pack_kv64 has no key gain
    gq = (1.0 + 0.3 * torch.randn((2, D), generator=g)) if gains else None
    gk = (1.0 + 0.3 * torch.randn((2, D), generator=g)) if gains else None
    return q16, k32, v32, gq, gk


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("path,Lq,Lk,D", TILED)
@pytest.mark.parametrize("split", [False, True])
def test_emulated_tiled_cache_is_inside_the_bound(dt, path, Lq, Lk, D, split):
    q16, k32, v32, gq, gk = _tiled_problem(dt, path, Lq, Lk, D, Lq + Lk)
    for shift in ([True, False] if dt == torch.float16 and path == "xt" else [None]):
        out, ref, bnd = run_tiled(path, q16, k32, v32, gq, gk, shift=shift, split=split)
        n_bad, worst = A.excess(out, ref, bnd)
        assert n_bad == 0, (shift, n_bad, worst)


# the denominator mutant at fp16 with 1370 keys stays below the output's resolution (see _mutant_cases)
@pytest.mark.parametrize("dt,path,Lq,Lk,D,mutant", [
    pytest.param(dt, path, Lq, Lk, D, m, id=f"{m}-{path}-{str(dt)[6:]}")
    for m in ("drop_last", "trunc", "den_unrounded") for dt in DTYPES for path, Lq, Lk, D in (("xt", 64, 1370, 32), ("xt64", 64, 447, 64))
    if not (m == "den_unrounded" and dt == torch.float16 and path == "xt")])
def test_tiled_cache_mutant_is_outside_the_bound(dt, path, Lq, Lk, D, mutant):
    """The tiled caches' own rounding point is the reverse of the other paths': a denominator of the UNROUNDED p lands outside."""
    q16, k32, v32, gq, gk = _tiled_problem(dt, path, Lq, Lk, D, 7 + Lk)
    out, ref, bnd = run_tiled(path, q16, k32, v32, gq, gk, **{mutant: True})
    assert A.excess(out, ref, bnd)[0] > 0, mutant


def _problem(dt, P, Lq, Lk, D, seed, gains=(False, False), score_mul=1.0):
    g = torch.Generator().manual_seed(seed)
    q16 = (score_mul * torch.randn((P, Lq, D), generator=g)).to(dt)
    k16 = torch.randn((P, Lk, D), generator=g).to(dt)
    v16 = torch.randn((P, Lk, D), generator=g).to(dt)
    gq = (1.0 + 0.3 * torch.randn((P, D), generator=g)) if gains[0] else None
    gk = (1.0 + 0.3 * torch.randn((P, D), generator=g)) if gains[1] else None
    return q16, k16, v16, gq, gk


def run(path, q16, k16, v16, gq, gk, scale=None, skip_gain=None, swap=None, **mut):
    """(emulated output, reference, bound) of one path; skip_gain: the k gain channel the emulation ignores; swap: V rows (j, j + 1) exchanged
    in the emulation."""
    dt = q16.dtype
    D = q16.shape[-1]
    c = A.c32(D ** -0.5 if scale is None else scale)
    q = _rms32(q16, gq, dt).double()
    kn = _rms32(k16, gk, dt, skip_gain).double()
    v = v16.double()
    if swap is not None:
        v = v.clone()
        v[:, [swap, swap + 1]] = v[:, [swap + 1, swap]]
    if path == "stream":
        out = emulate_stream(q, kn, v, k16.shape[-2], c, dt, **mut)
    elif path == "small":
        out = emulate_small(q, kn, v, c, dt, **mut)
    else:
        out = emulate_kvres(q, kn, v, c, dt, **mut)
    ref, bnd = A.model(q16, k16, v16, path, scale=scale, gq=gq, gk=gk)
    return out, ref, bnd


# (path, Lq, Lk, D): partial and full 64-key tiles, one and many tiles, both head dims
SHAPES = [("stream", 33, 1, 32), ("stream", 40, 65, 64), ("stream", 129, 130, 32), ("stream", 20, 1370, 32), ("stream", 8, 513, 64),
          ("small", 24, 24, 32), ("small", 32, 1, 32), ("small", 1, 32, 32),
          ("kvres", 70, 33, 32), ("kvres", 64, 512, 64), ("kvres", 40, 127, 32), ("kvres", 33, 64, 64)]


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("path,Lq,Lk,D", SHAPES)
@pytest.mark.parametrize("split", [False, True])
def test_emulated_kernel_is_inside_the_bound(dt, path, Lq, Lk, D, split):
    for gains, scale in (((False, False), None), ((True, True), 0.05), ((True, False), 1.0), ((False, True), None)):
        q16, k16, v16, gq, gk = _problem(dt, 2, Lq, Lk, D, Lq * 7 + Lk + D, gains)
        out, ref, bnd = run(path, q16, k16, v16, gq, gk, scale, split=split)
        n_bad, worst = A.excess(out, ref, bnd)
        assert n_bad == 0, (gains, scale, n_bad, worst)


@pytest.mark.parametrize("dt", DTYPES)
def test_kvres_range_guard_takes_the_exact_path(dt):
    """Scores far outside the max-free range: the emulated wave falls back, and the model follows it (fallback=None) -- the fast model would not
    hold the result."""
    q16, k16, v16, gq, gk = _problem(dt, 2, 64, 100, 32, 5, score_mul=60.0)
    out, ref, bnd = run("kvres", q16, k16, v16, gq, gk)
    assert A.excess(out, ref, bnd)[0] == 0
    ref_f, bnd_f = A.model(q16, k16, v16, "kvres", fallback=False)
    assert not torch.isfinite(ref_f).all() or A.excess(out, ref_f, bnd_f)[0] > 0


MUTANT_SHAPES = [("stream", 64, 1370, 32), ("stream", 64, 190, 64), ("small", 32, 27, 32), ("kvres", 64, 447, 64), ("kvres", 64, 130, 32)]
MUTANTS = {"drop_last": {"drop_last": True}, "swap": {"swap": 63}, "trunc": {"trunc": True}, "den_rounded": {"den_rounded": True},
           "skip_gain": {"skip_gain": 5}, "round_first": {"round_first": True}}


def _mutant_cases():
    for mutant in MUTANTS:
        for dt in DTYPES:
            for path, Lq, Lk, D in MUTANT_SHAPES:
                if mutant == "swap" and Lk <= 64:                 # needs a tile boundary
                    continue
                if mutant == "round_first" and path != "kvres":   # the pre-scale exists on the K/V-resident path only
                    continue
                # a denominator of the rounded P differs from the unrounded sum by rounding errors that average out: fp16's (2^-11) stay below
                # the output's half ulp unless few keys carry the row -- the K/V-resident shape with 130 keys at scale 1
                if mutant == "den_rounded" and dt == torch.float16 and (path, Lk) != ("kvres", 130):
                    continue
                yield pytest.param(dt, path, Lq, Lk, D, mutant, id=f"{mutant}-{path}-{Lk}-{D}-{str(dt)[6:]}")


@pytest.mark.parametrize("dt,path,Lq,Lk,D,mutant", list(_mutant_cases()))
def test_mutant_is_outside_the_bound(dt, path, Lq, Lk, D, mutant):
    # the denominator's rounding point shows where a few probabilities carry the row: peaked scores (scale 1)
    scale = 1.0 if mutant == "den_rounded" else None
    q16, k16, v16, gq, gk = _problem(dt, 2, Lq, Lk, D, 3 + Lk, (True, True))
    out, ref, bnd = run(path, q16, k16, v16, gq, gk, scale, **MUTANTS[mutant])
    n_bad, worst = A.excess(out, ref, bnd)
    assert n_bad > 0, (mutant, worst)


def test_dropped_key_passes_the_whole_tensor_bar():
    """Why the element-wise bound exists: with outputs of unit scale (values v = 1 + N(0, 1), RMS-normalised q and k: many keys share the
    weight) the stream kernel with the last key of Lk = 1370 dropped stays inside the bars of test_attention_matches_oracle against an fp32
    softmax (rel_l2 < 6e-3, max |err| < 3e-2 max |ref|), while more than a thousand elements leave the bound."""
    dt = torch.bfloat16
    q16, k16, v16, gq, gk = _problem(dt, 4, 130, 1370, 32, 0, (True, True))
    v16 = (v16.float() + 1.0).to(dt)
    out, ref, bnd = run("stream", q16, k16, v16, gq, gk, drop_last=True)
    soft = A.fp32_softmax(q16, k16, v16, gq=gq, gk=gk)
    rel = float((out.double() - soft).norm() / soft.norm())
    assert rel < 6e-3 and float((out.double() - soft).abs().max()) < 3e-2 * float(soft.abs().max()), rel
    assert A.excess(out, ref, bnd)[0] > 1000


@pytest.mark.parametrize("dt", DTYPES)
def test_normalised_operand_ambiguity_is_rare(dt):
    q16, _, _, gq, _ = _problem(dt, 4, 256, 1, 64, 9, (True, False))
    ref, amb = A.rms_operand(q16, gq, dt)
    assert bool(((_rms32(q16, gq, dt).double() - ref).abs() <= amb).all())
    assert float((amb > 0).double().mean()) < 0.01
