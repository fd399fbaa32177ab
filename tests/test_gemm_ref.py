"""The fp64 reference and error bound of the GEMM family (tests/gemm_ref.py) checked on the CPU before any GPU test relies on them: an
emulation of the kernel's arithmetic (exact products, fp32 accumulation per 32-deep MFMA k-step, fp32 epilogue, round-to-nearest-even
16-bit store) lies inside the bound, and each of the small bugs the bound exists to catch -- a truncating 16-bit store, a k-step of 32
dropped, the bias of the neighbouring column, the gate of the neighbouring row group -- lands outside it."""
import math

import pytest
import torch

import gemm_ref as G


def _r32(x):
    return x.to(torch.float32).double()


def _truncate16(x32: torch.Tensor, dt) -> torch.Tensor:
    """fp32 -> dt rounded toward zero (a store that drops the low bits instead of rounding)."""
    r = x32.to(dt)
    over = r.double().abs() > x32.double().abs()
    bits = r.view(torch.int16).clone()
    bits[over] -= 1                                   # sign-magnitude: one step toward zero
    return bits.view(dt)


def emulate(a16, w16, bias, epi, gate=None, rpg=1, x0=None, trunc=False, drop_step=None, bias_pair=False, gate_pair=False):
    """What gvf_gemm computes, on the CPU: each 32-deep k-step's exact sum added to an fp32 accumulator, then the fp32 epilogue and the
    16-bit store.  The keyword switches inject the perturbations."""
    dt = a16.dtype
    a, w = a16.double(), w16.double()
    M, K = a.shape
    N = w.shape[0]
    acc = torch.zeros((M, N), dtype=torch.float64)
    for s in range(K // 32):
        if s == drop_step:
            continue
        acc = _r32(acc + a[:, 32 * s:32 * s + 32] @ w[:, 32 * s:32 * s + 32].T)
    b = torch.zeros(N, dtype=torch.float64) if bias is None else bias.double()
    if bias_pair:
        b = b[torch.arange(N) & ~1]
    v = _r32(acc + b).float()
    store = (lambda x: _truncate16(x, dt)) if trunc else (lambda x: x.to(dt))
    if epi == G.EPI_STORE_16:
        return store(v)
    if epi == G.EPI_STORE_F32:
        return v
    if epi == G.EPI_GELU_16:
        u = 0.7978845608028654 * (v + 0.044715 * v * v * v)
        return store(v / (1.0 + torch.exp(-2.0 * u)))
    if epi == G.EPI_RESID_F32:
        rows = torch.arange(M)
        if gate_pair:
            rows = rows & ~1
        g = torch.ones((M, N)) if gate is None else gate[:, :N][rows // rpg]
        return x0 + g * v
    if epi == G.EPI_GEGLU_16:
        q = v.view(M, N // 64, 2, 32)
        vv = q[:, :, 0].reshape(M, N // 2).to(dt).float()
        gg = q[:, :, 1].reshape(M, N // 2).to(dt).float()
        return store(vv * (0.5 * gg * (1.0 + torch.erf(gg * 0.70710678118654752440))))
    raise ValueError(epi)


def _operands(dt, M, N, K, seed):
    g = torch.Generator().manual_seed(seed)
    a16 = torch.randn((M, K), generator=g).to(dt)
    w16 = (torch.randn((N, K), generator=g) / math.sqrt(K)).to(dt)
    bias = torch.randn((N,), generator=g)
    gate = torch.randn(((M + 6) // 7 + 1, N + 3), generator=g)
    x0 = torch.randn((M, N), generator=g)
    return a16, w16, bias, gate, x0


EPIS = [G.EPI_STORE_16, G.EPI_GELU_16, G.EPI_STORE_F32, G.EPI_RESID_F32, G.EPI_GEGLU_16]


@pytest.mark.parametrize("dt", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("M,N,K", [(67, 192, 96), (33, 128, 1056), (5, 64, 32)])
@pytest.mark.parametrize("epi", EPIS)
def test_correctly_rounded_result_is_inside_the_bound(dt, M, N, K, epi):
    a16, w16, bias, gate, x0 = _operands(dt, M, N, K, M + K + epi)
    for rpg, gt in ((7, gate), (1, None)):
        out = emulate(a16, w16, bias, epi, gate=gt, rpg=rpg, x0=x0)
        ref, bnd = G.model(a16, w16, bias, epi, gate=gt, rpg=rpg, x0=x0)
        n_bad, worst = G.excess(out, ref, bnd)
        assert n_bad == 0, (n_bad, worst)


@pytest.mark.parametrize("dt", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("epi", [G.EPI_STORE_16, G.EPI_GELU_16, G.EPI_GEGLU_16])
@pytest.mark.parametrize("K", [32, 2048])
def test_truncating_store_is_outside_the_bound(dt, epi, K):
    a16, w16, bias, _, x0 = _operands(dt, 64, 128, K, 11 + K)
    ref, bnd = G.model(a16, w16, bias, epi)
    n_bad, _ = G.excess(emulate(a16, w16, bias, epi, trunc=True), ref, bnd)
    assert n_bad > 0.05 * ref.numel(), n_bad


@pytest.mark.parametrize("dt", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("epi", EPIS)
@pytest.mark.parametrize("K,step", [(32, 0), (1056, 32), (512, 3)])
def test_dropped_k_step_is_outside_the_bound(dt, epi, K, step):
    a16, w16, bias, gate, x0 = _operands(dt, 40, 128, K, 5 + K)
    ref, bnd = G.model(a16, w16, bias, epi, gate=gate, rpg=7, x0=x0)
    n_bad, _ = G.excess(emulate(a16, w16, bias, epi, gate=gate, rpg=7, x0=x0, drop_step=step), ref, bnd)
    assert n_bad > 0.5 * ref.numel(), n_bad


@pytest.mark.parametrize("dt", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("epi", EPIS)
def test_bias_of_the_neighbouring_column_is_outside_the_bound(dt, epi):
    a16, w16, bias, gate, x0 = _operands(dt, 40, 192, 96, 21)
    ref, bnd = G.model(a16, w16, bias, epi, gate=gate, rpg=7, x0=x0)
    out = emulate(a16, w16, bias, epi, gate=gate, rpg=7, x0=x0, bias_pair=True)
    d = (out.double() - ref).abs() > bnd
    # every odd column is wrong (GEGLU: output column 32 b + i reads projection rows 64 b + i and 64 b + 32 + i, odd with i)
    cols = d.any(0)
    assert bool(cols[1::2].all()), cols


@pytest.mark.parametrize("dt", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("rpg", [1, 7])
def test_gate_of_the_neighbouring_row_group_is_outside_the_bound(dt, rpg):
    M = 64
    a16, w16, bias, gate, x0 = _operands(dt, M, 128, 96, 31)
    gate = torch.randn((M // rpg + 1, 131), generator=torch.Generator().manual_seed(3))
    ref, bnd = G.model(a16, w16, bias, G.EPI_RESID_F32, gate=gate, rpg=rpg, x0=x0)
    out = emulate(a16, w16, bias, G.EPI_RESID_F32, gate=gate, rpg=rpg, x0=x0, gate_pair=True)
    rows = ((out.double() - ref).abs() > bnd).any(1)
    moved = (torch.arange(M) // rpg) != ((torch.arange(M) & ~1) // rpg)     # the rows whose gate row the bug changes
    assert bool(moved.any()) and torch.equal(rows, moved)


@pytest.mark.parametrize("dt", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("adaln", [False, True])
def test_layernorm_operand_of_the_fp32_kernel_arithmetic_is_inside_its_band(dt, adaln):
    """ln_operand: the kernel's fp32 LayerNorm (statistics from 64-column partial sums added in fp32, one-pass variance, fused multiply-adds),
    emulated here in fp32, rounds to a 16-bit value inside [a16 - amb, a16 + amb] -- and amb is zero almost everywhere."""
    M, K, rpg = 48, 512, 16
    g = torch.Generator().manual_seed(7)
    X = (0.5 + 2.0 * torch.randn((M, K), generator=g)).float()
    ln_w, ln_b = 1.0 + 0.1 * torch.randn(K, generator=g), 0.1 * torch.randn(K, generator=g)
    shift, scale = (0.2 * torch.randn((M // rpg, K), generator=g), 0.2 * torch.randn((M // rpg, K), generator=g)) if adaln else (None, None)
    parts = X.view(M, K // 64, 64)
    psum, psq = parts.sum(-1), (parts * parts).sum(-1)
    s_, q_ = torch.zeros(M), torch.zeros(M)
    for p in range(K // 64):                           # the kernel adds the parts one by one in fp32
        s_, q_ = s_ + psum[:, p], q_ + psq[:, p]
    mean = s_ / K
    var = torch.clamp(q_ / K - mean * mean, min=0.0)
    rstd = torch.rsqrt(var + 1e-6)
    sv, tv = ln_w[None].expand(M, K), ln_b[None].expand(M, K)
    if adaln:
        gi = torch.arange(M) // rpg
        sc = 1.0 + scale[gi]
        sv, tv = sv * sc, tv * sc + shift[gi]
    y = X * rstd[:, None] + (-mean * rstd)[:, None]
    k16 = (y * sv + tv).to(dt)
    a16, amb = G.ln_operand(X, K // 64, dt, 1e-6, ln_w, ln_b, shift, scale, rpg)
    d = (k16.double() - a16.double()).abs()
    assert bool((d <= amb).all()), float((d - amb).max())
    assert float((amb > 0).double().mean()) < 0.05
